"""The fresh-batch path's host-side structure: the one-batch-ahead pipeline's order (train._StagedBatches._pipeline) and the
byte layout of a bucket's buffers (data.RawLayout / data.BatchLayout) against recorded literals.  No GPU, no torch device."""
import numpy as np
import pytest

from mobgt_amd.data import BatchLayout, RawLayout
from mobgt_amd.train import _StagedBatches


class _Logged(_StagedBatches):
    """Staging that only logs; batch `empty` stages to None (every sample filtered out)."""

    def __init__(self, empty=None):
        self.log, self.empty = [], empty

    def _stage(self, ids):
        self.log.append(("stage", ids[0]))
        return None if ids[0] == self.empty else ("slot%d" % ids[0], "st%d" % ids[0])


def _run(n, empty=None):
    loop = _Logged(empty)
    batches = [[j, 100 + j] for j in range(n)]

    def launch(j, slot, st):
        loop.log.append(("launch", j, slot, st))
        return "loss%d" % j

    handed = []
    for item in loop._pipeline(batches, launch):
        loop.log.append(("caller", item[0]))
        handed.append(item)
    return loop.log, handed


def test_pipeline_launches_then_stages_the_next_batch_then_hands_over():
    log, handed = _run(3)
    assert log == [("stage", 0), ("launch", 0, "slot0", "st0"), ("stage", 1), ("caller", 0),
                   ("launch", 1, "slot1", "st1"), ("stage", 2), ("caller", 1),
                   ("launch", 2, "slot2", "st2"), ("caller", 2)]                     # nothing is staged behind the last batch
    assert handed == [(j, [j, 100 + j], ("slot%d" % j, "st%d" % j), "loss%d" % j) for j in range(3)]


def test_pipeline_skips_the_launch_of_an_empty_batch_but_hands_it_over():
    log, handed = _run(3, empty=1)
    assert log == [("stage", 0), ("launch", 0, "slot0", "st0"), ("stage", 1), ("caller", 0),
                   ("stage", 2), ("caller", 1),
                   ("launch", 2, "slot2", "st2"), ("caller", 2)]
    assert handed[1] == (1, [1, 101], None, None) and handed[2][3] == "loss2"
    log, handed = _run(1, empty=0)
    assert log == [("stage", 0), ("caller", 0)] and handed == [(0, [0, 100], None, None)]


def test_pipeline_over_no_batches_does_nothing():
    assert _run(0) == ([], [])


# (name, offset, bytes) of every field in placement order, and the totals, as the layouts stood before they shared one
# placement routine
LAYOUTS = {
    (1, 1, 20): dict(
        raw=(('y', 0, 8), ('idx', 16, 8), ('counts', 32, 4), ('x', 48, 4), ('time', 64, 4), ('cat', 80, 4), ('time_normal', 96, 4), ('n_nodes', 112, 4), ('user', 128, 4)), raw_nbytes=144,
        batch=(('y', 0, 8), ('idx', 16, 8), ('counts', 32, 4), ('x', 48, 4), ('time', 64, 4), ('cat', 80, 4), ('time_normal', 96, 4), ('n_nodes', 112, 4), ('user', 128, 4), ('attn_bias', 144, 16), ('rel_pos', 160, 2), ('poi_pos', 176, 2), ('edge_input', 192, 20), ('in_degree', 224, 2), ('out_degree', 240, 2), ('spd', 256, 2), ('path', 272, 2)), raw_bytes=144, copy_bytes=256, nbytes=288),
    (3, 5, 20): dict(
        raw=(('y', 0, 24), ('idx', 32, 24), ('counts', 64, 300), ('x', 368, 60), ('time', 432, 60), ('cat', 496, 60), ('time_normal', 560, 60), ('n_nodes', 624, 12), ('user', 640, 12)), raw_nbytes=656,
        batch=(('y', 0, 24), ('idx', 32, 24), ('counts', 64, 300), ('x', 368, 60), ('time', 432, 60), ('cat', 496, 60), ('time_normal', 560, 60), ('n_nodes', 624, 12), ('user', 640, 12), ('attn_bias', 656, 432), ('rel_pos', 1088, 150), ('poi_pos', 1248, 150), ('edge_input', 1408, 1500), ('in_degree', 2912, 30), ('out_degree', 2944, 30), ('spd', 2976, 150), ('path', 3136, 150)), raw_bytes=656, copy_bytes=2976, nbytes=3296),
    (16, 65, 20): dict(
        raw=(('y', 0, 128), ('idx', 128, 128), ('counts', 256, 270400), ('x', 270656, 4160), ('time', 274816, 4160), ('cat', 278976, 4160), ('time_normal', 283136, 4160), ('n_nodes', 287296, 64), ('user', 287360, 64)), raw_nbytes=287424,
        batch=(('y', 0, 128), ('idx', 128, 128), ('counts', 256, 270400), ('x', 270656, 4160), ('time', 274816, 4160), ('cat', 278976, 4160), ('time_normal', 283136, 4160), ('n_nodes', 287296, 64), ('user', 287360, 64), ('attn_bias', 287424, 278784), ('rel_pos', 566208, 135200), ('poi_pos', 701408, 135200), ('edge_input', 836608, 1352000), ('in_degree', 2188608, 2080), ('out_degree', 2190688, 2080), ('spd', 2192768, 135200), ('path', 2327968, 135200)), raw_bytes=287424, copy_bytes=2192768, nbytes=2463168),
}


@pytest.mark.parametrize("G,N,D", sorted(LAYOUTS))
def test_layouts_are_byte_identical_to_the_recorded_ones(G, N, D):
    want = LAYOUTS[G, N, D]
    raw, lay = RawLayout(G, N), BatchLayout(G, N, D)
    assert tuple((k, o, n) for k, (o, n, _, _) in raw.offsets.items()) == want["raw"] and raw.nbytes == want["raw_nbytes"]
    assert tuple((k, o, n) for k, (o, n, _, _) in lay.offsets.items()) == want["batch"]
    assert (lay.raw_bytes, lay.copy_bytes, lay.nbytes) == (want["raw_bytes"], want["copy_bytes"], want["nbytes"])
    assert {k: v[:2] for k, v in raw.offsets.items()} == {k: lay.offsets[k][:2] for k in raw.offsets}
    if (G, N) == (3, 5):
        assert (lay.raw_bytes, lay.copy_bytes, lay.nbytes) == (656, 2976, 3296)
    # the host views cover the raw part only, the device views everything
    assert sorted(lay.views_np(np.zeros(lay.raw_bytes, dtype=np.uint8))) == sorted(raw.offsets)
    assert {k: v.shape for k, v in raw.views_np(np.zeros(raw.nbytes, dtype=np.uint8)).items()} == {k: v[3] for k, v in raw.offsets.items()}
