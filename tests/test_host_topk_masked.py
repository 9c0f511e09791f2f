"""ops.topk_rows restricted to candidates (allow words, per-row exclusion lists) off the GPU: the torch form equals a plain
restatement of the contract (csrc/topk.hip, mobgt_topk_rows_masked), pack_allow round-trips, the collator keeps x and y in one id
space (what exclude_visited relies on), and the C ABI entry point is declared."""
import os

import numpy as np
import pytest
import torch

from mobgt_amd import _lib, ops, synth
from mobgt_amd.data import DeviceCollator

SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0], np.float32)


def _unpack(words, V):
    w = words.long()
    return ((w[torch.arange(V) >> 5] >> (torch.arange(V) & 31)) & 1).bool()


def _plain(scores, k, col_offset, allow_mask, exclude, exclude_offset):
    """the contract, one row at a time: the candidate columns, their stable descending sort, padded with -1 / -inf"""
    G, V = scores.shape
    ids = torch.full((G, k), -1, dtype=torch.int64)
    vals = torch.full((G, k), float("-inf"))
    for g in range(G):
        ok = torch.ones(V, dtype=torch.bool) if allow_mask is None else allow_mask.clone()
        if exclude is not None:
            for p in exclude[g].tolist():
                c = p - exclude_offset
                if p != 0 and 0 <= c < V:
                    ok[c] = False
        cols = torch.nonzero(ok).flatten()
        v, o = torch.sort(scores[g, cols], descending=True, stable=True)
        m = min(k, cols.numel())
        ids[g, :m] = cols[o[:m]] + col_offset
        vals[g, :m] = v[:m]
    return ids, vals


def _bits(t):
    return t.contiguous().view(torch.int32)


def _scores(rng, G, V, kind):
    if kind == "random":
        return rng.standard_normal((G, V)).astype(np.float32)
    if kind == "ties":
        return rng.integers(-2, 3, (G, V)).astype(np.float32) * 0.5
    return rng.choice(SPECIAL, (G, V))


@pytest.mark.parametrize("V,k", [(5, 5), (40, 3), (70, 20), (300, 64)])
def test_cpu_masked_topk_is_the_plain_contract(V, k):
    rng = np.random.default_rng(V * 31 + k)
    G = 6
    for kind in ("random", "ties", "special"):
        s = torch.from_numpy(_scores(rng, G, V, kind))
        for density in (0.0, 0.1, 0.5, 1.0, None):
            mask = None if density is None else torch.from_numpy(rng.random(V) < density)
            allow = None if mask is None else ops.pack_allow(mask, V)
            for dt in (torch.int32, torch.int64, None):
                if dt is None:
                    exclude = None
                else:
                    # duplicates, padding 0, ids past V and below the offset; row 1 excludes every column; row 2 nothing
                    e = rng.integers(-3, V + 6, (G, V // 2 + 3))
                    e[:, ::4] = 0
                    e[:, 1] = e[:, 2]
                    e[2] = 0
                    exclude = torch.from_numpy(e).to(dt)
                    exclude = torch.cat([exclude, torch.zeros(G, V, dtype=dt)], 1)
                    exclude[1, -V:] = torch.arange(1, V + 1, dtype=dt)
                if allow is None and exclude is None:
                    continue
                for off in (0, 1):
                    ids, vals = ops.topk_rows(s, k, col_offset=off, allow=allow, exclude=exclude)
                    wi, wv = _plain(s, k, off, mask, exclude, off)
                    tag = (kind, density, dt, off)
                    assert torch.equal(ids, wi), tag
                    assert torch.equal(_bits(vals), _bits(wv)), tag


def test_cpu_masked_topk_rows_with_few_candidates_pad():
    s = torch.tensor([[0.0, 2.0, -0.0, 2.0, float("nan"), float("-inf"), 1.0]] * 3)
    excl = torch.tensor([[2, 0, 99], [0, 0, 0], [1, 2, 3]])
    allow = ops.pack_allow(torch.tensor([0, 1, 5, 6]), 7)           # columns 0, 1, 5, 6
    ids, vals = ops.topk_rows(s, 5, col_offset=10, allow=allow, exclude=excl, exclude_offset=1)
    # row 0 loses column 1 (id 2): 6 (1.0), 0 (0.0), 5 (-inf, a real candidate), then padding
    assert ids.tolist() == [[16, 10, 15, -1, -1], [11, 16, 10, 15, -1], [16, 15, -1, -1, -1]]
    assert torch.equal(vals[0, 2:], torch.full((3,), float("-inf")))
    # exclude_offset defaults to col_offset
    a = ops.topk_rows(s[:1], 3, col_offset=1, exclude=torch.tensor([[2]]))
    b = ops.topk_rows(s[:1], 3, col_offset=1, exclude=torch.tensor([[2]]), exclude_offset=1)
    assert torch.equal(a[0], b[0]) and 1 not in (a[0] - 1).tolist()


def test_cpu_masked_topk_writes_into_out():
    s = torch.randn(4, 50)
    out = (torch.empty(4, 7, dtype=torch.int64), torch.empty(4, 7))
    exclude = torch.randint(0, 51, (4, 9))
    got = ops.topk_rows(s, 7, col_offset=1, out=out, exclude=exclude)
    assert got[0] is out[0] and got[1] is out[1]
    wi, wv = _plain(s, 7, 1, None, exclude, 1)
    assert torch.equal(out[0], wi) and torch.equal(out[1], wv)


def test_pack_allow_round_trips():
    rng = np.random.default_rng(5)
    for V in (1, 31, 32, 33, 1000, 3680):
        for density in (0.0, 0.3, 1.0):
            mask = torch.from_numpy(rng.random(V) < density)
            w = ops.pack_allow(mask, V)
            assert w.dtype == torch.int32 and w.shape == ((V + 31) // 32,)
            assert torch.equal(_unpack(w, V), mask)
        ids = torch.from_numpy(rng.integers(1, V + 1, 2 * V))           # label space, offset 1, with duplicates
        want = torch.zeros(V, dtype=torch.bool)
        want[ids - 1] = True
        assert torch.equal(_unpack(ops.pack_allow(ids, V, offset=1), V), want)
        assert torch.equal(ops.pack_allow(ids, V, offset=1), ops.pack_allow(want, V))
    assert torch.equal(ops.pack_allow(torch.ones(64, dtype=torch.bool), 64), torch.full((2,), -1, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.pack_allow(torch.tensor([0, 5]), 5, offset=1)                # id 0 is column -1
    with pytest.raises(ValueError):
        ops.pack_allow(torch.tensor([6]), 5, offset=1)                   # column 5 of 5
    with pytest.raises(ValueError):
        ops.pack_allow(torch.ones(4, dtype=torch.bool), 5)


def test_collator_keeps_x_and_y_in_one_id_space():
    """exclude_visited compares batched_data.x with the label space of y: the collator stores node_name and target unchanged."""
    trajs = synth.make_batch_of_trajectories(seed=3, G=5, P=200, n_user=10, n_nodes=[4, 9, 1, 17, 6])
    h = DeviceCollator("cpu").pack_host(trajs)
    for g, t in enumerate(trajs):
        n = len(t["node_name"])
        assert np.array_equal(h["x"][g, :n, 0], np.asarray(t["node_name"]))
        assert (h["x"][g, n:, 0] == 0).all()                            # padding is 0, never a POI id (ids start at 1)
        assert int(h["y"][g]) == int(t["target"][0])
        assert min(t["node_name"]) >= 1


def test_masked_topk_entry_point_is_declared():
    assert "mobgt_topk_rows_masked" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mobgt_topk_rows_masked"][1]) == 16
    hdr = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "mobgt_hip.h")).read()
    assert "int mobgt_topk_rows_masked(" in hdr
