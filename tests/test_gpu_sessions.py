"""Check-in sessions on the device: `mobgt_sessions_to_raw` (csrc_data/sessions.hip, include/mobgt_data.h),
`data.SessionCollator` and the loops fed from a `data.SessionDataset`.

  * the kernel equals the host converter (`data.sessions_to_trajectories`, itself equal to the reference's gen_pickles on golden
    G12) in EVERY element of every output, padding included, over pre-poisoned buffers: G12, seeded batches, history lengths
    around the wave / workgroup / LDS-count boundaries with 5 POIs (every increment on a few cells) and with all-distinct POIs,
    refused graphs inside a good batch, a captured launch replayed on changed inputs;
  * SessionCollator returns DeviceCollator's batch for the converted dicts, field by field, with a bin table and with
    coordinate bins;
  * PredictLoop / EvalLoop / EpochLoop from sessions stage, rank and list exactly what they do from the converted dicts, and
    refuse out-of-range indices on the host with the dict path's messages.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mobgt_amd import _lib_data, data, ops, synth, workloads                # noqa: E402
from mobgt_amd.data import DeviceCollator, SessionCollator, SessionDataset, bucket_nodes, sessions_to_trajectories   # noqa: E402
from mobgt_amd.train import EpochLoop, EvalLoop, PredictLoop                # noqa: E402

DEV = "cuda"
OUTS = ("counts", "x", "time", "cat", "time_normal", "n_nodes", "status")


# ------------------------------------------------------------------------------------------------ the kernel
def _expected(sessions, N, bad=()):
    """host reference, padded as DeviceCollator.pack_host pads; graphs in `bad` (index -> status) are all zero"""
    G = len(sessions)
    e = dict(counts=np.zeros((G, N, N), np.int32), x=np.zeros((G, N), np.int32), time=np.zeros((G, N), np.int32),
             cat=np.zeros((G, N), np.int32), time_normal=np.zeros((G, N), np.float32), n_nodes=np.zeros(G, np.int32),
             status=np.zeros(G, np.int32))
    for g, t in enumerate(sessions_to_trajectories(sessions)):
        if g in bad:
            e["status"][g] = bad[g]
            continue
        n = len(t["node_name"])
        e["counts"][g, :n, :n] = t["edge_type"]
        e["x"][g, :n], e["time"][g, :n], e["cat"][g, :n], e["time_normal"][g, :n] = t["node_name"], t["time"], t["cat"], t["time_normal"]
        e["n_nodes"][g] = n
    return e


def _device_io(sessions, N, Lp, lens=None):
    G = len(sessions)
    seq = np.full((G, Lp, 3), -7, np.int32)                            # (rows beyond len are never read: poison)
    ln = np.zeros(G, np.int32)
    for g, (_, c) in enumerate(sessions):
        L = min(len(c) - 1, Lp)
        seq[g, :L] = c[:L]
        ln[g] = len(c) - 1
    if lens is not None:
        ln[:] = lens
    ins = torch.from_numpy(seq).to(DEV), torch.from_numpy(ln).to(DEV)
    shapes = dict(counts=(G, N, N), x=(G, N), time=(G, N), cat=(G, N), time_normal=(G, N), n_nodes=(G,), status=(G,))
    outs = {k: torch.full(shapes[k], 0x7f7f7f7f, dtype=torch.int32, device=DEV) for k in OUTS}     # every element must be written
    return ins, outs


def _launch(ins, outs, G, Lp, N):
    _lib_data.launch("mobgt_sessions_to_raw", ops._p(ins[0]), ops._p(ins[1]), *[ops._p(outs[k]) for k in OUTS], G, Lp, N, ops._stream())


def _compare(outs, want, what):
    for k in OUTS:
        got = outs[k].cpu().numpy()
        w = want[k].view(np.int32) if k == "time_normal" else want[k]
        assert np.array_equal(got, w), (what, k, np.argwhere(got != w)[:4].tolist())


def _check(sessions, N=None, Lp=None, what=""):
    n_max = max(len(np.unique(c[:-1, 0])) for _, c in sessions)
    N = bucket_nodes(n_max) if N is None else N
    Lp = max(len(c) - 1 for _, c in sessions) + 3 if Lp is None else Lp
    ins, outs = _device_io(sessions, N, Lp)
    _launch(ins, outs, len(sessions), Lp, N)
    _compare(outs, _expected(sessions, N), what)


def _random_session(rng, L, P, distinct=False):
    poi = (rng.permutation(P)[:L + 1] + 1) if distinct else rng.randint(1, P + 1, L + 1)
    return int(rng.randint(0, 50)), np.stack([poi, rng.randint(0, 48, L + 1), rng.randint(1, 300, L + 1)], 1).astype(np.int32)


def test_kernel_equals_the_converter_on_g12(golden_dir):
    z = np.load(os.path.join(golden_dir, "g12_sessions.npz"))
    o = z["offsets"]
    sessions = [(int(z["users"][i]), z["checkins"][o[i]:o[i + 1]].astype(np.int32)) for i in range(len(z["users"]))]
    _check(sessions, what="g12")
    assert bucket_nodes(int(z["ref_num_node"].max())) > int(z["ref_num_node"].max())      # (padded beyond the longest graph)


@pytest.mark.parametrize("G", [1, 17])
def test_kernel_on_seeded_batches(G):
    rng = np.random.RandomState(100 + G)
    for P in (5, 50, 100000):                                          # ids up to 100 000
        sessions = [_random_session(rng, int(rng.randint(1, 200)), P) for _ in range(G)]
        _check(sessions, what=(G, P))
    _check([_random_session(rng, 40, 7) for _ in range(G)], N=7, Lp=40, what="odd N, no padding in Lp")


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_kernel_over_history_lengths(L):
    """5 distinct POIs: every transition lands on at most 25 cells (the LDS counting path, maximal contention); all-distinct
    POIs: n = L nodes, across the LDS / global counting threshold (64) and the 1024-thread workgroup (1025)."""
    rng = np.random.RandomState(L)
    few = _random_session(rng, L, 5)
    many = _random_session(rng, L, 100000, distinct=True)
    assert len(np.unique(many[1][:-1, 0])) == L
    _check([few], what=("few", L))
    _check([many], what=("distinct", L))
    _check([few, many, few], what=("mixed", L))


def test_kernel_mixes_short_and_long_and_contended_global_counts():
    rng = np.random.RandomState(9)
    _check([_random_session(rng, 1, 50), _random_session(rng, 300, 100000), _random_session(rng, 1, 50)], what="1 with 300")
    # 70 distinct POIs visited 3000 times: over the LDS threshold, so every increment is a global atomic on few cells
    _check([_random_session(rng, 3000, 70), _random_session(rng, 4096, 66)], Lp=4096, what="contended global")
    # the stated limits at once: 4096 check-ins, 4096 nodes (the longest backward scans, a 64 MB tile)
    _check([_random_session(rng, 4096, 100000, distinct=True)], N=_lib_data.MAX_N, Lp=_lib_data.MAX_LP, what="limits")


def test_refused_graphs_are_zero_and_leave_the_others_exact():
    rng = np.random.RandomState(12)
    sessions = [_random_session(rng, 30, 20), _random_session(rng, 40, 100000, distinct=True), _random_session(rng, 9, 5),
                _random_session(rng, 20, 8), _random_session(rng, 64, 20)]
    N, Lp = 32, 64                                                     # graph 1 has 40 > N distinct POIs
    lens = [30, 40, 0, 65, 64]                                         # graph 2: len 0; graph 3: len > Lp
    ins, outs = _device_io(sessions, N, Lp, lens=lens)
    _launch(ins, outs, 5, Lp, N)
    _compare(outs, _expected(sessions, N, bad={1: _lib_data.SNODES, 2: _lib_data.SBADLEN, 3: _lib_data.SBADLEN}), "refused")
    assert _lib_data.SNODES != 0 and _lib_data.SBADLEN != 0


def test_entry_point_refuses_bad_sizes():
    ins, outs = _device_io([_random_session(np.random.RandomState(0), 5, 9)], 8, 8)
    L = _lib_data.lib()
    args = [ops._p(ins[0]), ops._p(ins[1])] + [ops._p(outs[k]) for k in OUTS]
    for G, Lp, N in ((1, 0, 8), (1, _lib_data.MAX_LP + 1, 8), (1, 8, 0), (1, 8, _lib_data.MAX_N + 1), (-1, 8, 8)):
        assert L.mobgt_sessions_to_raw(*args, G, Lp, N, ops._stream()) == _lib_data.CONSTANTS["MOBGT_DATA_EBADDIM"], (G, Lp, N)
    assert L.mobgt_sessions_to_raw(*args, 0, 8, 8, ops._stream()) == 0                     # nothing to do
    assert L.mobgt_sessions_to_raw(None, *args[1:], 1, 8, 8, ops._stream()) == _lib_data.CONSTANTS["MOBGT_DATA_EALIGN"]
    with pytest.raises(_lib_data.MobgtDataError, match="EBADDIM"):
        _launch(ins, outs, 1, 0, 8)
    torch.cuda.synchronize()
    assert all(int(outs[k].view(-1)[0]) == 0x7f7f7f7f for k in OUTS)                      # a refused call launched nothing


def test_captured_launch_replays_on_changed_inputs():
    rng = np.random.RandomState(3)
    G, N, Lp = 6, 208, 200
    batches = [[_random_session(rng, int(rng.randint(1, 200)), P) for _ in range(G)] for P in (70, 5, 100000, 30)]
    ins, outs = _device_io(batches[0], N, Lp)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _launch(ins, outs, G, Lp, N)
    torch.cuda.current_stream().wait_stream(s)
    for b in batches[1:] + batches[:1]:                                # (no stale state: sparse after dense after sparse)
        new, _ = _device_io(b, N, Lp)
        ins[0].copy_(new[0])
        ins[1].copy_(new[1])
        g.replay()
        torch.cuda.synchronize()
        _compare(outs, _expected(b, N), "replay")


# ------------------------------------------------------------------------------------------------ the collator
def _same_batch(a, b):
    for f in a._fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape, f
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), f
    assert torch.equal(a._counts, b._counts) and torch.equal(a._n_nodes, b._n_nodes)


def _session_collator(coll, **kw):
    return SessionCollator(coll.device, bin_table=coll.bin_table, multi_hop_max_dist=coll.D, rel_pos_max=coll.rel_pos_max,
                           max_node=coll.max_node, **kw)


@pytest.fixture(scope="module")
def fsq():
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, model_overrides=dict(n_layers=2))
    rng = np.random.RandomState(61)
    lens = list(np.clip(rng.lognormal(2.0, 0.9, 72).astype(int), 1, 120))
    sessions = synth.make_sessions(seed=61, G=len(lens), P=uni.P, n_user=uni.n_user, cat_of_poi=uni.cat_of_poi, n_nodes=lens)
    for u, c in sessions[::3]:                                         # a third of them end on a revisit
        if len(c) > 3:
            c[-2] = c[0]
    sessions[16 + 7][1][-1, 0] = 1                                     # y == 1 mid-batch: get_acc's stop (shifted target 0)
    return uni, model, coll, _session_collator(coll), sessions


def test_collator_equals_the_dict_collator_with_a_bin_table(fsq):
    uni, model, coll, scoll, sessions = fsq
    for part, n_pad in ((sessions[:16], None), (sessions[16:33], 128), (sessions[40:41], None)):
        want = coll(sessions_to_trajectories(part), idx0=5, n_pad=n_pad)
        _same_batch(scoll(part, idx0=5, n_pad=n_pad), want)
        _same_batch(scoll(SessionDataset(part), idx0=5, n_pad=n_pad), want)          # records of a dataset
    with pytest.raises(ValueError, match="n_pad"):
        scoll(sessions[:16], n_pad=2)


def test_collator_equals_the_dict_collator_with_coordinate_bins():
    uni = synth.make_sparse_universe(P=3000, n_cat=20, n_user=30, seed=2)
    kw = dict(coords=uni.coords, bin_edges=uni.bin_edges, multi_hop_max_dist=20, rel_pos_max=1024)
    coll, scoll = DeviceCollator(DEV, **kw), SessionCollator(DEV, **kw)
    sessions = synth.make_sessions(seed=8, G=9, P=uni.P, n_user=uni.n_user, cat_of_poi=uni.cat_of_poi, n_nodes=[1, 2, 3, 9, 17, 30, 64, 65, 90])
    _same_batch(scoll(sessions, n_pad=96), coll(sessions_to_trajectories(sessions), n_pad=96))


def test_histories_beyond_the_kernels_limit_fall_back_to_host_conversion(fsq):
    """A history of 4097 check-ins is converted on the host and staged as dicts: the collator's batch and the loops' staged
    bytes equal the dict path's, also when one bucket's staging buffers alternate between the two modes."""
    uni, model, coll, scoll, _ = fsq
    rng = np.random.RandomState(41)
    assert _lib_data.MAX_LP == 4096
    long_ = [_random_session(rng, 4097, 200)] + [_random_session(rng, int(rng.randint(1, 60)), 200) for _ in range(15)]
    d = _random_session(rng, 230, 1500, distinct=True)[1]             # 205 distinct POIs, then revisits: the same bucket, 244 check-ins
    short = [(3, np.concatenate([d[:205], d[:40]]))] + [_random_session(rng, int(rng.randint(1, 60)), 200) for _ in range(15)]
    sessions = [(u % uni.n_user, c) for u, c in long_ + short]
    ds, dicts = SessionDataset(sessions), sessions_to_trajectories(sessions)
    assert bucket_nodes(ds[0].n) == bucket_nodes(ds[16].n) == 208 and len(ds[0].checkins) - 1 == 4097
    _same_batch(scoll(sessions[:16], idx0=2), coll(dicts[:16], idx0=2))
    a, b = EvalLoop(model, scoll, ds, batch_size=16), EvalLoop(model, coll, dicts, batch_size=16)
    A, B = list(range(16)), list(range(16, 32))
    modes = []
    for ids in (A, B, B, A, A):                                        # (both staging buffers of the bucket see both modes)
        slot, st = a._stage(ids)
        modes.append(st["mode"])
        a.copy_stream.synchronize()
        (kb, want) = _staged_bytes(b, ids)
        assert (slot["layout"].G, slot["layout"].N) == kb == (16, 208)
        assert torch.equal(st["dev"][:slot["copy_bytes"]], want), (ids[0], modes)
    assert modes == ["dicts", "sessions", "sessions", "dicts", "dicts"]


# ------------------------------------------------------------------------------------------------ the loops
def _coords(uni):
    c = np.zeros((uni.P + 1, 2))
    c[1:] = uni.poi_table[:, 2:4]
    return torch.from_numpy(c)


@pytest.mark.parametrize("kw", [dict(), dict(exclude_visited=True), dict(within_km=2.0, near="last")], ids=["plain", "new_pois", "near_last"])
def test_predict_and_eval_loops_from_sessions_equal_the_dict_loops(fsq, kw):
    uni, model, coll, scoll, sessions = fsq
    ds, dicts = SessionDataset(sessions), sessions_to_trajectories(sessions)
    kw = dict(kw, coords=_coords(uni)) if "within_km" in kw else kw
    if "within_km" in kw:                                              # the anchor of near="last" is the last history check-in
        assert sum(len(np.unique(c[:-1, 0])) < len(c) - 1 and c[-2, 0] in c[:-2, 0] for _, c in sessions) >= 10
        assert all(d["node_name"][-1] == c[-2, 0] for d, (_, c) in zip(dicts, sessions))
    model.eval()
    si, ii, vi = PredictLoop(model, scoll, ds, k=10, batch_size=16, **kw).run()
    sd, idd, vd = PredictLoop(model, coll, dicts, k=10, batch_size=16, **kw).run()
    torch.cuda.synchronize()
    assert torch.equal(si, sd) and torch.equal(ii, idd) and torch.equal(vi.view(torch.int32), vd.view(torch.int32))
    assert int((ii >= 0).sum()) > 0
    got, want = EvalLoop(model, scoll, ds, batch_size=16, **kw).run(), EvalLoop(model, coll, dicts, batch_size=16, **kw).run()
    assert got == want and got["n"] == len(sessions)
    # the public entry points take the session forms as they are
    i2 = model.recommend(ds, scoll, k=10, **kw)[1]
    assert torch.equal(i2, ii) and model.evaluate(ds, scoll, **kw) == want


def _staged_bytes(loop, ids):
    slot, st = loop._stage(ids)
    loop.copy_stream.synchronize()
    n = slot["copy_bytes"]
    return (slot["layout"].G, slot["layout"].N), st["dev"][:n].clone()


@pytest.mark.parametrize("side", [True, False], ids=["side_collate", "in_graph_collate"])
def test_epoch_loop_stages_the_same_bytes_from_sessions_and_from_dicts(side):
    """The inputs of three steps over two buckets, byte for byte (inputs, not losses: the backward pass is not bit-reproducible
    from run to run), at staging and in the static batches the step graphs read after a run."""
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, model_overrides=dict(n_layers=2))     # (a model of its own: it trains)
    scoll = _session_collator(coll)
    ns = [3] * 8 + [7] * 8 + [20] * 8 + [24] * 8 + [5] * 16
    sessions = synth.make_sessions(seed=17, G=len(ns), P=uni.P, n_user=uni.n_user, cat_of_poi=uni.cat_of_poi, n_nodes=ns)
    ds, dicts = SessionDataset(sessions), sessions_to_trajectories(sessions)
    kw = dict(batch_size=16, seed=3, shuffle=False, balance=False, side_collate=side)
    a, b = EpochLoop(model, scoll, ds, **kw), EpochLoop(model, coll, dicts, **kw)
    batches = a.batches_of_epoch(0)
    assert batches == b.batches_of_epoch(0) and len(batches) == 3
    keys = []
    for rep in range(2):                                               # (twice: both staging buffers of every bucket)
        for ids in batches:
            (ka, xa), (kb, xb) = _staged_bytes(a, ids), _staged_bytes(b, ids)
            assert ka == kb and torch.equal(xa, xb), (rep, ids[0])
            keys.append(ka)
    assert len(set(keys)) == 2
    if not side:
        return
    # a run from sessions: afterwards every bucket's static batch holds the bytes of the last batch that used it
    c = EpochLoop(model, scoll, ds, **kw)
    losses = []
    res = c.run_epoch(0, on_step=lambda k, l: losses.append(l))
    torch.cuda.synchronize()
    assert res["steps"] == 3 and all(bool(torch.isfinite(l.float()).all()) for l in losses)
    for ids in batches[1:]:                                            # (batch 0's bucket was overwritten by batch 2)
        key, want = _staged_bytes(b, ids)
        assert torch.equal(c.slots[key]["buf"][:want.numel()], want), key


def test_first_use_of_a_session_stage_behind_a_busy_compute_stream(fsq):
    """A stage allocates its device session buffer on its first use, when the compute stream may still run a step.  Nothing
    queued on that stream for the new buffer may land after the copy stream has filled it (a fill that lands between the
    upload and the kernel that reads it leaves a batch of zeros): staged while the compute stream is kept busy for some tens
    of milliseconds, the buffer still holds the uploaded bytes once both streams are idle, and the stage the dict path's."""
    uni, model, coll, scoll, sessions = fsq
    ds, dicts = SessionDataset(sessions[:16]), sessions_to_trajectories(sessions[:16])
    a, b = EvalLoop(model, scoll, ds, batch_size=16), EvalLoop(model, coll, dicts, batch_size=16)
    ids = list(range(16))
    key, want = _staged_bytes(b, ids)
    slot, first = a._stage(ids)                                        # (the bucket and its first stage exist now)
    torch.cuda.synchronize()
    busy = torch.randn(4096, 4096, device=DEV)
    busy = (busy @ busy).clamp_(-1.0, 1.0)                             # (the GEMM library is loaded before the clock matters)
    torch.cuda.synchronize()
    for _ in range(40):
        busy = (busy @ busy).clamp_(-1.0, 1.0)                         # queued on the compute stream, not waited for
    slot, st = a._stage(ids)                                           # the second stage's first use
    assert st is not first and st["mode"] == "sessions"
    a.copy_stream.synchronize()
    got = st["dev"][:slot["copy_bytes"]].clone()
    torch.cuda.synchronize()
    assert (slot["layout"].G, slot["layout"].N) == key and torch.equal(got, want)
    nb = st["slay"].nbytes(st["Lp"])
    assert torch.equal(st["sdev"][:nb].cpu(), st["spin"][:nb]) and int(st["spin"][:nb].max()) > 0


def test_out_of_range_indices_raise_on_the_host_before_any_launch(fsq):
    uni, model, coll, scoll, sessions = fsq
    model.eval()
    good = [(u, c.copy()) for u, c in sessions[:16]]

    def both(mutate, match):
        bad = [(u, c.copy()) for u, c in good]
        bad = mutate(bad)
        msgs = []
        for cl, dset in ((scoll, SessionDataset(bad)), (coll, sessions_to_trajectories(bad))):
            loop = PredictLoop(model, cl, dset, k=5, batch_size=16)
            launched = []
            cl.upload = lambda st: launched.append(1)            # (shadows the method on this instance)
            try:
                with pytest.raises(IndexError, match=match) as e:
                    loop.run()
            finally:
                del cl.upload
            assert not launched                                        # nothing was copied or launched for the batch
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], msgs
    poi = lambda bad: (bad[3][1].__setitem__((0, 0), uni.P + 7), bad)[1]
    both(poi, r"batch\.x has index %d" % (uni.P + 7))
    rep = np.stack([np.full(140, 9), np.arange(140) % 48, np.ones(140, dtype=np.int64)], 1).astype(np.int32)
    both(lambda bad: bad[:5] + [(2, rep)] + bad[6:], r"batch\.edge_input has index 141, out of range for a table of 128 rows")
