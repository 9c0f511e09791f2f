"""The distance bins of one batch's pairs on the device (mobgt_bins_batch in csrc_pairbins/batch.hip, through geo.batch_bins and
DeviceCollator(pair_bins=)).  The squared chord is defined bit for bit (include/mobgt_bins.h), so `geo.batch_bins_host` on the
device's own unit vectors is an exact reference: every comparison with it is over every element.  Shapes: one element, a row
shorter than a store, odd N on both sides of a wave and of a workgroup's 8 rows, more than one workgroup per graph; threshold
counts 2, a few dozen, and one past the 2048 the kernel keeps in LDS.  Then the collator and the loops that can now collate a
coordinate-bin universe on their copy stream and replay a captured graph."""
import functools

import numpy as np
import pytest
import torch

import geo_cases
import pair_bins_cases
from mobgt_amd import _lib_bins, _pairbins, data, geo, synth, workloads
from mobgt_amd.data import DeviceBatch1, DeviceCollator, SessionCollator, bucket_nodes, sessions_to_trajectories
from mobgt_amd.ops import _p, _stream
from mobgt_amd.train import EpochLoop, EvalLoop, PredictLoop, TrainStep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 50
SHAPES = ((1, 1), (2, 3), (3, 65), (2, 257))
LDS_THRESHOLDS = 2048                              # csrc_bins/bins_search.h COARSE: beyond it the search continues in global memory


@functools.lru_cache(maxsize=None)
def on_device():
    """(coords, unit on the device, the same unit in numpy, c2 [P, P] with the header's expression) -- computed once."""
    c = geo_cases.city(P, 0)
    unit = geo.unit_vectors(torch.tensor(c, device=DEV))
    u = unit.cpu().numpy()
    c2 = geo._chord2_rows_host(u, 0, P)
    for a in (c, u, c2):
        a.setflags(write=False)
    return c, unit, u, c2


@functools.lru_cache(maxsize=None)
def threshold_sets():
    """nthr = 2; 23 thresholds that are pairs' own squared chords, one of them twice; geo.distance_bins' own, whose last is the
    farthest pair's; 2049: one past what the kernel keeps in LDS, pairs' own values among them."""
    c, unit, u, c2 = on_device()
    rng = np.random.RandomState(7)
    picked = rng.choice(c2[c2 > 0.0], 21, replace=False)
    mid = np.sort(np.concatenate([[0.0], picked, picked[:1]]))
    bins = geo.distance_bins(c, device=DEV, table=False)
    assert bins.thresholds[-1] == c2.max() and bins.thresholds[0] == 0.0
    big = np.sort(np.concatenate([[0.0], rng.uniform(0.0, c2.max(), LDS_THRESHOLDS - 20), picked[:20]]))
    assert len(mid) == 23 and len(big) == LDS_THRESHOLDS + 1 and (np.diff(mid) == 0.0).sum() == 1
    return dict(two=np.array([0.0, float(c2.max())]), mid=mid, bins=np.array(bins.thresholds), past_lds=big)


def ids(G, N, seed=0):
    """[G, N] int32 ids.  Row 0: ids 1 and P, POI P twice, the farthest pair (N >= 65), pads at the end; row 1: pads in the
    middle, one id P + 1 and one negative; row 2: pads only -- as far as the shape has room."""
    x = np.random.RandomState(100 * G + N + seed).randint(1, P + 1, size=(G, N)).astype(np.int32)
    x[0, 0] = P if N == 1 else 1
    if N >= 3:
        x[0, 1] = x[0, 2] = P
        x[0, max(3, N // 2 + 1):] = 0
    if N >= 65:
        c2 = on_device()[3]
        x[0, 3], x[0, 4] = (int(i) + 1 for i in np.unravel_index(np.argmax(c2), c2.shape))
    if G > 1:
        x[1, ::3] = 0
        if N >= 3:
            x[1, 1], x[1, 2] = P + 1, -5
    if G > 2:
        x[2] = 0
    return x


def pair_bins_of(thr):
    _, unit, _, _ = on_device()
    return geo.PairBins(P, unit, torch.tensor(thr, device=DEV), len(thr) - 1)


def poisoned(n):
    return torch.full((n,), -1, dtype=torch.int16, device=DEV)


@pytest.mark.parametrize("G,N", SHAPES)
@pytest.mark.parametrize("thr", ["two", "mid", "bins", "past_lds"])
def test_kernel_is_batch_bins_host_exactly(G, N, thr):
    _, unit, u, c2 = on_device()
    t = threshold_sets()[thr]
    x = ids(G, N)
    want = geo.batch_bins_host(u, t, x)
    got = geo.batch_bins(pair_bins_of(t), torch.from_numpy(x).to(DEV), out=poisoned(G * N * N).view(G, N, N))
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), want)
    if N >= 3:
        # the duplicated POI: c2 = +0.0, bin #{thr <= 0}; a pair that sits on a threshold counts it; the outsiders give 0
        assert want[0, 1, 2] == (t <= 0.0).sum() and want[0, 0, 1] == (t <= c2[0, P - 1]).sum()
        assert G == 1 or (want[1, 1] == 0).all() and (want[1, :, 2] == 0).all()
    assert (want[x == 0] == 0).all() and (G < 3 or (want[2] == 0).all())
    if thr == "bins" and N >= 65:
        assert want.max() == len(t)                                    # the farthest pair takes part: the last threshold is its own


def test_ids_as_a_column_and_a_fresh_output():
    _, unit, u, _ = on_device()
    t = threshold_sets()["mid"]
    x = ids(3, 65)
    got = geo.batch_bins(pair_bins_of(t), torch.from_numpy(x[:, :, None].copy()).to(DEV))
    assert got.shape == (3, 65, 65) and np.array_equal(got.cpu().numpy(), geo.batch_bins_host(u, t, x))
    with pytest.raises(ValueError, match="int32"):
        geo.batch_bins(pair_bins_of(t), torch.from_numpy(x).to(DEV).long())


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_output_that_starts_off_an_eight_byte_boundary(skew):
    """A view 2, 4 and 6 bytes past an 8-byte boundary (skew 1 and 3: one int16 past a 4-byte boundary), N odd: the row heads
    and tails move, nothing around the view is written."""
    _, unit, u, _ = on_device()
    t = threshold_sets()["mid"]
    G, N = 3, 65
    x = ids(G, N)
    buf = poisoned(G * N * N + 8)
    assert buf.data_ptr() % 8 == 0
    geo.batch_bins(pair_bins_of(t), torch.from_numpy(x).to(DEV), out=buf[skew:skew + G * N * N].view(G, N, N))
    flat = buf.cpu().numpy()
    assert (flat[:skew] == -1).all() and (flat[skew + G * N * N:] == -1).all()
    assert np.array_equal(flat[skew:skew + G * N * N], geo.batch_bins_host(u, t, x).ravel())


def test_kernel_is_the_table_on_real_pairs():
    _, unit, _, _ = on_device()
    for name in ("mid", "bins"):
        t = threshold_sets()[name]
        table = geo.bin_table(unit, t).cpu().numpy()
        x = np.clip(ids(2, 257), 0, P)                                 # (the table has no row for an outsider)
        x[x < 0] = 0
        got = geo.batch_bins(pair_bins_of(t), torch.from_numpy(x).to(DEV)).cpu().numpy()
        real = (x != 0)[:, :, None] & (x != 0)[:, None, :]
        assert real.any() and np.array_equal(got[real], table[x[:, :, None], x[:, None, :]][real]) and (got[~real] == 0).all()


def test_error_codes_come_back_with_nothing_launched():
    _, unit, _, _ = on_device()
    t = torch.tensor(threshold_sets()["mid"], device=DEV)
    G, N = 2, 3
    x = torch.from_numpy(ids(G, N)).to(DEV)
    out = poisoned(G * N * N)
    fn = _pairbins.lib().mobgt_bins_batch
    good = dict(unit=_p(unit), P=P, thr=_p(t), nthr=t.numel(), x=_p(x), G=G, N=N, out=_p(out))
    call = lambda **kw: (lambda a: fn(a["unit"], a["P"], a["thr"], a["nthr"], a["x"], a["G"], a["N"], a["out"], _stream()))(dict(good, **kw))
    assert call(nthr=1) == call(G=0) == call(P=0) == call(N=0) == call(nthr=_lib_bins.MAX_THRESHOLDS + 1) == _pairbins.EBADDIM
    assert call(unit=None) == call(thr=None) == call(x=None) == call(out=None) == _pairbins.EALIGN
    assert call(out=out.data_ptr() + 1) == call(x=x.data_ptr() + 2) == _pairbins.EALIGN
    torch.cuda.synchronize()
    assert bool((out == -1).all())
    assert call() == 0 and bool((out != -1).all())
    with pytest.raises(_pairbins.MobgtPairBinsError, match="EBADDIM"):
        geo.batch_bins(geo.PairBins(P, unit, t[:1], 0), x)


# ------------------------------------------------------------------------------------------------ the collator
def same_fields(a, b, skip=()):
    for f in DeviceBatch1._fields:
        if f not in skip:
            ta, tb = getattr(a, f), getattr(b, f)
            assert ta.dtype == tb.dtype and ta.shape == tb.shape and torch.equal(ta, tb), f


@functools.lru_cache(maxsize=None)
def small_universe():
    uni = synth.make_sparse_universe(P=400, n_cat=20, n_user=8, seed=0)
    return uni, geo.pair_bins(uni.coords, edges=uni.bin_edges, device=DEV, pad_row=True)


def test_collator_against_the_haversine_collator():
    uni, pb = small_universe()
    assert pb.P == 400 and pb.num_bins == uni.num_bins and pb.unit.is_cuda and pb.thresholds.is_cuda
    trajs = synth.make_batch_of_trajectories(seed=5, G=6, P=400, n_user=8, cat_of_poi=uni.cat_of_poi, n_nodes=[40, 3, 17, 64, 9, 25])
    ours, theirs = DeviceCollator(DEV, pair_bins=pb), DeviceCollator(DEV, coords=uni.coords, bin_edges=uni.bin_edges)
    assert ours.can_finish_into() and not theirs.can_finish_into()
    assert DeviceCollator(DEV, pair_bins=pb, coords=uni.coords).can_finish_into()
    a, b = ours(trajs), theirs(trajs)
    same_fields(a, b, skip=("poi_pos",))
    assert a.poi_pos.dtype == b.poi_pos.dtype == torch.int16 and a.poi_pos.shape == b.poi_pos.shape and int(a.poi_pos.max()) > 1
    x = a.x[:, :, 0].cpu().numpy()
    pair_bins_cases.assert_agrees_with_haversine(a.poi_pos.cpu().numpy(), uni.coords, x, uni.bin_edges, "against the haversine collator",
                                                 want=b.poi_pos.cpu().numpy())
    pair_bins_cases.assert_agrees_with_haversine(a.poi_pos.cpu().numpy(), uni.coords, x, uni.bin_edges, "against np.digitize")


@functools.lru_cache(maxsize=None)
def small_table():
    """The int16 bin table of the small universe, as geo.distance_bins leaves it on the device."""
    uni, _ = small_universe()
    table = geo.distance_bins(uni.coords, device=DEV, pad_row=True).table
    assert table.dtype == torch.int16 and table.is_contiguous() and table.shape == (401, 401)
    return table


def collator_with(source, **kw):
    """A collator per source of poi_pos the kernels serve: the chord search, the int16 table, none (all zeros)."""
    source_kw = dict(pair_bins=dict(pair_bins=small_universe()[1]), table=dict(bin_table=small_table()), none={})[source]
    return DeviceCollator(DEV, **source_kw, **kw)


@pytest.mark.parametrize("source", ["pair_bins", "table", "none"])
def test_finish_into_equals_finish(source):
    uni, pb = small_universe()
    coll = collator_with(source)
    trajs = synth.make_batch_of_trajectories(seed=6, G=5, P=400, n_user=8, cat_of_poi=uni.cat_of_poi, n_nodes=[61, 2, 33, 1, 20])
    G, N = 5, 65                                                       # (odd N: rows of poi_pos start on odd int16 offsets)
    h = coll.pack_host(trajs, idx0=3, n_pad=N)
    lay = data.BatchLayout(G, N, coll.D)
    buf = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)       # (as the loops allocate their staging buffers)
    v = lay.views_torch(buf)
    for k, arr in h.items():
        v[k].copy_(torch.from_numpy(arr))
    v["poi_pos"].fill_(-1)                                             # every element of it is written
    coll.finish_into(v)
    want = coll.finish({k: torch.from_numpy(arr).to(DEV) for k, arr in h.items()})
    same_fields(coll.batch_from_views(v), want)
    assert int(want.poi_pos.max()) > 1 if source != "none" else not bool(want.poi_pos.any())


# finish has two forms: finish_into's launches into fresh tensors (the kernel form) and torch ops behind mobgt_spd_batched (the
# torch form: haversine bins, a table that is not contiguous int16, ids that are not int32).  G = 4 graphs of 1, 5, 33 and 64
# nodes at the odd pitch N = 65, D = 20.
FORMS_N, FORMS_NODES = 65, (1, 5, 33, 64)


@functools.lru_cache(maxsize=None)
def forms_batch():
    """The raw arrays of that batch on the device (read only: finish writes none of them)."""
    uni, _ = small_universe()
    trajs = synth.make_batch_of_trajectories(seed=7, G=len(FORMS_NODES), P=400, n_user=8, cat_of_poi=uni.cat_of_poi, n_nodes=list(FORMS_NODES))
    h = DeviceCollator(DEV).pack_host(trajs, idx0=11, n_pad=FORMS_N)
    return {k: torch.from_numpy(arr).to(DEV) for k, arr in h.items()}


@pytest.mark.parametrize("rel_pos_max", [1024, 3])
def test_torch_form_of_finish_equals_the_kernel_form(rel_pos_max):
    """attn_bias holds 0 and -inf only and every other field is an integer or a copy: equality is exact.  The int64 table gives
    an int64 poi_pos, compared by value."""
    d = forms_batch()
    kernel = DeviceCollator(DEV, bin_table=small_table(), multi_hop_max_dist=20, rel_pos_max=rel_pos_max)
    by_torch = DeviceCollator(DEV, bin_table=small_table().long(), multi_hop_max_dist=20, rel_pos_max=rel_pos_max)
    assert kernel.can_finish_into() and not by_torch.can_finish_into()
    a, b = kernel.finish(dict(d)), by_torch.finish(dict(d))
    same_fields(a, b, skip=("poi_pos",))
    assert a.poi_pos.dtype == torch.int16 and a.poi_pos.shape == b.poi_pos.shape == (4, FORMS_N, FORMS_N)
    assert torch.equal(a.poi_pos.long(), b.poi_pos.long()) and int(a.poi_pos.max()) > 1
    assert a.edge_input.shape == (4, FORMS_N, FORMS_N, 20, 1)
    far = torch.isinf(a.attn_bias[3, 1:65, 1:65]).any()               # (among the 64 real nodes of the longest graph)
    assert bool(far) == (rel_pos_max == 3) and bool(torch.isinf(a.attn_bias[0, :, 2:]).all())
    # no table: all-zero int16 poi_pos by either form; ids given as int64 select the torch form
    none = DeviceCollator(DEV, multi_hop_max_dist=20, rel_pos_max=rel_pos_max)
    k, t = none.finish(dict(d)), none.finish(dict(d, x=d["x"].long()))
    same_fields(k, t, skip=("x",))
    assert torch.equal(k.x.long(), t.x) and k.poi_pos.dtype == torch.int16 and not bool(k.poi_pos.any())
    same_fields(k, a, skip=("poi_pos",))


def test_which_entry_points_a_finish_calls(monkeypatch):
    """The library calls of every form, in order, as the code before finish had one kernel path made them: the workspace query,
    mobgt_spd_batched, mobgt_collate_finish [, one mobgt_bins_batch]; the torch form stops behind mobgt_spd_batched."""
    from mobgt_amd import _lib
    uni, pb = small_universe()
    d, table = forms_batch(), small_table()
    real, real_launch = _lib.lib(), _pairbins.launch
    work = torch.empty(int(real.mobgt_spd_workspace_bytes(4, FORMS_N)), dtype=torch.uint8, device=DEV)
    seen = []

    class _Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)

    def launch(name, *args):
        seen.append(name)
        return real_launch(name, *args)

    monkeypatch.setattr(_lib, "lib", lambda: _Spy())
    monkeypatch.setattr(_pairbins, "launch", launch)

    def calls(fn):
        del seen[:]
        fn()
        return list(seen)

    def views(coll):
        lay = data.BatchLayout(4, FORMS_N, coll.D)
        v = lay.views_torch(torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV))
        for k, t in d.items():
            v[k].copy_(t)
        return v

    kernel = ["mobgt_spd_workspace_bytes", "mobgt_spd_batched", "mobgt_collate_finish"]
    for source, more in (("table", []), ("none", []), ("pair_bins", ["mobgt_bins_batch"])):
        coll = collator_with(source)
        assert calls(lambda: coll.finish(dict(d))) == kernel + more, source
        v = views(coll)
        assert calls(lambda: coll.finish_into(v)) == kernel + more, source
        assert calls(lambda: coll.finish_into(v, work)) == kernel[1:] + more, source
    by_torch = ["mobgt_spd_workspace_bytes", "mobgt_spd_batched"]
    haversine = DeviceCollator(DEV, coords=uni.coords, bin_edges=uni.bin_edges)
    assert calls(lambda: haversine.finish(dict(d))) == by_torch
    assert calls(lambda: DeviceCollator(DEV, bin_table=table.long()).finish(dict(d))) == by_torch
    assert calls(lambda: collator_with("none").finish(dict(d, x=d["x"].long()))) == by_torch
    torch.cuda.synchronize()


def test_session_collator_equals_the_dict_collator():
    uni, pb = small_universe()
    coll, scoll = DeviceCollator(DEV, pair_bins=pb), SessionCollator(DEV, pair_bins=pb)
    assert scoll.can_finish_into()
    sessions = synth.make_sessions(seed=8, G=9, P=uni.P, n_user=uni.n_user, cat_of_poi=uni.cat_of_poi, n_nodes=[1, 2, 3, 9, 17, 30, 64, 65, 90])
    same_fields(scoll(sessions, n_pad=96), coll(sessions_to_trajectories(sessions), n_pad=96))


# ------------------------------------------------------------------------------------------------ the loops
def big_model(seed=1):
    """workloads.build("big") at P = 1500 with two layers, and the pair_bins collator for its universe."""
    uni, model, _ = workloads.build("big", DEV, seed=seed, P=1500, model_overrides=dict(n_layers=2))
    pb = geo.pair_bins(uni.coords, edges=uni.bin_edges, device=DEV, pad_row=True)
    return uni, model, DeviceCollator(DEV, pair_bins=pb, multi_hop_max_dist=20, rel_pos_max=1024)


def short_trajectories(uni, n=40, seed=61):
    lens = [int(v) for v in np.clip(np.random.RandomState(seed).lognormal(2.0, 0.7, n).astype(int), 2, 40)]
    return synth.make_batch_of_trajectories(seed=seed, G=n, P=uni.P, n_user=uni.n_user, cat_of_poi=uni.cat_of_poi, n_nodes=lens)


@pytest.fixture(scope="module")
def big_eval():
    uni, model, coll = big_model()
    return uni, model.eval(), coll, short_trajectories(uni)


def test_eval_loop_replays_a_captured_graph(big_eval):
    """The graph loop against use_graph=False: exactly, as tests/test_gpu_eval.py compares them for the bin-table collator."""
    uni, model, coll, trajs = big_eval
    loop = EvalLoop(model, coll, trajs, batch_size=16)
    got = loop.run()
    assert loop.slots and all(s["side"] for s in loop.slots.values())
    assert loop.captures == len(loop.graphs) >= 1 and got["n"] == len(trajs)
    captures = loop.captures
    assert loop.run() == got and loop.captures == captures           # replayed: nothing captured again
    assert EvalLoop(model, coll, trajs, batch_size=16, use_graph=False).run() == got


def test_predict_loop_replays_a_captured_graph(big_eval):
    """ids and vals against use_graph=False: equal, as tests/test_gpu_topk.py compares them for the bin-table collator."""
    uni, model, coll, trajs = big_eval
    loop = PredictLoop(model, coll, trajs, k=10, batch_size=16)
    a = loop.run()
    torch.cuda.synchronize()
    assert loop.slots and all(s["side"] for s in loop.slots.values()) and len(loop.graphs) >= 1
    eager = PredictLoop(model, coll, trajs, k=10, batch_size=16, use_graph=False).run()
    torch.cuda.synchronize()
    for x, y in zip(a, eager):
        assert torch.equal(x, y)
    assert int((a[1] >= 1).sum()) > 0


def test_epoch_loop_steps_on_the_side_collated_batch():
    """One step of the loop (collate on the copy stream, finish_into) against one step of a TrainStep fed collator(batch) by
    hand, two models built alike.  The loss of a first step is a forward pass's: two forward passes over one batch agree to
    1e-6 relative (tests/test_gpu_loop.py, the bucket-padded batch)."""
    losses = []
    for by_loop in (True, False):
        uni, model, coll = big_model(seed=1)
        trajs = short_trajectories(uni, n=16, seed=9)
        if by_loop:
            loop = EpochLoop(model, coll, trajs, batch_size=16, seed=3, shuffle=False)
            loop.run_epoch(0, max_steps=1, on_step=lambda k, l: losses.append(float(l.item())))
            assert all(s["side"] for s in loop.slots.values())
        else:
            batch = coll(trajs, n_pad=bucket_nodes(max(len(t["node_name"]) for t in trajs)))
            ts = TrainStep(model, [batch], use_graph=True, seed=3)
            ts.prepare()
            losses.append(float(ts.step(0).item()))
    print("first-step loss: by the loop", losses[0], "by hand", losses[1])
    assert np.isfinite(losses).all()
    np.testing.assert_allclose(losses[0], losses[1], rtol=1e-6)
