"""The distance prior on the device (csrc_geoprior/geoprior.hip through mobgt_amd.geoprior) against the host forms, compared
EXACTLY -- integer histograms as lists, blended scores as uint32 views, no tolerance anywhere: pair_hist on either side of a wave,
of the column tile and of a second tile, with the thresholds on either side of the coarse stride and of the LDS histogram's
limit; csr_hist on empty, full and broken CSRs; blend_rows on either side of its chunk, both label offsets, int32 and int64 ids,
padded leading dimensions, in place and out of place; every return code with nothing launched; DistancePrior.fit; and the loops:
EvalLoop / PredictLoop with a prior.Stack and a bare DistancePrior, captured and eager, against blend_host on the downloaded
scores, set_weights without a new capture, and the weight sweep."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import anchor_cases as ac
import geoprior_cases as gc
import prior_cases as pc
from mobgt_amd import _geoprior, _lib_bins, data, geo, geoprior, metrics, ops, prior, workloads
from mobgt_amd.data import bucket_nodes
from mobgt_amd.train import EvalLoop, PredictLoop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, CHUNK, LDS_BINS = _geoprior.TILE, _geoprior.CHUNK, _geoprior.LDS_BINS
POISON = 77.0
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def up(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


def ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else v


def _run(name, *args):
    rc = getattr(_geoprior.LIBRARY.lib(), name)(*(ptr(a) for a in args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def universe(P, nthr=37):
    """-> (unit f64 [P, 3], thresholds f64 [nthr]) numpy: duplicates and a pole among the POIs, ties among the thresholds, the
    last the farthest pair's own c2; and the host's pair histogram of them"""
    u = gc.unit(P, seed=P)
    thr = gc.thresholds(u, nthr, seed=P + nthr)
    assert thr.size == nthr and thr[0] == 0.0 and thr[-1] == gc.chord2_max(u) and (nthr < 8 or (np.diff(thr) == 0).any())
    return u, thr


def pair_hist(u, thr):
    counts = torch.full((thr.size + 1,), -7, dtype=torch.int64, device=DEV)    # (poisoned: the call clears it)
    assert _run("mobgt_geoprior_pair_hist", up(u), u.shape[0], up(thr), thr.size, counts) == 0
    return counts.cpu().numpy()


# ------------------------------------------------------------------------------------------------ pair_hist
@pytest.mark.parametrize("P", (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3))
def test_pair_hist_on_either_side_of_a_wave_and_a_tile(P):
    u, thr = universe(P)
    want = geoprior.pair_hist_host(u, thr)
    got = pair_hist(u, thr)
    assert got.tolist() == want.tolist() and int(got.sum()) == P * P and got[0] == 0 and got[-1] >= 1


@pytest.mark.parametrize("nthr", (2, 3, 2048, 2049, 32767))
def test_pair_hist_on_either_side_of_the_coarse_stride_and_the_lds_limit(nthr):
    assert (nthr + 1 <= LDS_BINS) == (nthr != 32767)                    # 2048 | 2049: bins_search.h's COARSE; 32767: no LDS histogram
    for P in (193,) + ((T + 65,) if nthr == 32767 else ()):
        u, thr = universe(P, nthr)
        assert np.array_equal(u[0], u[1]) and abs(u[-1, 2] - 1.0) < 1e-15      # an exact duplicate and a pole
        want = geoprior.pair_hist_host(u, thr)
        got = pair_hist(u, thr)
        assert got.tolist() == want.tolist() and int(got.sum()) == P * P
        assert got[0] == 0 and got[-1] >= 2 and (got == 0).sum() >= (nthr >= 8)    # duplicates in a bin >= 1, the farthest pair in bin nthr


# ------------------------------------------------------------------------------------------------ csr_hist
def csr_hist(u, thr, rowptr, col, val, status=None):
    counts = torch.full((thr.size + 1,), -7, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status
    d = [up(rowptr), up(col), up(val)]
    assert _run("mobgt_geoprior_csr_hist", up(u), u.shape[0], up(thr), thr.size, *d, len(col), counts, status) == 0
    return counts.cpu().numpy(), status


def test_csr_hist_counts_what_the_host_counts():
    P = 300
    u, thr = universe(P)
    empty = np.zeros(0, dtype=np.int32)
    got, status = csr_hist(u, thr, np.zeros(P + 1, dtype=np.int64), empty, empty)          # nnz = 0: every row is empty, col and val null
    assert got.tolist() == [0] * 38 and status.tolist() == [0]
    for kw in (dict(full_row=17), dict(big=True), dict(full_row=P - 1, seed=5)):
        rowptr, col, val = gc.csr(P, **kw)
        host = [0]
        want = geoprior.csr_hist_host(u, thr, rowptr, col, val, status=host)
        got, status = csr_hist(u, thr, rowptr, col, val)
        assert got.tolist() == want.tolist() and int(got.sum()) == int(val.astype(np.int64).sum()) and status.tolist() == host == [0]
        assert (col == np.repeat(np.arange(P), np.diff(rowptr))).any() and (np.diff(rowptr) == 0).any()    # self-transitions, empty rows
    assert int(val.astype(np.int64).sum()) < 2 ** 31 < int(gc.csr(P, big=True)[2].astype(np.int64).sum())
    one = np.zeros(P + 1, dtype=np.int64)                               # one row holds everything
    one[6:] = P
    col, val = np.arange(P, dtype=np.int32), np.arange(1, P + 1, dtype=np.int32)
    got, status = csr_hist(u, thr, one, col, val)
    assert got.tolist() == geoprior.csr_hist_host(u, thr, one, col, val).tolist() and status.tolist() == [0]


def test_csr_hist_skips_and_flags_what_fit_did_not_make():
    """None of these inputs is read out of bounds: a rowptr pair and an entry of col are checked before they index anything."""
    P = 300
    u, thr = universe(P)
    rowptr, col, val = gc.csr(P, full_row=17)
    nnz = len(col)
    down, beyond, before, bad = rowptr.copy(), rowptr.copy(), rowptr.copy(), col.copy()
    down[18] = rowptr[17] - 1                                           # the full row descends (row 18 then starts early: valid)
    beyond[18] = nnz + 7                                                # the full row runs beyond nnz (and row 18 descends)
    before[17] = -1                                                     # the full row starts before the table (and row 16 descends)
    bad[int(rowptr[17]) + 3] = P                                        # an entry of the full row: POI P + 1
    assert rowptr[17] >= 1 and rowptr[18] - rowptr[17] == P
    clean = geoprior.csr_hist_host(u, thr, rowptr, col, val)
    for rp, cl in ((down, col), (beyond, col), (before, col), (rowptr, bad)):
        host = [0]
        want = geoprior.csr_hist_host(u, thr, rp, cl, val, status=host)
        got, status = csr_hist(u, thr, rp, cl, val)
        assert host == [geoprior.SBADINDEX] and status.tolist() == host and got.tolist() == want.tolist()
        assert 0 < int(got.sum()) and want.tolist() != clean.tolist()   # something was skipped, and the other entries still count
        again, status = csr_hist(u, thr, rowptr, col, val, status=status)                  # a clean call on the same word
        assert again.tolist() == clean.tolist() and status.tolist() == [geoprior.SBADINDEX]   # not cleared


def test_hist_return_codes_with_nothing_launched():
    P = 65
    u, thr = universe(P)
    rowptr, col, val = gc.csr(P)
    d_u, d_t, d_r, d_c, d_v = up(u), up(thr), up(rowptr), up(col), up(val)
    counts = torch.full((38,), -7, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    null, odd = ctypes.c_void_p(0), lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    pair = lambda unit=d_u, P=P, t=d_t, n=37, c=counts: _run("mobgt_geoprior_pair_hist", unit, P, t, n, c)
    csr = lambda unit=d_u, P=P, t=d_t, n=37, r=d_r, c=d_c, v=d_v, nnz=len(col), out=counts, s=status: \
        _run("mobgt_geoprior_csr_hist", unit, P, t, n, r, c, v, nnz, out, s)
    for call in (pair, csr):
        for kw in (dict(P=0), dict(P=_lib_bins.MAX_P + 1), dict(n=1), dict(n=_lib_bins.MAX_THRESHOLDS + 1)):
            assert call(**kw) == _geoprior.EBADDIM, kw
        for key, t in (("unit", d_u), ("t", d_t)):
            assert call(**{key: null}) == _geoprior.EALIGN and call(**{key: odd(t)}) == _geoprior.EALIGN, key
    assert pair(c=null) == pair(c=odd(counts)) == _geoprior.EALIGN
    for kw in (dict(nnz=-1), dict(nnz=2 ** 31)):
        assert csr(**kw) == _geoprior.EBADDIM, kw
    for key, t in (("r", d_r), ("out", counts)):
        assert csr(**{key: null}) == csr(**{key: odd(t)}) == _geoprior.EALIGN, key
    for key, t in (("c", d_c), ("v", d_v), ("s", status)):
        assert csr(**{key: null}) == csr(**{key: ctypes.c_void_p(t.data_ptr() + 2)}) == _geoprior.EALIGN, key
    assert counts.tolist() == [-7] * 38 and status.tolist() == [0]      # nothing was launched, nothing cleared
    with pytest.raises(_geoprior.MobgtGeopriorError, match="MOBGT_GEOPRIOR_EBADDIM") as e:
        _geoprior.launch("mobgt_geoprior_pair_hist", None, 0, None, 37, None, None)
    assert e.value.code == _geoprior.EBADDIM
    assert pair() == 0 and counts.cpu().numpy().tolist() == geoprior.pair_hist_host(u, thr).tolist()      # and the same buffers are good


# ------------------------------------------------------------------------------------------------ blend_rows
BLEND_P = CHUNK + 2
ARGS = ("scores", "ld_scores", "out", "ld_out", "G", "V", "label_offset", "hist", "hist_dtype", "ld_hist", "n_hist_cols", "unit", "P",
        "thresholds", "nthr", "table", "weight")
POINTERS = ("scores", "out", "hist", "unit", "thresholds", "table", "weight")


@functools.lru_cache(maxsize=None)
def tables(P=BLEND_P, nthr=300):
    u, thr = universe(P, nthr)
    return geoprior.DistanceTables(u, thr, (np.random.RandomState(nthr).standard_normal(nthr + 1) * 3).astype(F), P)


def _direct(t, G, V, label_offset=1, wide=False, in_place=False, weight=0.75, seed=0):
    """Device buffers and sizes of a direct call: {argument: tensor or int}, and the host inputs under "host".  wide: int64 ids.
    Every row of scores and out is three columns wider than V and holds POISON there; hist is three columns wider than its n."""
    dtype = np.int64 if wide else np.int32
    hist = gc.hist_rows(G, t.P, seed=seed, dtype=dtype)
    scores = pc.scores(G, V, seed=seed)
    n = hist.shape[1]
    d = dict(G=G, V=V, label_offset=label_offset, hist_dtype=_geoprior.I64 if wide else _geoprior.I32, n_hist_cols=n, ld_hist=n + 3,
             P=t.P, nthr=t.thresholds.size, ld_scores=V + 3, ld_out=V + 3)
    d["hist"] = up(np.concatenate([hist, np.full((G, 3), 5, dtype=dtype)], axis=1))     # (the columns beyond n hold an id: not read)
    d["unit"], d["thresholds"], d["table"] = up(t.unit), up(t.thresholds), up(t.table)
    d["weight"] = up(np.array([9.0, weight], dtype=F))[1:]             # a view into a longer buffer
    d["scores"] = up(np.concatenate([scores, np.full((G, 3), POISON, dtype=F)], axis=1))
    d["out"] = d["scores"] if in_place else torch.full((G, V + 3), POISON, dtype=torch.float32, device=DEV)
    d["host"] = (scores, hist)
    return d


def _call(d, **over):
    return _run("mobgt_geoprior_blend_rows", *(over.get(a, d[a]) for a in ARGS))


def _assert_blended(d, t, weight=0.75):
    scores, hist = d["host"]
    V = d["V"]
    want = geoprior.blend_host(scores, hist, t, weight, d["label_offset"])
    got = d["out"].cpu().numpy()
    assert np.array_equal(bits(got[:, :V]), bits(want))                 # every element inside is the rule's, NaN payloads included
    assert np.all(got[:, V:] == POISON)                                 # and nothing beyond V was touched
    if d["out"] is not d["scores"]:
        assert np.array_equal(bits(d["scores"].cpu().numpy()[:, :V]), bits(scores))
    return want


@pytest.mark.parametrize("form", ("in-place-i32", "out-i64"))
@pytest.mark.parametrize("label_offset", (0, 1))
@pytest.mark.parametrize("G", (1, 3, 16))
@pytest.mark.parametrize("V", (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3))
def test_blend_equals_the_host_rule(V, G, label_offset, form):
    """P = CHUNK + 2: the widths are V < P + 1 and V > P + 1.  16 rows walk through every anchor of geoprior_cases.hist_rows: POI 1
    and P, a duplicate, the pole, an all-pad row, and last ids P + 1, -3 and beyond 2^31."""
    t = tables()
    d = _direct(t, G, V, label_offset, wide=form == "out-i64", in_place=form == "in-place-i32", seed=V + G)
    assert _call(d) == 0
    want = _assert_blended(d, t)
    scores, hist = d["host"]
    if G == 16:
        changed = bits(want) != bits(scores)
        none = [g for g in range(G) if not 1 <= ([x for x in hist[g] if x != 0] or [0])[-1] <= t.P]
        assert len(none) >= 5 and not changed[none].any() and not changed[:, BLEND_P + 1 - label_offset:].any()
        if V >= CHUNK - 1:                                              # (V = 1: one column, no POI's at label_offset 0)
            assert changed[[g for g in range(G) if g not in none]].mean(axis=1).min() > 0.3
    if G == 16 and V > CHUNK:
        assert (bits(want) == 0xFFC12345).any() and (bits(want) == 0x80000000).any() and np.isinf(want).any()


@pytest.mark.parametrize("wide", (False, True), ids=("i32", "i64"))
@pytest.mark.parametrize("n", ac.WIDTHS)
def test_the_anchor_search_across_waves_and_strides(n, wide):
    """The history rows of anchor_cases, n ids wide, by direct call: the only id in the first and in the last position, and two
    ids whose positions lie in different waves and strides, the later one deciding -- two anchors lie at different distances, so
    a wrong winner shows in the output."""
    t = tables()
    d = _direct(t, ac.G, ac.V, ac.LABEL_OFFSET, wide=wide, seed=n)
    scores = d["host"][0]
    hist = ac.rows(n, 3, 17, np.int64 if wide else np.int32)
    assert _call(d, hist=up(hist), n_hist_cols=n, ld_hist=n) == 0
    d["host"] = (scores, hist)
    want = _assert_blended(d, t)
    if n > 1:
        assert (bits(want[3]) != bits(geoprior.blend_host(scores, ac.loser(hist), t, 0.75, ac.LABEL_OFFSET)[3])).any()


def test_blend_of_no_rows_launches_nothing():
    t = tables()
    d = _direct(t, 0, 40)
    assert _call(d) == 0 and _call(d, scores=ctypes.c_void_p(0), out=ctypes.c_void_p(0), hist=ctypes.c_void_p(0)) == 0
    d = _direct(t, 3, 0)
    assert _call(d) == 0 and bool((d["out"] == POISON).all())


@pytest.mark.parametrize("nthr", (2, 2049, 32767))
def test_blend_on_either_side_of_the_coarse_stride(nthr):
    t = tables(193, nthr)
    for lo, V in ((1, 193), (0, 194), (1, 80)):
        d = _direct(t, 16, V, lo, seed=nthr % 7 + V, weight=-1.25)
        assert _call(d) == 0
        _assert_blended(d, t, weight=-1.25)


def test_blend_weight_zero_and_the_weight_is_read_on_the_device():
    t = tables()
    d = _direct(t, 16, CHUNK + 1, weight=0.0, seed=3)
    assert _call(d) == 0
    want = _assert_blended(d, t, weight=0.0)
    scores = d["host"][0]
    assert ((want == scores) | (np.isnan(want) & np.isnan(scores))).all()
    flipped = bits(want) != bits(scores)
    assert flipped.any() and ((bits(scores)[flipped] == 0x80000000) & (bits(want)[flipped] == 0)).all()
    assert _call(d, weight=up(np.array([2.5], dtype=F))) == 0           # another buffer: the weight is read where the call points
    _assert_blended(d, t, weight=2.5)


def test_blend_return_codes_with_nothing_launched():
    t = tables()
    G, V = 3, 33
    d = _direct(t, G, V)
    before = d["out"].clone()
    n = d["n_hist_cols"]
    bad = [("G", -1), ("G", 65536), ("V", -1), ("V", 2 ** 31), ("n_hist_cols", -1), ("n_hist_cols", 2 ** 31), ("P", 0),
           ("P", _lib_bins.MAX_P + 1), ("nthr", 1), ("nthr", _lib_bins.MAX_THRESHOLDS + 1), ("ld_scores", V - 1), ("ld_out", V - 1),
           ("ld_hist", n - 1), ("label_offset", -1), ("label_offset", 2)]
    for key, value in bad:
        assert _call(d, **{key: value}) == _geoprior.EBADDIM, (key, value)
    assert _call(d, out=d["scores"], ld_out=V + 4) == _geoprior.EBADDIM      # in place with another leading dimension
    for value in (-1, 2):
        assert _call(d, hist_dtype=value) == _geoprior.EDTYPE, value
    wide = _direct(t, G, V, wide=True)
    for key in POINTERS:
        assert _call(d, **{key: ctypes.c_void_p(0)}) == _geoprior.EALIGN, key
        assert _call(d, **{key: ctypes.c_void_p(d[key].data_ptr() + 2)}) == _geoprior.EALIGN, key
        if key in ("hist", "unit", "thresholds"):                       # 8-byte elements at a 4-byte address
            assert _call(wide, **{key: ctypes.c_void_p(wide[key].data_ptr() + 4)}) == _geoprior.EALIGN, key
    assert torch.equal(d["out"], before) and torch.equal(wide["out"], before)             # nothing was launched
    with pytest.raises(_geoprior.MobgtGeopriorError, match="MOBGT_GEOPRIOR_EBADDIM") as e:
        _geoprior.launch("mobgt_geoprior_blend_rows", *(-1 if a == "G" else None if a in POINTERS else 1 for a in ARGS), None)
    assert e.value.code == _geoprior.EBADDIM
    assert _call(d) == 0                                                # and the same buffers are good
    _assert_blended(d, t)


# ------------------------------------------------------------------------------------------------ the public calls
@pytest.fixture(scope="module")
def world():
    """A seeded distance-decay log of 200 POIs: the baseline and the distance prior fitted on its 60 train sessions, the samples
    every prefix of the 12 others; a small untrained fq Graphormer; and the reference of every batch -- test_step's scores, the
    batch's hist, user and y -- on the host."""
    from mobgt_amd.model_fqandtoyo import Graphormer
    coords, sessions, train = gc.decay_log(seed=11, P=200, box_km=12.0, train=360, test=108, length=9)
    sessions = [(s % 20, list(range(1 + 10 * s, 11 + 10 * s))) for s in range(20)] + sessions      # every POI is visited, so has a category
    train = np.r_[np.ones(20, dtype=bool), train]
    ds = data.SessionDataset([(u, pc.as_checkins(p)) for u, p in sessions])
    built = data.build_universe(ds, train=train, coords_deg=coords, radius_km=3.0, device=DEV)
    torch.manual_seed(13)
    args = dict(workloads.COMMON, n_layers=2, hidden_dim=128, dataset_name="foursquaregraph", ffn_dim=256)
    model = Graphormer(universe=built.universe, num_bins=built.bins.num_bins + 2, **args).to(DEV).eval()
    coll = data.SessionCollator(DEV, bin_table=built.bins.table)
    mb = data.MarkovBaseline.fit(ds, train, P=200, device=DEV)
    pb = geo.pair_bins(coords, bins=built.bins, device=DEV)
    samples = data.PrefixDataset(ds, sessions=~train, device=DEV)
    batches = []
    with torch.no_grad():
        for ids in EvalLoop(model, coll, samples, batch_size=8).batches():
            recs = [samples[i] for i in ids]
            b = coll(recs, n_pad=bucket_nodes(max(r.n for r in recs)))
            scores = model.test_step(b)["y_pred"][0]
            batches.append(tuple(v.cpu().numpy() for v in (scores, b.x.reshape(len(recs), -1), b.user.reshape(-1), b.y.reshape(-1))))
    assert built.universe.P == 200 and model.label_offset == 1 and len(samples) >= 60
    assert len({bucket_nodes(samples[i].n) for i in range(len(samples))}) >= 2
    table = torch.from_numpy(np.concatenate([[[0.0, 0.0]], coords]))   # [P + 1, 2]: row 0 the pad POI
    return dict(model=model, coll=coll, mb=mb, pb=pb, samples=samples, batches=batches, coords=table)


def test_fit_on_the_device_is_the_host_fit(world):
    mb, pb = world["mb"], world["pb"]
    dp = mb.distance_prior(pb, distance=0.5)
    u, thr = pb.unit.cpu().numpy(), pb.thresholds.cpu().numpy()
    g = mb.graph
    n = geoprior.pair_hist_host(u, thr)
    t = geoprior.csr_hist_host(u, thr, g.rowptr.cpu().numpy(), g.col.cpu().numpy(), g.val.cpu().numpy())
    assert dp.pair_counts.dtype == np.int64 and dp.pair_counts.tolist() == n.tolist() and int(n.sum()) == 200 * 200
    assert dp.transition_counts.tolist() == t.tolist() and int(t.sum()) == int(g.val.sum()) == 360 + 180
    assert dp.table.device.type == "cuda" and dp.table.dtype == torch.float32
    assert np.array_equal(bits(dp.table.cpu().numpy()), bits(geoprior.table_from_counts(n, t))) and np.array_equal(bits(dp.tables().table), bits(dp.table.cpu().numpy()))
    assert dp.weights.tolist() == [0.5] and dp.status.tolist() == [0] and dp.device == mb.device
    table = dp.curve()[3]
    assert table[1:5].mean() > table[len(table) // 2:].mean()           # near bins are favoured: the log was drawn that way
    with pytest.raises(ValueError, match="the baseline is on cuda:0, the bins on cpu"):
        mb.distance_prior(pb.to("cpu"))
    broken = data.MarkovBaseline.fit(*mb._fitted_on, P=200, device=DEV)
    broken.graph.col[3] = 200
    with pytest.raises(ValueError, match=rf"DistancePrior.fit: .*\(status {geoprior.SBADINDEX}\)"):
        broken.distance_prior(pb)


def test_the_public_blend_and_a_captured_graph(world):
    dp = world["mb"].distance_prior(world["pb"], distance=0.75)
    t = dp.tables()
    G, V = 16, 201
    hist = gc.hist_rows(G, 200)
    scores = pc.scores(G, V)
    want = geoprior.blend_host(scores, hist, t, 0.75, 1)
    s = up(scores)
    assert dp.blend(s, up(hist), 1) is s and np.array_equal(bits(s.cpu().numpy()), bits(want))
    W = up(np.array([[9.0], [-2.0]], dtype=F))
    out = torch.full((G, V + 2), POISON, device=DEV)
    dp.blend(up(scores), (up(hist).long(), torch.ones(G, dtype=torch.int64, device=DEV)), 0, out=out, weights=W[1])
    assert np.array_equal(bits(out.cpu().numpy()[:, :V]), bits(geoprior.blend_host(scores, hist, t, -2.0, 0))) and bool((out[:, V:] == POISON).all())
    src, dst, h = up(scores), torch.zeros(G, V, device=DEV), up(hist)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.blend(src, h, 1, out=dst)
    torch.cuda.current_stream().wait_stream(stream)
    dp.set_weights(distance=3.0)
    graph.replay()
    torch.cuda.synchronize()
    assert dp.get_weights() == dict(distance=3.0)
    assert np.array_equal(bits(dst.cpu().numpy()), bits(geoprior.blend_host(scores, hist, t, 3.0, 1)))
    # a stack on the device: the members' host rules in turn
    mp = world["mb"].prior(0.75, 1.5, 0.3)
    user = np.arange(1, G + 1, dtype=np.int32)
    st = prior.Stack(mp, dp)
    got = st.blend(up(scores), (up(hist), up(user)), 1)
    turn = geoprior.blend_host(prior.blend_host(scores, hist, user, mp.tables(), (0.75, 1.5, 0.3), 1), hist, t, 3.0, 1)
    assert np.array_equal(bits(got.cpu().numpy()), bits(turn))
    W4 = up(np.array([[9, 9, 9, 9], [0.5, 0.25, 2.0, -1.0]], dtype=F))
    out = torch.full((G, V + 2), POISON, device=DEV)
    st.blend(up(scores), (up(hist), up(user)), 1, out=out, weights=W4[1])
    turn = geoprior.blend_host(prior.blend_host(scores, hist, user, mp.tables(), (0.5, 0.25, 2.0), 1), hist, t, -1.0, 1)
    assert np.array_equal(bits(out.cpu().numpy()[:, :V]), bits(turn)) and bool((out[:, V:] == POISON).all())
    st.check()


# ------------------------------------------------------------------------------------------------ the loops
COUNTS = ("n", "acc@1", "acc@5", "acc@10", "acc@20")
SUMS = ("ndcg@1", "ndcg@5", "ndcg@10", "ndcg@20", "mrr")
MARKOV = dict(user=1.0, transition=2.0, popularity=0.5)
DISTANCE = 4.0


def _same(got, want):
    for k in COUNTS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in SUMS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)


def _reference(world, markov, distance):
    """test_step scores -> the members' blend_host in turn -> metrics.restricted_sums, batch by batch -> the loop's dict"""
    mt, dt = world["mb"].prior().tables(), world["mb"].distance_prior(world["pb"]).tables()
    total, blended = None, []
    for scores, hist, user, y in world["batches"]:
        s = scores
        if markov is not None:
            s = prior.blend_host(s, hist, user, mt, markov, 1)
        if distance is not None:
            s = geoprior.blend_host(s, hist, dt, distance, 1)
        blended.append(s)
        sums = metrics.restricted_sums(torch.from_numpy(s), torch.from_numpy(y), target_offset=-1, hist=torch.from_numpy(hist).long(), hist_offset=1)
        total = sums if total is None else total + sums
    return metrics.finalize(total[0, :10]), blended


def _stack(world, distance=DISTANCE):
    return prior.Stack(world["mb"].prior(**MARKOV), world["mb"].distance_prior(world["pb"], distance))


def test_eval_loop_with_a_stack(world):
    kw = dict(batch_size=8)
    st = _stack(world)
    loop = EvalLoop(world["model"], world["coll"], world["samples"], prior=st, **kw)
    got = loop.run()
    eager = EvalLoop(world["model"], world["coll"], world["samples"], use_graph=False, prior=st, **kw).run()
    assert loop.captures >= 2 and got == eager                          # two buckets at least, key for key
    w = tuple(MARKOV[k] for k in prior.WEIGHTS)
    want, _ = _reference(world, w, DISTANCE)
    _same(got, want)
    assert got["n"] == len(world["samples"]) and all(p.status.tolist() == [0] for p in st.priors)
    assert got["mrr"] != _reference(world, w, None)[0]["mrr"] and got["mrr"] != _reference(world, None, None)[0]["mrr"]     # the term counts
    assert world["model"].evaluate(world["samples"], world["coll"], prior=st, **kw) == got
    # new weights need no new capture
    captures = loop.captures
    st.set_weights(distance=-1.5)
    second = loop.run()
    assert loop.captures == captures and second != got
    assert second == EvalLoop(world["model"], world["coll"], world["samples"], prior=_stack(world, -1.5), **kw).run()
    _same(second, _reference(world, w, -1.5)[0])


def test_a_sweep_over_the_stack_is_its_single_runs(world):
    W = [[1.0, 2.0, 0.5, 4.0], [0.0, 0.25, 2.0, 0.0], [0.0, 0.0, 0.0, 1.0], [0.5, 0.0, 0.0, -3.0]]
    st = _stack(world, 7.0)
    got = EvalLoop(world["model"], world["coll"], world["samples"], batch_size=8, prior=st, prior_weights=W).run()
    assert isinstance(got, list) and len(got) == 4
    for row, one in zip(W, got):
        single = prior.Stack(world["mb"].prior(*row[:3]), world["mb"].distance_prior(world["pb"], row[3]))
        assert one == EvalLoop(world["model"], world["coll"], world["samples"], batch_size=8, prior=single).run()
    assert len({r["mrr"] for r in got}) == 4 and st.get_weights()["distance"] == 7.0   # the stack's own weights are not touched
    with pytest.raises(ValueError, match=r"\[L, 4\] rows of \(user, transition, popularity, distance\) weights"):
        EvalLoop(world["model"], world["coll"], world["samples"], batch_size=8, prior=st, prior_weights=[[1.0, 2.0, 0.5]])
    results = st.tune(world["model"], world["coll"], world["samples"], W, batch_size=8)
    best = max(range(4), key=lambda i: (results[i]["mrr"], -i))
    assert results == got and st.get_weights() == dict(zip(st.WEIGHTS, W[best]))


def test_a_bare_distance_prior_in_both_loops(world):
    dp = world["mb"].distance_prior(world["pb"], DISTANCE)
    kw = dict(batch_size=8)
    got = EvalLoop(world["model"], world["coll"], world["samples"], prior=dp, **kw).run()
    _same(got, _reference(world, None, DISTANCE)[0])
    assert got == EvalLoop(world["model"], world["coll"], world["samples"], prior=prior.Stack(dp), **kw).run()
    sweep = EvalLoop(world["model"], world["coll"], world["samples"], prior=dp, prior_weights=[[DISTANCE], [0.0]], **kw).run()
    assert sweep[0] == got and sweep[1] != got
    # the lists are the host top-k of the blended scores, restricted to the unvisited POIs within 2 km of the anchor
    k, V = 10, world["model"].out_proj.out_features
    rkw = dict(exclude_visited=True, within_km=2.0, coords=world["coords"])
    loop = PredictLoop(world["model"], world["coll"], world["samples"], k=k, prior=dp, **kw, **rkw)
    idx, ids, vals = loop.run()
    assert idx.tolist() == [i for b in loop.batches() for i in b] and loop.captures >= 2
    pos = ops.pack_positions(world["coords"], V, 1)
    _, blended = _reference(world, None, DISTANCE)
    row, short = 0, 0
    for s, (_, hist, _, _) in zip(blended, world["batches"]):
        x = torch.from_numpy(hist).long()
        words = ops.near_words(pos, x, 1, ops.chord2_of_km(2.0), "last")
        wi, wv = ops.topk_rows(torch.from_numpy(s), k, col_offset=1, allow=words, exclude=x)
        assert torch.equal(ids[row:row + len(s)].cpu(), wi), row
        assert torch.equal(vals[row:row + len(s)].cpu().view(torch.int32), wv.view(torch.int32)), row
        row += len(s)
        short += int((wi == -1).sum())
    assert row == len(ids) and bool((ids >= 0).any())
    eager = PredictLoop(world["model"], world["coll"], world["samples"], k=k, use_graph=False, prior=prior.Stack(dp), **kw, **rkw).run()
    assert torch.equal(eager[1], ids) and torch.equal(eager[2].view(torch.int32), vals.view(torch.int32))
    plain = PredictLoop(world["model"], world["coll"], world["samples"], k=k, **kw, **rkw).run()
    assert not torch.equal(plain[1], ids)                               # the prior moved a list
