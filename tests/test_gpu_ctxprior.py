"""The context prior on the device (csrc_ctxprior/ctxprior.hip through mobgt_amd.ctxprior) against the host forms, compared
EXACTLY -- integer histograms as lists, blended scores as uint32 views, no tolerance anywhere: slot_hist with sessions on either
side of a wave of pairs, of a workgroup's step of sessions and of one pass of the grid, with the cells on either side of the LDS
histogram's limit, on contended cells and on broken offsets, slots and categories; blend_rows on either side of its chunk, both
label offsets, int32 and int64 ids, padded leading dimensions, in place and out of place, every invalid context and the table
sizes up to MAX_CAT; every return code with nothing launched; ContextPrior.fit; and the loops: EvalLoop / PredictLoop with a
prior.Stack of three and a bare ContextPrior, captured and eager, against the host rules on the downloaded scores, set_weights
without a new capture, the weight sweep and the maximum-likelihood fit of the stack's six weights."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import anchor_cases as ac
import ctxprior_cases as cc
import geoprior_cases as gc
import prior_cases as pc
from mobgt_amd import _ctxprior, ctxprior, data, geo, geoprior, metrics, ops, prior, priorfit, workloads
from mobgt_amd.data import bucket_nodes
from mobgt_amd.train import EvalLoop, PredictLoop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK, THREADS, LDS_CELLS, SESSIONS, MAX_GRID, MAX_CAT, MAX_SLOTS = (getattr(_ctxprior, k) for k in (
    "CHUNK", "THREADS", "LDS_CELLS", "SESSIONS", "MAX_GRID", "MAX_CAT", "MAX_SLOTS"))
POISON = 77.0
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def up(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


def ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else v


def _run(name, *args):
    rc = getattr(_ctxprior.LIBRARY.lib(), name)(*(ptr(a) for a in args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------ slot_hist
def slot_hist(seq, offsets, train, S, C, status=None, n_sessions=None):
    counts = torch.full((S * C,), -7, dtype=torch.int64, device=DEV)    # (poisoned: the call clears it)
    status = torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status
    n = len(train) if n_sessions is None else n_sessions
    assert _run("mobgt_ctxprior_slot_hist", up(seq), len(seq), up(offsets), n, up(train), S, C, counts, status) == 0
    return counts.cpu().numpy().reshape(S, C), status


SHAPES = {"one pair": [2], "63 sessions": [2] * (SESSIONS - 1), "64 sessions": [2] * SESSIONS, "65 sessions": [2] * (SESSIONS + 1),
          "63 pairs": [64], "64 pairs": [65], "65 pairs": [66], "one long session": [5000],
          "a second pass of the grid": [2] * (SESSIONS * MAX_GRID + 3),
          "mixed": list(np.random.RandomState(9).randint(0, 13, size=300)) + [200, 1, 0, 2]}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_slot_hist_counts_what_the_host_counts(shape):
    lengths = SHAPES[shape]
    S, C = 48, 12
    for train in (0.7, 1.0, 0.0):                                       # some train, all train, no train
        seq, offsets, flags = cc.packed(lengths, S, C, seed=len(lengths), train=train)
        host = [0]
        want = ctxprior.slot_hist_host(seq, offsets, flags, S, C, status=host)
        got, status = slot_hist(seq, offsets, flags, S, C)
        assert got.tolist() == want.tolist() and status.tolist() == host == [0]
        pairs = int(sum(max(int(n) - 1, 0) for n, t in zip(lengths, flags) if t))
        assert int(got.sum()) == pairs and (train != 0.0 or pairs == 0) and (train != 1.0 or pairs >= 1)


def test_slot_hist_of_no_sessions_clears_the_counts():
    seq, offsets, flags = cc.packed([3, 4], 5, 4)
    got, status = slot_hist(seq, offsets[:1], flags[:0], 5, 4)
    assert got.tolist() == [[0] * 4] * 5 and status.tolist() == [0]
    got, status = slot_hist(seq[:0], np.zeros(3, dtype=np.int64), flags, 5, 4)             # two empty sessions, no row
    assert got.tolist() == [[0] * 4] * 5 and status.tolist() == [0]


@pytest.mark.parametrize("S,C", ((31, 1057), (32, 1024), (9, 3641), (1, 1), (MAX_SLOTS, MAX_CAT)))
def test_slot_hist_on_either_side_of_the_lds_limit(S, C):
    assert S * C in (LDS_CELLS - 1, LDS_CELLS, LDS_CELLS + 1, 1, MAX_SLOTS * MAX_CAT)
    seq, offsets, flags = cc.packed([2, 9, 2, 40, 3] * 40, S, C, seed=S, train=0.8)
    seq[-1, 2], seq[-2, 1] = C, S - 1                                   # the last cell is counted into
    flags[-1] = 1
    want = ctxprior.slot_hist_host(seq, offsets, flags, S, C)
    got, status = slot_hist(seq, offsets, flags, S, C)
    assert np.array_equal(got, want) and status.tolist() == [0] and got[S - 1, C - 1] >= 1 and int(got.sum()) == int(want.sum()) >= 1


@pytest.mark.parametrize("S,C", ((48, 12), (9, 3641)))                 # the LDS form and the global form
def test_slot_hist_with_every_pair_in_one_cell(S, C):
    seq, offsets, flags = cc.packed([20000] + [8] * 3000, S, C, train=1.0)
    seq[:, 1], seq[:, 2] = S - 2, C - 1
    got, status = slot_hist(seq, offsets, flags, S, C)
    assert got[S - 2, C - 2] == 19999 + 7 * 3000 == int(got.sum()) and status.tolist() == [0]
    assert np.array_equal(got, ctxprior.slot_hist_host(seq, offsets, flags, S, C))


def test_slot_hist_skips_and_flags():
    """None of these inputs is read out of bounds: an offsets pair is checked before it bounds a walk, a slot and a category
    before they index a cell."""
    S, C = 6, 5
    seq, offsets, flags = cc.packed([4, 70, 5, 2, 9], S, C, seed=3, train=1.0)
    clean = ctxprior.slot_hist_host(seq, offsets, flags, S, C)
    down, beyond, before = offsets.copy(), offsets.copy(), offsets.copy()
    down[2] = offsets[1] - 1                                            # session 1 descends (session 2 then starts early: valid)
    beyond[5] = len(seq) + 7                                            # the last session runs beyond M
    before[0] = -1                                                      # the first starts before the log
    for off in (down, beyond, before):
        host = [0]
        want = ctxprior.slot_hist_host(seq, off, flags, S, C, status=host)
        got, status = slot_hist(seq, off, flags, S, C)
        assert host == [ctxprior.SBADINDEX] and status.tolist() == host and got.tolist() == want.tolist()
        assert 0 < int(got.sum()) and want.tolist() != clean.tolist()   # a session was skipped, and the others still count
        again, status = slot_hist(seq, offsets, flags, S, C, status=status)                # a clean call on the same word
        assert again.tolist() == clean.tolist() and status.tolist() == [ctxprior.SBADINDEX]   # not cleared
    got, status = slot_hist(seq, beyond, np.array([1, 1, 1, 1, 0], dtype=np.uint8), S, C)  # a broken session out of train is flagged too
    assert status.tolist() == [ctxprior.SBADINDEX]
    for column, value in ((1, -1), (1, S), (2, 0), (2, C + 1)):
        bad = seq.copy()
        bad[30, column] = value                                         # inside session 1: second row of one pair, first of the next
        host = [0]
        want = ctxprior.slot_hist_host(bad, offsets, flags, S, C, status=host)
        status = torch.full((1,), 4, dtype=torch.int32, device=DEV)
        got, status = slot_hist(bad, offsets, flags, S, C, status=status)
        assert host == [ctxprior.SBADVALUE] and status.tolist() == [4 | ctxprior.SBADVALUE], (column, value)      # ORed into
        assert got.tolist() == want.tolist() and int(got.sum()) == int(clean.sum()) - 1


def test_slot_hist_return_codes_with_nothing_launched():
    S, C = 6, 5
    seq, offsets, flags = cc.packed([4, 7, 5], S, C, train=1.0)
    d_seq, d_off, d_train = up(seq), up(offsets), up(flags)
    counts = torch.full((S * C,), -7, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    null = ctypes.c_void_p(0)
    call = lambda seq=d_seq, M=len(seq), off=d_off, n=3, train=d_train, S=S, C=C, out=counts, st=status: \
        _run("mobgt_ctxprior_slot_hist", seq, M, off, n, train, S, C, out, st)
    for kw in (dict(M=-1), dict(M=2 ** 31), dict(n=-1), dict(n=2 ** 31), dict(S=0), dict(S=MAX_SLOTS + 1), dict(C=0), dict(C=MAX_CAT + 1)):
        assert call(**kw) == _ctxprior.EBADDIM, kw
    for key, t, odd in (("seq", d_seq, 2), ("off", d_off, 4), ("out", counts, 4), ("st", status, 2)):
        assert call(**{key: null}) == call(**{key: ctypes.c_void_p(t.data_ptr() + odd)}) == _ctxprior.EALIGN, key
    assert call(train=null) == _ctxprior.EALIGN
    assert counts.tolist() == [-7] * (S * C) and status.tolist() == [0]     # nothing was launched, nothing cleared
    with pytest.raises(_ctxprior.MobgtCtxpriorError, match="MOBGT_CTXPRIOR_EBADDIM") as e:
        _ctxprior.launch("mobgt_ctxprior_slot_hist", None, 0, None, 0, None, 0, 1, None, None, None)
    assert e.value.code == _ctxprior.EBADDIM
    assert call() == 0 and counts.cpu().numpy().reshape(S, C).tolist() == ctxprior.slot_hist_host(seq, offsets, flags, S, C).tolist()


# ------------------------------------------------------------------------------------------------ blend_rows
BLEND_P = CHUNK + 2
ARGS = ("scores", "ld_scores", "out", "ld_out", "G", "V", "label_offset", "hist", "hist_dtype", "ld_hist", "n_hist_cols", "time", "cat",
        "ctx_dtype", "ld_ctx", "poi_cat", "P", "cat_table", "slot_table", "n_cat", "n_slots", "weights")
POINTERS = ("scores", "out", "hist", "time", "cat", "poi_cat", "cat_table", "slot_table", "weights")
WEIGHTS = (0.75, -1.25)


@functools.lru_cache(maxsize=2)
def tables(P=BLEND_P, C=12, S=48):
    return cc.tables(P, C, S, seed=C + S)


@functools.lru_cache(maxsize=2)
def device_tables(P=BLEND_P, C=12, S=48):
    t = tables(P, C, S)
    return up(t.poi_cat), up(t.cat_table), up(t.slot_table)


def _direct(t, G, V, label_offset=1, wide=False, ctx_wide=None, in_place=False, weights=WEIGHTS, seed=0, P=BLEND_P):
    """Device buffers and sizes of a direct call: {argument: tensor or int}, and the host inputs under "host".  wide: int64 ids;
    ctx_wide: int64 slots and categories (default: as the ids).  Every row of scores and out is three columns wider than V and
    holds POISON there; hist is three columns wider than its n, time and cat five."""
    ctx_wide = wide if ctx_wide is None else ctx_wide
    dtype, ctx = (np.int64 if wide else np.int32), (np.int64 if ctx_wide else np.int32)
    hist, time, cat = cc.sample_rows(G, t.P, t.n_cat, t.n_slots, seed=seed, dtype=dtype, ctx_dtype=ctx)
    scores = pc.scores(G, V, seed=seed)
    n = hist.shape[1]
    code = lambda w: _ctxprior.I64 if w else _ctxprior.I32
    d = dict(G=G, V=V, label_offset=label_offset, hist_dtype=code(wide), ctx_dtype=code(ctx_wide), n_hist_cols=n, ld_hist=n + 3, ld_ctx=n + 5,
             P=t.P, n_cat=t.n_cat, n_slots=t.n_slots, ld_scores=V + 3, ld_out=V + 3)
    d["hist"] = up(np.concatenate([hist, np.full((G, 3), 5, dtype=dtype)], axis=1))        # (the columns beyond n hold an id: not read)
    d["time"] = up(np.concatenate([time, np.full((G, 5), 1, dtype=ctx)], axis=1))
    d["cat"] = up(np.concatenate([cat, np.full((G, 5), 1, dtype=ctx)], axis=1))
    d["poi_cat"], d["cat_table"], d["slot_table"] = device_tables(t.P, t.n_cat, t.n_slots)
    d["weights"] = up(np.array([9.0, *weights], dtype=F))[1:]           # a view into a longer buffer
    d["scores"] = up(np.concatenate([scores, np.full((G, 3), POISON, dtype=F)], axis=1))
    d["out"] = d["scores"] if in_place else torch.full((G, V + 3), POISON, dtype=torch.float32, device=DEV)
    d["host"] = (scores, hist, time, cat)
    return d


def _call(d, **over):
    return _run("mobgt_ctxprior_blend_rows", *(over.get(a, d[a]) for a in ARGS))


def _assert_blended(d, t, weights=WEIGHTS):
    scores, hist, time, cat = d["host"]
    V = d["V"]
    want = ctxprior.blend_host(scores, hist, time, cat, t, weights, d["label_offset"])
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
    """P = CHUNK + 2: the widths are V < P + 1 and V > P + 1.  Rows of V + 3 floats: with V = CHUNK + 1 every row starts 16-byte
    aligned (the four-columns-per-lane form), with the other widths most do not.  16 rows walk through ctxprior_cases.CONTEXTS."""
    t = tables()
    d = _direct(t, G, V, label_offset, wide=form == "out-i64", in_place=form == "in-place-i32", seed=V + G)
    assert _call(d) == 0
    want = _assert_blended(d, t)
    scores, hist, time, cat = d["host"]
    if G == 16:
        changed = bits(want) != bits(scores)
        rows = cc.anchors(hist, time, cat)
        none = [g for g, a in enumerate(rows) if a is None or not 1 <= a[0] <= t.P or not (1 <= a[1] <= t.n_cat or 0 <= a[2] < t.n_slots)]
        assert len(none) >= 5 and not changed[none].any() and not changed[:, BLEND_P + 1 - label_offset:].any()
        if V >= CHUNK - 1:                                              # (V = 1: one column, no POI's at label_offset 0)
            assert changed[[g for g in range(G) if g not in none]].mean(axis=1).min() > 0.3
    if G == 16 and V > CHUNK:
        assert (bits(want) == 0xFFC12345).any() and (bits(want) == 0x80000000).any() and np.isinf(want).any()


@pytest.mark.parametrize("wide", (False, True), ids=("i32", "i64"))
@pytest.mark.parametrize("n", ac.WIDTHS)
def test_the_anchor_search_across_waves_and_strides(n, wide):
    """The history rows of anchor_cases, n ids wide, by direct call: the only id in the first and in the last position, and two
    ids whose positions lie in different waves and strides, the later one deciding.  Slot and category are read AT the anchor
    position: every position carries another valid (slot, category) -- 13 * 48 >= 600 of them -- so a wrong winner shows in
    the output."""
    t = tables(C=13)
    d = _direct(t, ac.G, ac.V, ac.LABEL_OFFSET, wide=wide, seed=n)
    scores = d["host"][0]
    dtype = np.int64 if wide else np.int32
    hist = ac.rows(n, 3, 17, dtype)
    at = np.tile(np.arange(n, dtype=dtype), (ac.G, 1))
    time, cat = at % t.n_slots, 1 + at // t.n_slots
    assert n == 0 or (cat.max() <= t.n_cat and len(set(zip(time[0].tolist(), cat[0].tolist()))) == n)
    assert _call(d, hist=up(hist), n_hist_cols=n, ld_hist=n, time=up(time), cat=up(cat), ld_ctx=n) == 0
    d["host"] = (scores, hist, time, cat)
    want = _assert_blended(d, t)
    if n > 1:
        assert (bits(want[3]) != bits(ctxprior.blend_host(scores, ac.loser(hist), time, cat, t, WEIGHTS, ac.LABEL_OFFSET)[3])).any()


def test_blend_of_no_rows_launches_nothing():
    t = tables()
    d = _direct(t, 0, 40)
    null = ctypes.c_void_p(0)
    assert _call(d) == 0 and _call(d, scores=null, out=null, hist=null, time=null, cat=null) == 0
    d = _direct(t, 3, 0)
    assert _call(d) == 0 and bool((d["out"] == POISON).all())


@pytest.mark.parametrize("S", (1, 48))
@pytest.mark.parametrize("C", (1, 63, 64, 65, THREADS + 1, MAX_CAT))
def test_blend_across_the_table_sizes(C, S):
    """P = 150 < V - 1 + label_offset: columns beyond the POIs are copied; ids of one width, slots and categories of the other."""
    t = tables(150, C, S)
    for lo, V, wide in ((1, 160, False), (0, 163, True)):
        d = _direct(t, 16, V, lo, wide=wide, ctx_wide=not wide, seed=C % 11 + S + V, weights=(-1.5, 0.5))
        assert _call(d) == 0
        want = _assert_blended(d, t, weights=(-1.5, 0.5))
        assert (bits(want) != bits(d["host"][0])).any()


def test_blend_weights_zero_and_the_weights_are_read_on_the_device():
    t = tables()
    d = _direct(t, 16, CHUNK + 1, weights=(0.0, 0.0), seed=3)
    assert _call(d) == 0
    want = _assert_blended(d, t, weights=(0.0, 0.0))
    scores = d["host"][0]
    assert ((want == scores) | (np.isnan(want) & np.isnan(scores))).all()
    flipped = bits(want) != bits(scores)
    assert flipped.any() and ((bits(scores)[flipped] == 0x80000000) & (bits(want)[flipped] == 0)).all()
    assert _call(d, weights=up(np.array([2.5, -0.5], dtype=F))) == 0    # another buffer: the weights are read where the call points
    _assert_blended(d, t, weights=(2.5, -0.5))
    d["weights"].copy_(up(np.array([0.0, 4.0], dtype=F)))               # the same buffer with new values
    assert _call(d) == 0
    _assert_blended(d, t, weights=(0.0, 4.0))


def test_blend_return_codes_with_nothing_launched():
    t = tables()
    G, V = 3, 33
    d = _direct(t, G, V)
    before = d["out"].clone()
    n = d["n_hist_cols"]
    bad = [("G", -1), ("G", 65536), ("V", -1), ("V", 2 ** 31), ("n_hist_cols", -1), ("n_hist_cols", 2 ** 31), ("P", 0), ("P", 2 ** 31),
           ("n_cat", 0), ("n_cat", MAX_CAT + 1), ("n_slots", 0), ("n_slots", MAX_SLOTS + 1), ("ld_scores", V - 1), ("ld_out", V - 1),
           ("ld_hist", n - 1), ("ld_ctx", n - 1), ("label_offset", -1), ("label_offset", 2)]
    for key, value in bad:
        assert _call(d, **{key: value}) == _ctxprior.EBADDIM, (key, value)
    assert _call(d, out=d["scores"], ld_out=V + 4) == _ctxprior.EBADDIM      # in place with another leading dimension
    for key in ("hist_dtype", "ctx_dtype"):
        for value in (-1, 2):
            assert _call(d, **{key: value}) == _ctxprior.EDTYPE, (key, value)
    wide = _direct(t, G, V, wide=True)
    for key in POINTERS:
        assert _call(d, **{key: ctypes.c_void_p(0)}) == _ctxprior.EALIGN, key
        assert _call(d, **{key: ctypes.c_void_p(d[key].data_ptr() + 2)}) == _ctxprior.EALIGN, key
        if key in ("hist", "time", "cat"):                              # 8-byte elements at a 4-byte address
            assert _call(wide, **{key: ctypes.c_void_p(wide[key].data_ptr() + 4)}) == _ctxprior.EALIGN, key
    assert torch.equal(d["out"], before) and torch.equal(wide["out"], before)             # nothing was launched
    with pytest.raises(_ctxprior.MobgtCtxpriorError, match="MOBGT_CTXPRIOR_EBADDIM") as e:
        _ctxprior.launch("mobgt_ctxprior_blend_rows", *(-1 if a == "G" else None if a in POINTERS else 1 for a in ARGS), None)
    assert e.value.code == _ctxprior.EBADDIM
    assert _call(d) == 0                                                # and the same buffers are good
    _assert_blended(d, t)


# ------------------------------------------------------------------------------------------------ the public calls
@pytest.fixture(scope="module")
def world():
    """A seeded context_log of 200 POIs on a city's coordinates: the baseline, the distance prior and the context prior fitted on
    its 80 train sessions, the samples every prefix of the 12 others; a small untrained fq Graphormer; and the reference of every
    batch -- test_step's scores, the batch's x, user, time, cat and y -- on the host."""
    from mobgt_amd.model_fqandtoyo import Graphormer
    sessions, _, poi_cat = cc.context_log(seed=11, P=200, sessions=72, length=9)
    cover = [(s % 20, np.array([(p, (7 * p) % 48, poi_cat[p - 1]) for p in range(1 + 10 * s, 11 + 10 * s)])) for s in range(20)]
    sessions = cover + sessions                                         # every POI is visited, so has a category
    train = np.arange(len(sessions)) < 80
    coords = gc.city(200, seed=11, box_km=12.0, special=False)
    ds = data.SessionDataset(sessions)
    built = data.build_universe(ds, train=train, coords_deg=coords, radius_km=3.0, device=DEV)
    torch.manual_seed(13)
    args = dict(workloads.COMMON, n_layers=2, hidden_dim=128, dataset_name="foursquaregraph", ffn_dim=256)
    model = Graphormer(universe=built.universe, num_bins=built.bins.num_bins + 2, **args).to(DEV).eval()
    coll = data.SessionCollator(DEV, bin_table=built.bins.table)
    mb = data.MarkovBaseline.fit(ds, train, P=200, device=DEV)
    pb = geo.pair_bins(coords, bins=built.bins, device=DEV)
    cp = data.ContextPrior.fit(ds, train, counts=built.counts, device=DEV)
    samples = data.PrefixDataset(ds, sessions=~train, device=DEV)
    batches = []
    with torch.no_grad():
        for ids in EvalLoop(model, coll, samples, batch_size=8).batches():
            recs = [samples[i] for i in ids]
            b = coll(recs, n_pad=bucket_nodes(max(r.n for r in recs)))
            scores = model.test_step(b)["y_pred"][0]
            G = len(recs)
            assert b.time.dtype == b.cat.dtype == torch.int32 and b.time.shape == b.cat.shape == b.x.shape == (G, b.x.shape[1], 1)
            batches.append(tuple(v.cpu().numpy() for v in (scores, b.x.reshape(G, -1), b.user.reshape(-1), b.time.reshape(G, -1),
                                                           b.cat.reshape(G, -1), b.y.reshape(-1))))
    assert built.universe.P == 200 and model.label_offset == 1 and len(samples) >= 60 and cp.n_slots == 48 and cp.n_cat == 12
    assert len({bucket_nodes(samples[i].n) for i in range(len(samples))}) >= 2
    return dict(model=model, coll=coll, mb=mb, pb=pb, cp=cp, ds=ds, train=train, counts=built.counts, samples=samples, batches=batches)


def test_fit_on_the_device_is_the_host_fit(world):
    ds, train, counts = world["ds"], world["train"], world["counts"]
    cp = data.ContextPrior.fit(ds, train, category=0.5, time=2.0, device=DEV)              # counts=None: universe_counts of its own
    host = data.ContextPrior.fit(ds, train, device="cpu")
    for got in (cp, world["cp"]):                                       # ... and given: the same prior
        assert got.slot_cat.dtype == np.int64 and got.slot_cat.tolist() == host.slot_cat.tolist() and int(got.slot_cat.sum()) == 80 * 9
        assert got.graph_cat.tolist() == host.graph_cat.tolist() == counts.graph_cat.tolist()
        assert got.cat_table.device.type == "cuda" and got.cat_table.dtype == got.slot_table.dtype == torch.float32
        assert np.array_equal(bits(got.cat_table.cpu().numpy()), bits(host.cat_table.numpy()))
        assert np.array_equal(bits(got.slot_table.cpu().numpy()), bits(host.slot_table.numpy()))
        assert np.array_equal(bits(got.tables().slot_table), bits(host.tables().slot_table))
        assert got.poi_cat.tolist() == host.poi_cat.tolist() == counts.poi_cat.tolist() and got.status.tolist() == [0]
        assert (got.P, got.n_cat, got.n_slots) == (200, 12, 48) and got.device == counts.poi_cat.device
    assert cp.weights.tolist() == [0.5, 2.0] and world["cp"].poi_cat.data_ptr() == counts.poi_cat.data_ptr()
    with pytest.raises(ValueError, match="the counts are on cuda:0, the prior is fitted on cpu"):
        data.ContextPrior.fit(ds, train, counts=counts, device="cpu")
    with pytest.raises(TypeError, match="a PrefixDataset holds every transition of a session once per prefix"):
        data.ContextPrior.fit(world["samples"], train, device=DEV)


def test_every_prior_refuses_out_at_scores_with_another_row_stride(world):
    """In place means out IS scores: an `out` that starts where scores starts with another row stride is refused by all three
    priors alike, on the host, before a launch (the entry points' own EBADDIM is pinned by their return-code tests)."""
    buf = torch.zeros(2, 8, device=DEV)
    scores, out = buf[:, :3], torch.as_strided(buf, (2, 3), (4, 1))
    ids = torch.tensor([[4, 9, 0], [7, 0, 0]], dtype=torch.int32, device=DEV)
    batch = types.SimpleNamespace(x=ids, user=torch.ones(2, dtype=torch.int32, device=DEV), time=ids, cat=ids)
    for p in (world["mb"].prior(), world["mb"].distance_prior(world["pb"]), world["cp"]):
        with pytest.raises(ValueError, match=f"{type(p).__name__}.blend: .*in place means out is scores"):
            p.blend(scores, batch, 1, out=out)
        p.check()
    torch.cuda.synchronize()
    assert not buf.any()


def test_the_public_blend_and_a_captured_graph(world):
    cp = data.ContextPrior.fit(world["ds"], world["train"], counts=world["counts"], category=0.75, time=-1.25, device=DEV)
    t = cp.tables()
    G, V = 16, 201
    hist, time, cat = cc.sample_rows(G, 200, 12, 48)
    scores = pc.scores(G, V)
    want = ctxprior.blend_host(scores, hist, time, cat, t, WEIGHTS, 1)
    s = up(scores)
    assert cp.blend(s, (up(hist), up(time), up(cat)), 1) is s and np.array_equal(bits(s.cpu().numpy()), bits(want))
    W = up(np.array([[9.0, 9.0], [-2.0, 0.5]], dtype=F))
    out = torch.full((G, V + 2), POISON, device=DEV)
    batch = types.SimpleNamespace(x=up(hist).long()[:, :, None], time=up(time)[:, :, None], cat=up(cat)[:, :, None])
    assert cp.blend(up(scores), batch, 0, out=out, weights=W[1]) is out
    assert np.array_equal(bits(out.cpu().numpy()[:, :V]), bits(ctxprior.blend_host(scores, hist, time, cat, t, (-2.0, 0.5), 0)))
    assert bool((out[:, V:] == POISON).all())
    src, dst, rows = up(scores), torch.zeros(G, V, device=DEV), (up(hist), up(time), up(cat))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        cp.blend(src, rows, 1, out=dst)
    torch.cuda.current_stream().wait_stream(stream)
    cp.set_weights(category=3.0, time=0.25)
    graph.replay()
    torch.cuda.synchronize()
    assert cp.get_weights() == dict(category=3.0, time=0.25)
    assert np.array_equal(bits(dst.cpu().numpy()), bits(ctxprior.blend_host(scores, hist, time, cat, t, (3.0, 0.25), 1)))
    # a stack of three on the device: the members' host rules in turn
    mp, dp = world["mb"].prior(0.75, 1.5, 0.3), world["mb"].distance_prior(world["pb"], 2.0)
    user = np.arange(1, G + 1, dtype=np.int32)
    st = prior.Stack(mp, dp, cp)
    assert st.WEIGHTS == ("user", "transition", "popularity", "distance", "category", "time")
    batch = types.SimpleNamespace(x=up(hist), user=up(user), time=up(time), cat=up(cat))

    def turn(wm, wd, wc):
        s = prior.blend_host(scores, hist, user, mp.tables(), wm, 1)
        return ctxprior.blend_host(geoprior.blend_host(s, hist, dp.tables(), wd, 1), hist, time, cat, t, wc, 1)
    got = st.blend(up(scores), batch, 1)
    assert np.array_equal(bits(got.cpu().numpy()), bits(turn((0.75, 1.5, 0.3), 2.0, (3.0, 0.25))))
    W6 = up(np.array([[9] * 6, [0.5, 0.25, 2.0, -1.0, 1.5, -0.5]], dtype=F))
    out = torch.full((G, V + 2), POISON, device=DEV)
    st.blend(up(scores), batch, 1, out=out, weights=W6[1])
    assert np.array_equal(bits(out.cpu().numpy()[:, :V]), bits(turn((0.5, 0.25, 2.0), -1.0, (1.5, -0.5)))) and bool((out[:, V:] == POISON).all())
    st.check()


# ------------------------------------------------------------------------------------------------ the loops
COUNTS = ("n", "acc@1", "acc@5", "acc@10", "acc@20")
SUMS = ("ndcg@1", "ndcg@5", "ndcg@10", "ndcg@20", "mrr")
MARKOV = dict(user=1.0, transition=2.0, popularity=0.5)
DISTANCE = 4.0
CONTEXT = (1.5, 0.75)
KW = dict(batch_size=8)


def _same(got, want):
    for k in COUNTS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in SUMS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)


def _reference(world, markov, distance, context):
    """test_step scores -> the members' blend_host in turn -> metrics.restricted_sums, batch by batch -> the loop's dict"""
    mt, dt, ct = world["mb"].prior().tables(), world["mb"].distance_prior(world["pb"]).tables(), world["cp"].tables()
    total, blended = None, []
    for scores, hist, user, time, cat, y in world["batches"]:
        s = scores
        if markov is not None:
            s = prior.blend_host(s, hist, user, mt, markov, 1)
        if distance is not None:
            s = geoprior.blend_host(s, hist, dt, distance, 1)
        if context is not None:
            s = ctxprior.blend_host(s, hist, time, cat, ct, context, 1)
        blended.append(s)
        sums = metrics.restricted_sums(torch.from_numpy(s), torch.from_numpy(y), target_offset=-1, hist=torch.from_numpy(hist).long(), hist_offset=1)
        total = sums if total is None else total + sums
    return metrics.finalize(total[0, :10]), blended


def _context(world, weights=CONTEXT):
    cp = world["cp"]
    return ctxprior.ContextPrior(cp.poi_cat, cp.graph_cat, cp.slot_cat, cp.tables().cat_table, cp.tables().slot_table, *weights)


def _stack(world, context=CONTEXT):
    return prior.Stack(world["mb"].prior(**MARKOV), world["mb"].distance_prior(world["pb"], DISTANCE), _context(world, context))


def test_eval_loop_with_a_stack_of_three(world):
    model, coll, samples = (world[k] for k in ("model", "coll", "samples"))
    st = _stack(world)
    loop = EvalLoop(model, coll, samples, prior=st, **KW)
    got = loop.run()
    eager = EvalLoop(model, coll, samples, use_graph=False, prior=st, **KW).run()
    assert loop.captures >= 2 and got == eager                          # two buckets at least, key for key
    w = tuple(MARKOV[k] for k in prior.WEIGHTS)
    want, _ = _reference(world, w, DISTANCE, CONTEXT)
    _same(got, want)
    assert got["n"] == len(samples) and all(p.status.tolist() == [0] for p in st.priors)
    two = prior.Stack(*st.priors[:2])
    assert got["mrr"] != EvalLoop(model, coll, samples, prior=two, **KW).run()["mrr"] != _reference(world, None, None, None)[0]["mrr"]
    assert got["mrr"] != _reference(world, w, DISTANCE, None)[0]["mrr"]  # the terms count
    assert model.evaluate(samples, coll, prior=st, **KW) == got
    # new weights need no new capture
    captures = loop.captures
    st.set_weights(time=-1.5)
    second = loop.run()
    assert loop.captures == captures and second != got
    assert second == EvalLoop(model, coll, samples, prior=_stack(world, (CONTEXT[0], -1.5)), **KW).run()
    _same(second, _reference(world, w, DISTANCE, (CONTEXT[0], -1.5))[0])


def test_a_sweep_over_the_stack_is_its_single_runs(world):
    model, coll, samples = (world[k] for k in ("model", "coll", "samples"))
    W = [[1.0, 2.0, 0.5, 4.0, 1.5, 0.75], [0.0, 0.25, 2.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0, 2.0, 0.0], [0.5, 0.0, 0.0, -3.0, -1.0, 3.0]]
    st = _stack(world, (7.0, 7.0))
    got = EvalLoop(model, coll, samples, prior=st, prior_weights=W, **KW).run()
    assert isinstance(got, list) and len(got) == 4
    for row, one in zip(W, got):
        single = prior.Stack(world["mb"].prior(*row[:3]), world["mb"].distance_prior(world["pb"], row[3]), _context(world, row[4:]))
        assert one == EvalLoop(model, coll, samples, prior=single, **KW).run()
    assert len({r["mrr"] for r in got}) == 4 and st.get_weights()["time"] == 7.0       # the stack's own weights are not touched
    with pytest.raises(ValueError, match=r"\[L, 6\] rows of \(user, transition, popularity, distance, category, time\) weights"):
        EvalLoop(model, coll, samples, prior=st, prior_weights=[[1.0, 2.0, 0.5, 4.0]], **KW)
    results = st.tune(model, coll, samples, W, **KW)
    best = max(range(4), key=lambda i: (results[i]["mrr"], -i))
    assert results == got and st.get_weights() == dict(zip(st.WEIGHTS, W[best]))


def test_a_bare_context_prior_in_both_loops(world):
    model, coll, samples = (world[k] for k in ("model", "coll", "samples"))
    cp = _context(world)
    got = EvalLoop(model, coll, samples, prior=cp, **KW).run()
    _same(got, _reference(world, None, None, CONTEXT)[0])
    assert got == EvalLoop(model, coll, samples, prior=prior.Stack(cp), **KW).run()
    sweep = EvalLoop(model, coll, samples, prior=cp, prior_weights=[list(CONTEXT), [0.0, 0.0]], **KW).run()
    assert sweep[0] == got and sweep[1] != got
    results = cp.tune(model, coll, samples, [[0.0, 0.0], list(CONTEXT)], **KW)
    best = max(range(2), key=lambda i: (results[i]["mrr"], -i))
    assert results == sweep[::-1] and cp.get_weights() == dict(zip(cp.WEIGHTS, ([0.0, 0.0], list(CONTEXT))[best]))
    cp.set_weights(*CONTEXT)
    # the lists are the host top-k of the blended scores, restricted to the unvisited POIs
    k = 10
    loop = PredictLoop(model, coll, samples, k=k, prior=cp, exclude_visited=True, **KW)
    idx, ids, vals = loop.run()
    assert idx.tolist() == [i for b in loop.batches() for i in b] and loop.captures >= 2
    _, blended = _reference(world, None, None, CONTEXT)
    row = 0
    for s, (_, hist, _, _, _, _) in zip(blended, world["batches"]):
        wi, wv = ops.topk_rows(torch.from_numpy(s), k, col_offset=1, exclude=torch.from_numpy(hist).long())
        assert torch.equal(ids[row:row + len(s)].cpu(), wi), row
        assert torch.equal(vals[row:row + len(s)].cpu().view(torch.int32), wv.view(torch.int32)), row
        row += len(s)
    assert row == len(ids) and bool((ids >= 0).any())
    eager = PredictLoop(model, coll, samples, k=k, use_graph=False, prior=prior.Stack(cp), exclude_visited=True, **KW).run()
    assert torch.equal(eager[1], ids) and torch.equal(eager[2].view(torch.int32), vals.view(torch.int32))
    plain = PredictLoop(model, coll, samples, k=k, exclude_visited=True, **KW).run()
    assert not torch.equal(plain[1], ids)                               # the prior moved a list


def test_fit_weights_on_the_stack_of_three(world):
    """K = 7 (the model's scale and six weights) <= MOBGT_PRIORFIT_MAX_K.  The optimum of a strictly convex J is unique: with both
    gradients <= tol = 1e-7 the device fit and fit_host on the downloaded scores and features differ by at most about 1e-6; the
    gate is test_gpu_priorfit's 1e-5."""
    model, coll, samples = (world[k] for k in ("model", "coll", "samples"))
    make = lambda: prior.Stack(world["mb"].prior(), world["mb"].distance_prior(world["pb"]), _context(world, (1.0, 1.0)))
    twin = make()
    assert twin.n_weights + 1 == 7 <= priorfit.MAX_K
    V = model.out_proj.out_features
    scores, feats, y = [], [], []
    with torch.no_grad():
        for ids in EvalLoop(model, coll, samples, **KW).batches():
            recs = [samples[i] for i in ids]
            b = coll(recs, n_pad=bucket_nodes(max(r.n for r in recs)))
            scores.append(model.poi_scores(model.encode(b)).cpu().numpy())
            feats.append(twin.features(b, 1, torch.zeros(6, len(recs), V, device=DEV)).cpu().numpy())
            y.append(b.y.reshape(-1).cpu().numpy())
    scores, feats, y = np.concatenate(scores), np.concatenate(feats, axis=1), np.concatenate(y)
    for scale_model in (True, False):                                   # (an untrained model's scale may come out <= 0: nothing is written then)
        st, twin = make(), make()
        ev = EvalLoop(model, coll, samples, prior=st, **KW)
        before = ev.run()
        captures = ev.captures
        res = st.fit_weights(model, coll, samples, scale_model=scale_model, **KW)
        want = priorfit.fit_host(scores, feats, y, target_offset=-1, prior=twin, scale_model=scale_model)
        print(f"scale_model={scale_model}: passes {res.passes} (host {want.passes}), grad {res.grad:.2e}, scale {res.scale:.4f}, "
              f"weights {res.weights}, nll {res.nll_start:.4f} -> {res.nll:.4f}")
        assert res.converged and want.converged and res.passes <= 12 and res.grad <= 1e-7 and res.n == want.n == len(samples)
        assert res.nll < res.nll_start and len(res.history) == res.passes
        assert abs(res.scale - want.scale) <= 1e-5 and max(abs(res.weights[k] - want.weights[k]) for k in st.WEIGHTS) <= 1e-5
        assert res.applied == want.applied == (res.scale > 0)
        got = st.get_weights()
        assert len(got) == 6 and all(np.isfinite(v) for v in got.values())
        if res.applied:
            assert got == {k: float(np.float32(res.weights[k] / res.scale)) for k in st.WEIGHTS}
            after = ev.run()                                            # the evaluation's graphs read the new weights, no new capture
            assert ev.captures == captures and after != before
            assert after == EvalLoop(model, coll, samples, prior=make().set_weights(**got), **KW).run()
        else:
            assert got == twin.get_weights() == dict.fromkeys(st.WEIGHTS, 1.0)
        assert scale_model or res.applied                               # without the scale the fit is always written
