"""The visit prior on the device (csrc_visitprior/visitprior.hip through mobgt_amd.visitprior) against the host forms, compared
EXACTLY -- counts as lists, tables and blended scores as uint32 views, no tolerance anywhere: the fit on every packed log of
visitprior_cases; blend_rows on either side of its chunk and of the 16-byte form, both label offsets, int32 and int64 ids, in
place and into a buffer with another row stride, rows that hit every branch of the rule and tables that fit does not make; every
return code with nothing launched; the weights read on the device and a captured graph replayed with new ones; and the loops:
EvalLoop / PredictLoop with a prior.Stack of four against the host rules on the downloaded scores, the weight sweep, and the
maximum-likelihood fit of the stack's eight weights.

A column is c = col + 1 - label_offset with col >= 0 and label_offset 0 or 1, so no valid entry falls below column 0: that
branch of the rule is met by the col = -1 entry of the broken tables only."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import geoprior_cases as gc
import prior_cases as pc
import visitprior_cases as vc
from mobgt_amd import _visitprior, ctxprior, data, geo, geoprior, metrics, ops, prior, priorfit, visitprior, workloads
from mobgt_amd.data import bucket_nodes
from mobgt_amd.train import EvalLoop, PredictLoop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK, THREADS = _visitprior.CHUNK, _visitprior.THREADS
POISON = 77.0
F = np.float32
LOGS = vc.logs()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def up(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


def ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else v


def _run(name, *args):
    rc = getattr(_visitprior.LIBRARY.lib(), name)(*(ptr(a) for a in args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("name", list(LOGS))
def test_the_device_fit_is_the_host_fit(name):
    sessions, train, P = LOGS[name]
    ds = vc.dataset(*vc.pack(sessions))
    want = visitprior.visit_counts_host(ds, train, P=P)
    vp = data.VisitPrior.fit(ds, train, P=P, visits=0.5, recency=2.0, device=DEV)
    got = vp.counts()
    assert vp.device == torch.device(DEV) and vp.rowptr.dtype == torch.int64 and vp.col.dtype == torch.int32 and vp.status.tolist() == [0]
    assert (got.rowptr.tolist(), got.col.tolist(), got.cnt.tolist(), got.age.tolist(), got.tot.tolist()) == \
        (want.rowptr.tolist(), want.col.tolist(), want.cnt.tolist(), want.age.tolist(), want.tot.tolist())
    assert (vp.U, vp.P) == (want.U, want.P) == (got.U, got.P) and vp.weights.tolist() == [0.5, 2.0]
    freq, rec = visitprior.tables_from_counts(want.rowptr, want.cnt, want.age, want.tot)
    assert vp.freq.dtype == vp.rec.dtype == torch.float32 and vp.freq.device == vp.rec.device == vp.col.device
    assert np.array_equal(bits(vp.freq.cpu().numpy()), bits(freq)) and np.array_equal(bits(vp.rec.cpu().numpy()), bits(rec))
    host = data.VisitPrior.fit(ds, train, P=P, device="cpu")
    assert np.array_equal(bits(host.freq.numpy()), bits(freq)) and host.col.tolist() == got.col.tolist()
    if name == "mixed":
        assert vp.U == 13 and int(want.tot[2]) > THREADS and int(np.diff(want.rowptr)[4]) == P == vc.LOG_P == 2 * CHUNK + 3


def test_the_fit_launches_flag_what_the_host_should_have_refused():
    """mobgt_visitprior_keys by direct call: a POI beyond P, a user beyond U and a session index beyond S skip their rows, leave
    their keys at -1 and raise their bits; the others are written."""
    sessions = [(0, [1, 2, 3]), (1, [2, 2]), (0, [3, 1])]
    seq, offsets, users = vc.pack(sessions)
    sid = np.repeat(np.arange(3, dtype=np.int32), np.diff(offsets))
    slot0, ord0 = np.array([0, 3, 5], dtype=np.int64), np.array([0, 0, 3], dtype=np.int64)
    P, U, M, T = 3, 2, 7, 7

    def keys(seq=seq, sid=sid, users=users):
        k = torch.full((T,), 5, dtype=torch.int64, device=DEV)
        o = torch.full((T,), -9, dtype=torch.int32, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert _run("mobgt_visitprior_keys", up(seq), up(sid), M, up(offsets[:-1]), up(slot0), up(ord0), up(users), 3, P, U, k, o, T, st) == 0
        return k.tolist(), o.tolist(), st.tolist()
    good = ([0, 1, 2, 4, 4, 2, 0], [0, 1, 2, 0, 1, 3, 4], [0])
    assert keys() == good
    bad = seq.copy()
    bad[1, 0] = 4
    k, o, st = keys(seq=bad)
    assert st == [visitprior.SBADVALUE] and k == [0, -1, 2, 4, 4, 2, 0] and o[:1] + o[2:] == good[1][:1] + good[1][2:]
    k, o, st = keys(users=np.array([0, 2, 0], dtype=np.int64))
    assert st == [visitprior.SBADVALUE] and k == [0, 1, 2, -1, -1, 2, 0]
    wild = sid.copy()
    wild[6] = 3
    k, o, st = keys(sid=wild)
    assert st == [visitprior.SBADINDEX] and k == [0, 1, 2, 4, 4, 2, -1]
    null = ctypes.c_void_p(0)
    args = lambda **kw: [kw.get(a, d) for a, d in (("seq", up(seq)), ("sid", up(sid)), ("M", M), ("first", up(offsets[:-1])), ("slot0", up(slot0)),
                                                    ("ord0", up(ord0)), ("users", up(users)), ("S", 3), ("P", P), ("U", U),
                                                    ("keys", torch.zeros(T, dtype=torch.int64, device=DEV)),
                                                    ("ord", torch.zeros(T, dtype=torch.int32, device=DEV)), ("T", T),
                                                    ("status", torch.zeros(1, dtype=torch.int32, device=DEV)))]
    for kw in (dict(M=-1), dict(M=2 ** 31), dict(S=-1), dict(T=2 ** 31), dict(P=0), dict(P=2 ** 31), dict(U=-1), dict(U=2 ** 31)):
        assert _run("mobgt_visitprior_keys", *args(**kw)) == _visitprior.EBADDIM, kw
    for key in ("seq", "sid", "first", "slot0", "ord0", "users", "keys", "ord", "status"):
        assert _run("mobgt_visitprior_keys", *args(**{key: null})) == _visitprior.EALIGN, key
    z64, z32 = torch.zeros(8, dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    fill = lambda **kw: _run("mobgt_visitprior_fill", *[kw.get(a, d) for a, d in (("keys", z64), ("ord", z32), ("pos", z64), ("T", 4), ("P", P),
                                                                                   ("U", U), ("nnz", 2), ("tot", z32), ("rowptr", z64), ("col", z32),
                                                                                   ("cnt", z32), ("age", z32), ("status", z32))])
    for kw in (dict(T=-1), dict(nnz=5), dict(nnz=-1), dict(P=0), dict(U=2 ** 31)):
        assert fill(**kw) == _visitprior.EBADDIM, kw
    for key in ("keys", "ord", "pos", "tot", "rowptr", "col", "cnt", "age", "status"):
        assert fill(**{key: null}) == _visitprior.EALIGN, key
    assert not z64.any() and not z32.any()                              # nothing was launched


# ------------------------------------------------------------------------------------------------ blend_rows
BLEND_P = 2 * CHUNK + 3
WIDTHS = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
ARGS = ("scores", "ld_scores", "out", "ld_out", "G", "V", "label_offset", "hist", "hist_dtype", "ld_hist", "n_hist_cols", "user", "user_dtype",
        "ld_user", "user_offset", "rowptr", "col", "freq", "rec", "nnz", "U", "P", "weights", "status")
POINTERS = ("scores", "out", "hist", "user", "rowptr", "col", "freq", "rec", "weights", "status")
WEIGHTS = (0.75, -1.25)


@functools.lru_cache(maxsize=1)
def tables():
    rowptr, col, freq, rec, U = vc.tables(BLEND_P, CHUNK, WIDTHS)
    return visitprior.VisitTables(rowptr, col, freq, rec, U, BLEND_P)


@functools.lru_cache(maxsize=1)
def device_tables():
    t = tables()
    return up(t.rowptr), up(t.col), up(t.freq), up(t.rec)


def _direct(G, V, label_offset=1, wide=False, form="out", weights=WEIGHTS, seed=0):
    """Device buffers and sizes of a direct call: {argument: tensor or int}, and the host inputs under "host".  wide: int64 ids.
    form "in-place": out is scores, rows of V + 3 floats; "out": scores rows of V + 3 and out rows of V + 5 floats (odd strides:
    most rows start off a 16-byte boundary); "aligned": rows of a multiple of four floats, 4 and 8 beyond V (every row starts on
    one).  Every column from V on holds POISON.  hist is passed and not read: it holds ids beyond P."""
    t = tables()
    dtype = np.int64 if wide else np.int32
    user = vc.users_of_rows(G, t.U, dtype)
    scores = pc.scores(G, V, seed=seed)
    code = _visitprior.I64 if wide else _visitprior.I32
    up4 = (V + 3) // 4 * 4
    ld_s, ld_o = {"in-place": (V + 3, V + 3), "out": (V + 3, V + 5), "aligned": (up4 + 4, up4 + 8)}[form]
    d = dict(G=G, V=V, label_offset=label_offset, hist_dtype=code, user_dtype=code, n_hist_cols=2, ld_hist=5, ld_user=2, user_offset=1,
             nnz=len(t.col), U=t.U, P=t.P, ld_scores=ld_s, ld_out=ld_o)
    d["hist"] = up(np.full((G, 5), 2 ** 30, dtype=dtype))
    d["user"] = up(np.stack([user, np.full(G, 3, dtype=dtype)], 1))     # (ld_user = 2: the column beside holds a user, not read)
    d["rowptr"], d["col"], d["freq"], d["rec"] = device_tables()
    d["weights"] = up(np.array([9.0, *weights], dtype=F))[1:]           # a view into a longer buffer
    d["status"] = torch.zeros(1, dtype=torch.int32, device=DEV)
    d["scores"] = up(np.concatenate([scores, np.full((G, ld_s - V), POISON, dtype=F)], axis=1))
    d["out"] = d["scores"] if form == "in-place" else torch.full((G, ld_o), POISON, dtype=torch.float32, device=DEV)
    d["host"] = (scores, user)
    return d


def _call(d, **over):
    return _run("mobgt_visitprior_blend_rows", *(over.get(a, d[a]) for a in ARGS))


def _assert_blended(d, t=None, weights=WEIGHTS, status=0):
    t = tables() if t is None else t
    scores, user = d["host"]
    V = d["V"]
    host = [0]
    want = visitprior.blend_host(scores, user, t, weights, d["label_offset"], status=host)
    got = d["out"].cpu().numpy()
    assert np.array_equal(bits(got[:, :V]), bits(want))                 # every element inside is the rule's, NaN payloads included
    assert np.all(got[:, V:] == POISON)                                 # and nothing beyond V was touched
    if d["out"] is not d["scores"]:
        kept = d["scores"].cpu().numpy()
        assert np.array_equal(bits(kept[:, :V]), bits(scores)) and np.all(kept[:, V:] == POISON)
    assert d["status"].tolist() == host == [status]
    return want


@pytest.mark.parametrize("form", ("in-place-i32", "out-i64", "aligned-i32"))
@pytest.mark.parametrize("label_offset", (0, 1))
@pytest.mark.parametrize("G", (1, 3, 16))
@pytest.mark.parametrize("V", WIDTHS)
def test_blend_equals_the_host_rule(V, G, label_offset, form):
    """P = 2 * CHUNK + 3 >= every V: entries at or beyond column V are skipped.  16 rows walk through visitprior_cases.tables'
    users (none, one entry, all P POIs twice, the edges, the first and the last POI, more entries than threads) and through
    users 0, U + 1, negative and far beyond the table."""
    t = tables()
    kind, ids = form.rsplit("-", 1)
    d = _direct(G, V, label_offset, wide=ids == "i64", form=kind, seed=V + G)
    if kind == "aligned":                                               # (every row on a 16-byte boundary; with odd strides row 1 is not)
        assert all((d[k].data_ptr() | 4 * d["ld_" + k]) % 16 == 0 for k in ("scores", "out"))
    assert _call(d) == 0
    want = _assert_blended(d)
    scores, user = d["host"]
    changed = bits(want) != bits(scores)
    if V >= CHUNK - 1:
        assert changed[0].mean() > 0.5                                  # row 0 is the user with all P POIs
    if G == 16:
        none = [g for g, u in enumerate(user) if not 1 <= u <= t.U or t.rowptr[u] == t.rowptr[u - 1]]
        assert len(none) >= 6 and not changed[none].any() and (V < CHUNK - 1 or changed[6].mean() > 0.5)   # row 6: that user again
        edges = (t.col[t.rowptr[3]:t.rowptr[4]] + 1 - label_offset).tolist()               # the columns of user 3, row 2
        for c in (0, CHUNK - 1, CHUNK, V - 1):                          # (column 0 is no POI's with label_offset 0)
            if 0 <= c - 1 + label_offset and c < V:
                assert c in edges and (changed[2, c] or not np.isfinite(scores[2, c])), c
        assert V in edges or V - 1 + label_offset >= t.P                # ... and an entry just beyond the last column
    if G == 16 and V > CHUNK:
        assert (bits(want) == 0xFFC12345).any() and (bits(want) == 0x80000000).any() and np.isinf(want).any()


def test_blend_of_no_rows_launches_nothing():
    d = _direct(0, 40)
    null = ctypes.c_void_p(0)
    assert _call(d) == 0 and _call(d, scores=null, out=null, hist=null, user=null) == 0
    d = _direct(3, 0)
    assert _call(d) == 0 and bool((d["out"] == POISON).all()) and d["status"].tolist() == [0]


def test_blend_weights_zero_and_the_weights_are_read_on_the_device():
    d = _direct(16, CHUNK + 1, weights=(0.0, 0.0), seed=3)
    assert _call(d) == 0
    want = _assert_blended(d, weights=(0.0, 0.0))
    scores = d["host"][0]
    assert ((want == scores) | (np.isnan(want) & np.isnan(scores))).all()
    flipped = bits(want) != bits(scores)
    assert flipped.any() and ((bits(scores)[flipped] == 0x80000000) & (bits(want)[flipped] == 0)).all()
    assert _call(d, weights=up(np.array([2.5, -0.5], dtype=F))) == 0    # another buffer: the weights are read where the call points
    _assert_blended(d, weights=(2.5, -0.5))
    d["weights"].copy_(up(np.array([0.0, 4.0], dtype=F)))               # the same buffer with new values
    assert _call(d) == 0
    _assert_blended(d, weights=(0.0, 4.0))


@pytest.mark.parametrize("form", ("in-place", "out"))
def test_blend_flags_tables_that_fit_does_not_make(form):
    """A rowptr pair that descends, one beyond nnz and one from before the table make their row count as empty; the entries of
    col outside [0, P), at the ends of the row of all P POIs and at the start of a short row, are skipped; each raises SBADINDEX and the rest is blended.  None of
    these is read out of bounds: a pair is checked before it bounds a search, an entry before it is a column."""
    t = tables()
    at = np.arange(t.U + 1)
    V = CHUNK + 1
    for rowptr in (np.where(at == t.U, t.rowptr[-2] - 1, t.rowptr), np.where(at == t.U, len(t.col) + 1, t.rowptr), np.where(at == 0, -1, t.rowptr)):
        d = _direct(16, V, form=form, seed=5)
        assert _call(d, rowptr=up(rowptr)) == 0
        _assert_blended(d, t._replace(rowptr=rowptr), status=visitprior.SBADINDEX)
    col = t.col.copy()
    col[t.rowptr[2]], col[t.rowptr[3] - 1] = -1, t.P                    # still ascending
    assert col[t.rowptr[3]] == 0 and 1 < t.rowptr[4] - t.rowptr[3] <= THREADS < t.rowptr[3] - t.rowptr[2]
    col[t.rowptr[3]] = -1                                               # ... and the first entry of a short row, which is not searched
    d = _direct(16, t.P + 2, form=form, seed=6)
    d["status"].fill_(4)
    assert _call(d, col=up(col)) == 0
    scores, user = d["host"]
    want = visitprior.blend_host(scores, user, t._replace(col=col), WEIGHTS, 1)
    clean = visitprior.blend_host(scores, user, t, WEIGHTS, 1)
    got = d["out"].cpu().numpy()
    assert np.array_equal(bits(got[:, :t.P + 2]), bits(want)) and d["status"].tolist() == [4 | visitprior.SBADINDEX]       # ORed into
    differ = np.nonzero((bits(want) != bits(clean)).any(axis=0))[0]
    assert set(differ.tolist()) <= {0, t.P - 1} and len(differ) >= 1 and np.all(got[:, t.P + 2:] == POISON)
    assert _call(d) == 0 and d["status"].tolist() == [4 | visitprior.SBADINDEX]            # a clean call does not clear the word


def test_blend_return_codes_with_nothing_launched():
    G, V = 3, 33
    d = _direct(G, V)
    before = d["out"].clone()
    bad = [("G", -1), ("G", 65536), ("V", -1), ("V", 2 ** 31), ("n_hist_cols", -1), ("n_hist_cols", 2 ** 31), ("P", 0), ("P", 2 ** 31),
           ("U", -1), ("U", 2 ** 31), ("U", 2 ** 62 // BLEND_P + 1), ("nnz", -1), ("nnz", 2 ** 31), ("ld_scores", V - 1), ("ld_out", V - 1),
           ("ld_hist", 1), ("ld_user", 0), ("label_offset", -1), ("label_offset", 2), ("user_offset", -1), ("user_offset", 2)]
    for key, value in bad:
        assert _call(d, **{key: value}) == _visitprior.EBADDIM, (key, value)
    assert _call(d, out=d["scores"], ld_out=V + 4) == _visitprior.EBADDIM      # in place with another leading dimension
    for key in ("hist_dtype", "user_dtype"):
        for value in (-1, 2):
            assert _call(d, **{key: value}) == _visitprior.EDTYPE, (key, value)
    wide = _direct(G, V, wide=True)
    for key in POINTERS:
        assert _call(d, **{key: ctypes.c_void_p(0)}) == _visitprior.EALIGN, key
        assert _call(d, **{key: ctypes.c_void_p(d[key].data_ptr() + 2)}) == _visitprior.EALIGN, key
        if key in ("hist", "user", "rowptr"):                           # 8-byte elements at a 4-byte address
            assert _call(wide, **{key: ctypes.c_void_p(wide[key].data_ptr() + 4)}) == _visitprior.EALIGN, key
    assert torch.equal(d["out"], before) and torch.equal(wide["out"], before) and d["status"].tolist() == [0]    # nothing was launched
    with pytest.raises(_visitprior.MobgtVisitpriorError, match="MOBGT_VISITPRIOR_EBADDIM") as e:
        _visitprior.launch("mobgt_visitprior_blend_rows", *(-1 if a == "G" else None if a in POINTERS else 1 for a in ARGS), None)
    assert e.value.code == _visitprior.EBADDIM
    assert _call(d) == 0                                                # and the same buffers are good
    _assert_blended(d)


# ------------------------------------------------------------------------------------------------ the public calls
@pytest.fixture(scope="module")
def world():
    """A seeded favourites_log of 200 POIs and 20 users on a city's coordinates: the baseline, the distance prior, the context
    prior and the visit prior fitted on its train sessions, the samples every prefix of the others; a small untrained fq
    Graphormer; and the reference of every batch -- test_step's scores, the batch's x, user, time, cat and y -- on the host."""
    from mobgt_amd.model_fqandtoyo import Graphormer
    sessions, mask = vc.favourites_log(seed=11, users=20, P=200, sessions=10, held_out=0.2)
    cover = [(s % 20, np.array([(p, (7 * p) % 48, 1 + p % 12) for p in range(1 + 10 * s, 11 + 10 * s)])) for s in range(20)]
    sessions = cover + sessions                                         # every POI is visited, so has a category
    train = np.concatenate([np.ones(20, dtype=bool), mask])
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
    vp = data.VisitPrior.fit(ds, train, P=200, device=DEV)
    samples = data.PrefixDataset(ds, sessions=~train, device=DEV)
    batches = []
    with torch.no_grad():
        for ids in EvalLoop(model, coll, samples, batch_size=8).batches():
            recs = [samples[i] for i in ids]
            b = coll(recs, n_pad=bucket_nodes(max(r.n for r in recs)))
            scores = model.test_step(b)["y_pred"][0]
            G = len(recs)
            batches.append(tuple(v.cpu().numpy() for v in (scores, b.x.reshape(G, -1), b.user.reshape(-1), b.time.reshape(G, -1),
                                                           b.cat.reshape(G, -1), b.y.reshape(-1))))
    assert built.universe.P == 200 and model.label_offset == 1 and 60 <= len(samples) <= 400 and vp.U == 20 and len(ds) == 220
    return dict(model=model, coll=coll, mb=mb, pb=pb, cp=cp, vp=vp, ds=ds, train=train, samples=samples, batches=batches)


def test_the_public_blend_and_a_captured_graph(world):
    ds, train = world["ds"], world["train"]
    vp = data.VisitPrior.fit(ds, train, P=200, visits=0.75, recency=-1.25, device=DEV)
    host = data.VisitPrior.fit(ds, train, P=200, device="cpu")
    t = vp.tables()
    assert t.col.tolist() == host.tables().col.tolist() and np.array_equal(bits(t.rec), bits(host.tables().rec))
    with pytest.raises(TypeError, match="a PrefixDataset holds every transition of a session once per prefix"):
        data.VisitPrior.fit(world["samples"], train, device=DEV)
    G, V = 16, 201
    user = (np.arange(G) * 3 % 23).astype(np.int32)                     # 0 and 21, 22 are no users of the table
    hist = np.zeros((G, 4), dtype=np.int32)                             # empty histories
    scores = pc.scores(G, V)
    want = visitprior.blend_host(scores, user, t, WEIGHTS, 1)
    s = up(scores)
    assert vp.blend(s, (up(hist), up(user)), 1) is s and np.array_equal(bits(s.cpu().numpy()), bits(want)) and (bits(want) != bits(scores)).any()
    W = up(np.array([[9.0, 9.0], [-2.0, 0.5]], dtype=F))
    out = torch.full((G, V + 2), POISON, device=DEV)
    batch = types.SimpleNamespace(x=up(hist).long()[:, :, None], user=up(user).long()[:, None])
    assert vp.blend(up(scores), batch, 0, out=out, weights=W[1]) is out
    assert np.array_equal(bits(out.cpu().numpy()[:, :V]), bits(visitprior.blend_host(scores, user, t, (-2.0, 0.5), 0)))
    assert bool((out[:, V:] == POISON).all())
    src, dst, rows = up(scores), torch.zeros(G, V, device=DEV), (up(hist), up(user))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        vp.blend(src, rows, 1, out=dst)
    torch.cuda.current_stream().wait_stream(stream)
    vp.set_weights(visits=3.0, recency=0.25)
    graph.replay()
    torch.cuda.synchronize()
    assert vp.get_weights() == dict(visits=3.0, recency=0.25)
    assert np.array_equal(bits(dst.cpu().numpy()), bits(visitprior.blend_host(scores, user, t, (3.0, 0.25), 1)))
    vp.check()
    # the constructor's check runs on the tables' device
    swapped = vp.col.clone()
    swapped[:2] = vp.col[:2].flip(0)
    with pytest.raises(ValueError, match="col must ascend strictly inside every row"):
        visitprior.VisitPrior(200, vp.rowptr, swapped, vp.cnt, vp.age, vp.tot, t.freq, t.rec)
    with pytest.raises(ValueError, match="rowptr is on cuda:0, col on cpu"):
        visitprior.VisitPrior(200, vp.rowptr, vp.col.cpu(), vp.cnt, vp.age, vp.tot, t.freq, t.rec)


# ------------------------------------------------------------------------------------------------ the loops
COUNTS = ("n", "acc@1", "acc@5", "acc@10", "acc@20")
SUMS = ("ndcg@1", "ndcg@5", "ndcg@10", "ndcg@20", "mrr")
MARKOV = dict(user=1.0, transition=2.0, popularity=0.5)
DISTANCE = 4.0
CONTEXT = (1.5, 0.75)
VISIT = (2.0, 1.25)
KW = dict(batch_size=8)


def _same(got, want):
    for k in COUNTS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in SUMS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)


def _reference(world, markov, distance, context, visit):
    """test_step scores -> the members' blend_host in turn -> metrics.restricted_sums, batch by batch -> the loop's dict"""
    mt, dt = world["mb"].prior().tables(), world["mb"].distance_prior(world["pb"]).tables()
    ct, vt = world["cp"].tables(), world["vp"].tables()
    total, blended = None, []
    for scores, hist, user, time, cat, y in world["batches"]:
        s = scores
        if markov is not None:
            s = prior.blend_host(s, hist, user, mt, markov, 1)
        if distance is not None:
            s = geoprior.blend_host(s, hist, dt, distance, 1)
        if context is not None:
            s = ctxprior.blend_host(s, hist, time, cat, ct, context, 1)
        if visit is not None:
            s = visitprior.blend_host(s, user, vt, visit, 1)
        blended.append(s)
        sums = metrics.restricted_sums(torch.from_numpy(s), torch.from_numpy(y), target_offset=-1, hist=torch.from_numpy(hist).long(), hist_offset=1)
        total = sums if total is None else total + sums
    return metrics.finalize(total[0, :10]), blended


def _visit(world, weights=VISIT):
    vp = world["vp"]
    return visitprior.VisitPrior(vp.P, vp.rowptr, vp.col, vp.cnt, vp.age, vp.tot, vp.tables().freq, vp.tables().rec, *weights)


def _context(world, weights=CONTEXT):
    cp = world["cp"]
    return ctxprior.ContextPrior(cp.poi_cat, cp.graph_cat, cp.slot_cat, cp.tables().cat_table, cp.tables().slot_table, *weights)


def _stack(world, visit=VISIT):
    return prior.Stack(world["mb"].prior(**MARKOV), world["mb"].distance_prior(world["pb"], DISTANCE), _context(world), _visit(world, visit))


def test_eval_loop_with_a_stack_of_four(world):
    model, coll, samples = (world[k] for k in ("model", "coll", "samples"))
    st = _stack(world)
    assert st.WEIGHTS == ("user", "transition", "popularity", "distance", "category", "time", "visits", "recency")
    loop = EvalLoop(model, coll, samples, prior=st, **KW)
    got = loop.run()
    eager = EvalLoop(model, coll, samples, use_graph=False, prior=st, **KW).run()
    assert loop.captures >= 1 and got == eager
    w = tuple(MARKOV[k] for k in prior.WEIGHTS)
    want, _ = _reference(world, w, DISTANCE, CONTEXT, VISIT)
    _same(got, want)
    assert got["n"] == len(samples) and all(p.status.tolist() == [0] for p in st.priors)
    three = prior.Stack(*st.priors[:3])
    assert got["mrr"] != EvalLoop(model, coll, samples, prior=three, **KW).run()["mrr"]                # the fourth member counts
    assert got["mrr"] != _reference(world, w, DISTANCE, CONTEXT, None)[0]["mrr"]
    assert model.evaluate(samples, coll, prior=st, **KW) == got
    # new weights need no new capture
    captures = loop.captures
    st.set_weights(recency=-1.5)
    second = loop.run()
    assert loop.captures == captures and second != got
    assert second == EvalLoop(model, coll, samples, prior=_stack(world, (VISIT[0], -1.5)), **KW).run()
    _same(second, _reference(world, w, DISTANCE, CONTEXT, (VISIT[0], -1.5))[0])


def test_a_sweep_over_the_stack_is_its_single_runs(world):
    model, coll, samples = (world[k] for k in ("model", "coll", "samples"))
    W = [[1.0, 2.0, 0.5, 4.0, 1.5, 0.75, 2.0, 1.25], [0.0, 0.25, 2.0, 0.0, 0.0, 1.0, 0.0, 3.0], [0.5, 0.0, 0.0, -3.0, -1.0, 3.0, 4.0, 0.0]]
    st = _stack(world, (7.0, 7.0))
    got = EvalLoop(model, coll, samples, prior=st, prior_weights=W, **KW).run()
    assert isinstance(got, list) and len(got) == 3
    for row, one in zip(W, got):
        single = prior.Stack(world["mb"].prior(*row[:3]), world["mb"].distance_prior(world["pb"], row[3]), _context(world, row[4:6]),
                             _visit(world, row[6:]))
        assert one == EvalLoop(model, coll, samples, prior=single, **KW).run()
    assert len({r["mrr"] for r in got}) == 3 and st.get_weights()["recency"] == 7.0         # the stack's own weights are not touched
    with pytest.raises(ValueError, match=r"\[L, 8\] rows of \(user, transition, popularity, distance, category, time, visits, recency\) weights"):
        EvalLoop(model, coll, samples, prior=st, prior_weights=[[1.0, 2.0, 0.5, 4.0, 1.0, 1.0]], **KW)


def test_a_bare_visit_prior_in_both_loops(world):
    model, coll, samples = (world[k] for k in ("model", "coll", "samples"))
    vp = _visit(world)
    got = EvalLoop(model, coll, samples, prior=vp, **KW).run()
    _same(got, _reference(world, None, None, None, VISIT)[0])
    assert got == EvalLoop(model, coll, samples, prior=prior.Stack(vp), **KW).run()
    sweep = EvalLoop(model, coll, samples, prior=vp, prior_weights=[list(VISIT), [0.0, 0.0]], **KW).run()
    assert sweep[0] == got and sweep[1] != got
    # the lists are the host top-k of the blended scores, here of the stack of four
    k = 10
    st = _stack(world)
    loop = PredictLoop(model, coll, samples, k=k, prior=st, **KW)
    idx, ids, vals = loop.run()
    assert idx.tolist() == [i for b in loop.batches() for i in b]
    _, blended = _reference(world, tuple(MARKOV[k] for k in prior.WEIGHTS), DISTANCE, CONTEXT, VISIT)
    row = 0
    for s in blended:
        wi, wv = ops.topk_rows(torch.from_numpy(s), k, col_offset=1)
        assert torch.equal(ids[row:row + len(s)].cpu(), wi), row
        assert torch.equal(vals[row:row + len(s)].cpu().view(torch.int32), wv.view(torch.int32)), row
        row += len(s)
    assert row == len(ids) and bool((ids >= 0).any())
    eager = PredictLoop(model, coll, samples, k=k, use_graph=False, prior=st, **KW).run()
    assert torch.equal(eager[1], ids) and torch.equal(eager[2].view(torch.int32), vals.view(torch.int32))
    three = PredictLoop(model, coll, samples, k=k, prior=prior.Stack(*st.priors[:3]), **KW).run()
    assert not torch.equal(three[1], ids)                               # the visit prior moved a list
    recs = model.recommend(samples, coll, k=k, prior=st, **KW)
    assert torch.equal(recs[1], ids)


def test_fit_weights_on_the_stack_of_four(world):
    """Eight weights: with the model's scale they are K = 9 features, one more than MOBGT_PRIORFIT_MAX_K, and the fit is refused
    with PriorFitLoop's message; scale_model=False fits the eight exactly.  The optimum of a strictly convex J is unique: with
    both gradients <= tol = 1e-7 the device fit and fit_host on the downloaded scores and features differ by at most about 1e-6;
    the gate is test_gpu_priorfit's 1e-5."""
    model, coll, samples = (world[k] for k in ("model", "coll", "samples"))
    make = lambda: prior.Stack(world["mb"].prior(), world["mb"].distance_prior(world["pb"]), _context(world, (1.0, 1.0)), _visit(world, (1.0, 1.0)))
    st, twin = make(), make()
    assert st.n_weights == 8 == priorfit.MAX_K
    with pytest.raises(ValueError, match=r"PriorFitLoop: 8 prior weights and the model's scale are 9 features, one launch takes up to 8 "
                                         r"\(MOBGT_PRIORFIT_MAX_K\)"):
        st.fit_weights(model, coll, samples, **KW)
    assert st.get_weights() == dict.fromkeys(st.WEIGHTS, 1.0)
    V = model.out_proj.out_features
    scores, feats, y = [], [], []
    with torch.no_grad():
        for ids in EvalLoop(model, coll, samples, **KW).batches():
            recs = [samples[i] for i in ids]
            b = coll(recs, n_pad=bucket_nodes(max(r.n for r in recs)))
            scores.append(model.poi_scores(model.encode(b)).cpu().numpy())
            feats.append(twin.features(b, 1, torch.zeros(8, len(recs), V, device=DEV)).cpu().numpy())
            y.append(b.y.reshape(-1).cpu().numpy())
    scores, feats, y = np.concatenate(scores), np.concatenate(feats, axis=1), np.concatenate(y)
    ev = EvalLoop(model, coll, samples, prior=st, **KW)
    before = ev.run()
    captures = ev.captures
    res = st.fit_weights(model, coll, samples, scale_model=False, **KW)
    want = priorfit.fit_host(scores, feats, y, target_offset=-1, prior=twin, scale_model=False)
    print(f"passes {res.passes} (host {want.passes}), grad {res.grad:.2e}, weights {res.weights}, nll {res.nll_start:.4f} -> {res.nll:.4f}")
    assert res.converged and want.converged and res.passes <= 12 and res.grad <= 1e-7 and res.n == want.n == len(samples)
    assert res.nll < res.nll_start and max(abs(res.weights[k] - want.weights[k]) for k in st.WEIGHTS) <= 1e-5
    assert res.applied and want.applied
    got = st.get_weights()
    assert got == {k: float(np.float32(res.weights[k])) for k in st.WEIGHTS}
    after = ev.run()                                                    # the evaluation's graphs read the new weights, no new capture
    assert ev.captures == captures and after != before
    assert after == EvalLoop(model, coll, samples, prior=make().set_weights(**got), **KW).run()
