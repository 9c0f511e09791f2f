"""The visit prior's rule on the host (mobgt_amd.visitprior: visit_counts_host, tables_from_counts and blend_host, the references of
the kernels in csrc_visitprior/visitprior.hip; a VisitPrior fitted on the CPU; prior.Stack with the other three): the counts
against a dict-counter loop, the tables against their formulas and the blend against a per-element loop, all compared exactly --
integers as lists, floats as uint32 views; what the constructor and fit refuse; and, on a seeded log of habits, that visit counts
and recency each rank the held-out targets better than popularity and both better than either."""
import types

import numpy as np
import pytest
import torch

import geoprior_cases as gc
import prior_cases as pc
import visitprior_cases as vc
from mobgt_amd import _visitprior, baseline, ctxprior, data, geo, geoprior, prior, priorfit, visitprior

F = np.float32
LOGS = vc.logs()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the counts
@pytest.mark.parametrize("name", list(LOGS))
def test_the_counts_are_the_dict_loop(name):
    sessions, train, P = LOGS[name]
    seq, offsets, users = vc.pack(sessions)
    c = visitprior.visit_counts_host(vc.dataset(seq, offsets, users), train, P=P)
    rowptr, col, cnt, age, tot = vc.loop_counts(seq, offsets, users, train, P)
    assert (c.rowptr.tolist(), c.col.tolist(), c.cnt.tolist(), c.age.tolist(), c.tot.tolist()) == (rowptr, col, cnt, age, tot)
    assert (c.rowptr.dtype, c.col.dtype, c.cnt.dtype, c.age.dtype, c.tot.dtype) == (np.int64, np.int32, np.int32, np.int32, np.int32)
    U = int(users.max()) + 1 if len(users) else 0
    assert (c.U, c.P) == (U, P) and len(c.rowptr) == U + 1 and c.rowptr[0] == 0 and c.rowptr[-1] == len(c.col)
    assert int(c.cnt.sum()) == int(c.tot.sum()) == sum(len(p) for (_, p), t in zip(sessions, train) if t)
    for u in range(U):
        r0, r1 = int(c.rowptr[u]), int(c.rowptr[u + 1])
        mine = c.col[r0:r1]
        assert r1 >= r0 and (np.diff(mine) > 0).all() and (r1 == r0 or (0 <= mine[0] and mine[-1] < P))
        assert (r1 > r0) == (c.tot[u] > 0) and int(c.cnt[r0:r1].sum()) == c.tot[u]
        assert sorted(c.age[r0:r1].tolist())[:1] == [0][:r1 - r0] and len(set(c.age[r0:r1].tolist())) == r1 - r0
        last = [p[-1] for (v, p), t in zip(sessions, train) if t and v == u]
        if last:                                                        # age 0 belongs to the POI of the user's last train check-in
            assert c.age[r0 + mine.tolist().index(last[-1] - 1)] == 0
    # a mask and the indices of the train sessions are one thing
    again = visitprior.visit_counts_host(vc.dataset(seq, offsets, users), np.nonzero(train)[0], P=P)
    assert all(np.array_equal(a, b) for a, b in zip(c[:5], again[:5]))


def test_the_shapes_of_the_mixed_log():
    sessions, train, P = LOGS["mixed"]
    seq, offsets, users = vc.pack(sessions)
    c = visitprior.visit_counts_host(vc.dataset(seq, offsets, users), train, P=P)
    width = np.diff(c.rowptr)
    assert c.U == 13 and width[[0, 6, 12]].tolist() == [0, 0, 0] and c.tot[[0, 6, 12]].tolist() == [0, 0, 0]      # no train session
    assert c.tot[1] == 1 and width[1] == 1                              # the one-row session
    assert c.tot[2] > vc.THREADS and width[3] == 1 and c.cnt[c.rowptr[3]] == c.tot[3] == 7 and c.col[c.rowptr[3]] == 6
    assert width[4] == P == c.tot[4] - 1 and c.cnt[c.rowptr[4]] == 2 and c.age[c.rowptr[4]] == 0
    none = visitprior.visit_counts_host(vc.dataset(seq, offsets, users), LOGS["nothing in train"][1], P=P)
    assert none.U == 13 and len(none.col) == 0 and not none.rowptr.any() and not none.tot.any()


def test_the_tables_are_their_formulas():
    sessions, train, P = LOGS["mixed"]
    c = visitprior.visit_counts_host(vc.dataset(*vc.pack(sessions)), train, P=P)
    freq, rec = visitprior.tables_from_counts(c.rowptr, c.cnt, c.age, c.tot)
    assert freq.dtype == rec.dtype == np.float32 and freq.shape == rec.shape == c.col.shape and (freq > 0).all() and (rec > 0).all()
    table = prior.log_table(int(c.cnt.max()))
    assert np.array_equal(bits(freq), bits(table[c.cnt])) and np.array_equal(bits(freq), bits(np.log1p(c.cnt.astype(np.float64)).astype(F)))
    n = np.repeat(c.tot, np.diff(c.rowptr)).astype(np.float64)
    assert np.array_equal(bits(rec), bits(np.log((n + 1.0) / (c.age.astype(np.float64) + 1.0)).astype(F)))
    for u in range(c.U):                                                # R is largest for the POI visited last
        r0, r1 = int(c.rowptr[u]), int(c.rowptr[u + 1])
        if r1 - r0 > 1:
            assert rec[r0:r1].argmax() == c.age[r0:r1].argmin() and (rec[r0:r1] == rec[r0:r1].max()).sum() == 1
    empty = visitprior.tables_from_counts([0, 0], np.zeros(0, np.int32), np.zeros(0, np.int32), [0])
    assert empty[0].shape == empty[1].shape == (0,) and empty[0].dtype == np.float32
    for bad in (dict(cnt=c.cnt * 0), dict(age=c.age - 1), dict(age=c.age + int(c.tot.max())), dict(rowptr=c.rowptr[::-1].copy()),
                dict(rowptr=c.rowptr[:-1]), dict(cnt=c.cnt.astype(np.float64))):
        with pytest.raises(ValueError, match="tables_from_counts"):
            visitprior.tables_from_counts(**{**dict(rowptr=c.rowptr, cnt=c.cnt, age=c.age, tot=c.tot), **bad})


# ------------------------------------------------------------------------------------------------ the blend
CHUNK = _visitprior.CHUNK
P_BLEND = 2 * CHUNK + 3
WIDTHS = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)


def _tables(P=P_BLEND):
    rowptr, col, freq, rec, U = vc.tables(P, CHUNK, WIDTHS)
    return visitprior.VisitTables(rowptr, col, freq, rec, U, P)


@pytest.mark.parametrize("label_offset", (0, 1))
@pytest.mark.parametrize("V", (1, 5, 37, 60))
@pytest.mark.parametrize("weights", ((0.75, -1.25), (0.0, 0.0), (2.0, 0.0)))
def test_blend_host_is_the_loop(weights, V, label_offset):
    """P = 40: V = 1, 5 and 37 are smaller than the POIs' columns, 60 larger; -0.0, NaN payloads and infinities are sown into
    the scores."""
    t = _tables(40)
    scores = pc.scores(16, V, seed=V)
    for dtype in (np.int32, np.int64):
        user = vc.users_of_rows(16, t.U, dtype)
        status = [4]
        got = visitprior.blend_host(scores, user, t, weights, label_offset, status=status)
        want, bad = vc.loop_blend(scores, user, t.rowptr, t.col, t.freq, t.rec, t.U, t.P, weights, label_offset)
        assert np.array_equal(bits(got), bits(want)) and status == [4] and bad == 0 and got.dtype == np.float32
    changed = bits(got) != bits(scores)
    rows_without = [g for g, u in enumerate(user) if not 1 <= u <= t.U or t.rowptr[u] == t.rowptr[u - 1]]
    assert len(rows_without) >= 6 and not changed[rows_without].any() and not changed[:, 40 + 1 - label_offset:].any()
    if weights == (0.0, 0.0):                                           # a weight of 0 is still added: -0.0 becomes +0.0, nothing else
        assert ((bits(scores)[changed] == 0x80000000) & (bits(got)[changed] == 0)).all()
        if V == 60:
            assert changed.any()
    elif V >= 37:                                                       # (infinities and NaNs stay what they are)
        assert changed[0].mean() > 0.5 and changed[6].mean() > 0.5    # the user with all P POIs, twice
    assert np.array_equal(bits(visitprior.blend_host(scores, user[:, None], t, weights, label_offset)), bits(got))
    if V == 60:
        assert (bits(got) == 0xFFC12345).any() and np.isinf(got).any()
        shifted = visitprior.blend_host(scores, user - 1, t, weights, label_offset, user_offset=0)
        assert np.array_equal(bits(shifted), bits(got))


def test_blend_host_flags_tables_that_fit_does_not_make():
    t = _tables(40)
    scores = pc.scores(16, 41)
    user = vc.users_of_rows(16, t.U)
    clean = visitprior.blend_host(scores, user, t, (1.0, 1.0), 1)
    at = np.arange(t.U + 1)
    # the last pair descending, the last pair beyond nnz, the first pair from before the table: one row each
    for rowptr, row in ((np.where(at == t.U, t.rowptr[-2] - 1, t.rowptr), t.U - 1), (np.where(at == t.U, len(t.col) + 1, t.rowptr), t.U - 1),
                        (np.where(at == 0, -1, t.rowptr), 0)):
        status = [0]
        got = visitprior.blend_host(scores, user, t._replace(rowptr=rowptr), (1.0, 1.0), 1, status=status)
        want, bad = vc.loop_blend(scores, user, rowptr, t.col, t.freq, t.rec, t.U, t.P, (1.0, 1.0), 1)
        assert status == [visitprior.SBADINDEX] and bad == 1 and np.array_equal(bits(got), bits(want))
        mine = user == row + 1                                          # that user's rows count as empty, the others blend
        assert mine.any() and np.array_equal(bits(got[mine]), bits(scores[mine])) and np.array_equal(bits(got[~mine]), bits(clean[~mine]))
    col = t.col.copy()
    col[t.rowptr[2]], col[t.rowptr[3] - 1] = -1, 40                     # the ends of the full row: still ascending
    status = [0]
    got = visitprior.blend_host(scores, user, t._replace(col=col), (1.0, 1.0), 1, status=status)
    want, bad = vc.loop_blend(scores, user, t.rowptr, col, t.freq, t.rec, t.U, t.P, (1.0, 1.0), 1)
    assert status == [visitprior.SBADINDEX] and bad == 1 and np.array_equal(bits(got), bits(want))
    differ = np.nonzero((bits(got) != bits(clean)).any(axis=0))[0]
    assert set(differ.tolist()) <= {0, 39} and len(differ) >= 1         # the two entries are skipped, nothing else changes


# ------------------------------------------------------------------------------------------------ a CPU prior, the stack
@pytest.fixture(scope="module")
def log():
    sessions, mask = vc.favourites_log(seed=0)
    ds = data.SessionDataset(sessions)
    mb = baseline.MarkovBaseline.fit(ds, mask, P=400, device="cpu")
    vp = data.VisitPrior.fit(ds, mask, P=400, device="cpu")
    return sessions, mask, ds, mb, vp


def test_a_prior_fitted_on_the_cpu(log):
    sessions, mask, ds, mb, vp = log
    assert isinstance(vp, visitprior.VisitPrior) and data.VisitPrior is visitprior.VisitPrior and isinstance(vp, prior.Prior)
    c = visitprior.visit_counts_host(ds, mask, P=400)
    rowptr, col, cnt, age, tot = vc.loop_counts(ds.seq, ds.offsets, ds.users, mask, 400)
    assert (vp.P, vp.U) == (400, 30) and vp.device.type == "cpu" and vp.status.tolist() == [0]
    assert (vp.rowptr.tolist(), vp.col.tolist(), vp.cnt.tolist(), vp.age.tolist(), vp.tot.tolist()) == (rowptr, col, cnt, age, tot)
    freq, rec = visitprior.tables_from_counts(c.rowptr, c.cnt, c.age, c.tot)
    assert vp.freq.dtype == torch.float32 and np.array_equal(bits(vp.freq.numpy()), bits(freq)) and np.array_equal(bits(vp.rec.numpy()), bits(rec))
    t = vp.tables()
    assert isinstance(t, visitprior.VisitTables) and np.array_equal(bits(t.freq), bits(freq)) and np.array_equal(bits(t.rec), bits(rec))
    assert t.rowptr.tolist() == rowptr and t.col.tolist() == col and (t.U, t.P) == (30, 400) and vp.counts().age.tolist() == age
    assert vp.weights.tolist() == [1.0, 1.0] and vp.get_weights() == {"visits": 1.0, "recency": 1.0} and vp.n_weights == 2
    assert vp.WEIGHTS == ("visits", "recency")
    given = data.VisitPrior.fit(ds, np.nonzero(mask)[0], visits=0.5, recency=-2.0, device="cpu")      # P: the largest id present
    assert given.P == int(ds.seq[:, 0].max()) and given.weights.tolist() == [0.5, -2.0] and given.cnt.tolist() == cnt
    assert given.set_weights(recency=3.0).weights.tolist() == [0.5, 3.0] and given.set_weights().get_weights() == {"visits": 0.5, "recency": 3.0}
    # the public call of a CPU prior is the host form, in place by default and into `out` otherwise; no history is needed
    user = np.arange(16, dtype=np.int64) * 2                            # 0: no user; 2 .. 30: users 1 .. 29
    hist = np.zeros((16, 3), dtype=np.int64)                            # empty histories: the rows are scored all the same
    scores = pc.scores(16, 401)
    want = visitprior.blend_host(scores, user, t, (1.0, 1.0), 1)
    s = torch.from_numpy(scores.copy())
    assert vp.blend(s, (torch.from_numpy(hist), torch.from_numpy(user)), 1) is s and np.array_equal(bits(s.numpy()), bits(want))
    assert (bits(want)[1:] != bits(scores)[1:]).any(axis=1).all() and not (bits(want)[0] != bits(scores)[0]).any()
    out = torch.full((16, 403), 9.0)
    batch = types.SimpleNamespace(x=torch.from_numpy(hist).int()[:, :, None], user=torch.from_numpy(user).int()[:, None])
    vp.blend(torch.from_numpy(scores.copy()), batch, 0, out=out, weights=torch.tensor([9.0, 0.5, 2.0])[1:])
    assert np.array_equal(bits(out[:, :401].numpy()), bits(visitprior.blend_host(scores, user, t, (0.5, 2.0), 0)))
    assert bool((out[:, 401:] == 9.0).all())
    # features: the table values themselves, 0 where the rule adds nothing
    feats = vp.features((torch.from_numpy(hist), torch.from_numpy(user)), 1, torch.full((2, 16, 401), 5.0))
    assert np.array_equal(bits(feats[0].numpy()), bits(visitprior.blend_host(np.zeros((16, 401), F), user, t, (1.0, 0.0), 1)))
    assert np.array_equal(bits(feats[1].numpy()), bits(visitprior.blend_host(np.zeros((16, 401), F), user, t, (0.0, 1.0), 1)))
    u3 = slice(int(t.rowptr[3]), int(t.rowptr[4]))
    assert np.array_equal(bits(feats[1][2].numpy()[t.col[u3] + 0]), bits(t.rec[u3]))       # row 2 is user 3: column c = col + 1 - 1


def test_a_stack_of_four_is_the_host_rules_in_turn(log):
    sessions, mask, ds, mb, vp = log
    mp = mb.prior(0.75, 1.5, 0.3)
    dp = mb.distance_prior(geo.pair_bins(gc.city(400, seed=2), edges=np.arange(0.0, 30.0, 2.5), device="cpu"), 2.0)
    cp = data.ContextPrior.fit(ds, mask, category=0.6, time=-0.4, device="cpu")
    vp = visitprior.VisitPrior(vp.P, vp.rowptr, vp.col, vp.cnt, vp.age, vp.tot, vp.tables().freq, vp.tables().rec, 1.25, 0.5)
    st = prior.Stack(mp, dp, cp, vp)
    assert st.WEIGHTS == ("user", "transition", "popularity", "distance", "category", "time", "visits", "recency") and st.n_weights == 8
    rng = np.random.RandomState(4)
    hist = rng.randint(1, 401, size=(16, 5)).astype(np.int64)
    hist[3] = 0
    time, cat, user = rng.randint(0, 48, size=(16, 5)), rng.randint(1, 13, size=(16, 5)), np.arange(1, 17)
    scores = pc.scores(16, 401, seed=4)
    batch = types.SimpleNamespace(**{k: torch.from_numpy(v) for k, v in dict(x=hist, user=user, time=time, cat=cat).items()})

    def turn(wm, wd, wc, wv):
        s = prior.blend_host(scores, hist, user, mp.tables(), wm, 1)
        s = ctxprior.blend_host(geoprior.blend_host(s, hist, dp.tables(), wd, 1), hist, time, cat, cp.tables(), wc, 1)
        return visitprior.blend_host(s, user, vp.tables(), wv, 1)
    got = st.blend(torch.from_numpy(scores.copy()), batch, 1)
    assert np.array_equal(bits(got.numpy()), bits(turn((0.75, 1.5, 0.3), 2.0, (0.6, -0.4), (1.25, 0.5))))
    assert (bits(got.numpy())[3] != bits(scores)[3]).any()              # the row without a history is scored by this prior
    W = torch.tensor([[9.0] * 8, [0.5, 0.25, 2.0, -1.0, -1.5, 3.0, 0.0, 4.0]])
    out = torch.full((16, 404), 9.0)
    assert st.blend(torch.from_numpy(scores.copy()), batch, 1, out=out, weights=W[1]) is out
    assert np.array_equal(bits(out[:, :401].numpy()), bits(turn((0.5, 0.25, 2.0), -1.0, (-1.5, 3.0), (0.0, 4.0))))
    assert bool((out[:, 401:] == 9.0).all())
    st.set_weights(recency=2.0, user=0.0)
    assert vp.weights.tolist() == [1.25, 2.0] and mp.weights.tolist()[0] == 0.0
    st.check()
    feats = st.features(batch, 1, torch.full((8, 16, 401), 5.0))
    assert np.array_equal(bits(feats[6].numpy()), bits(visitprior.blend_host(np.zeros((16, 401), F), user, vp.tables(), (1.0, 0.0), 1)))
    # a stack of MarkovPrior and VisitPrior keeps taking (hist, user) pairs
    pair = (torch.from_numpy(hist), torch.from_numpy(user))
    two = prior.Stack(mp, vp).blend(torch.from_numpy(scores.copy()), pair, 1)
    want = visitprior.blend_host(prior.blend_host(scores, hist, user, mp.tables(), (0.0, 1.5, 0.3), 1), user, vp.tables(), (1.25, 2.0), 1)
    assert np.array_equal(bits(two.numpy()), bits(want))
    with pytest.raises(ValueError, match="visits, recency belong to more than one member"):
        prior.Stack(vp, vp)
    assert st.n_weights + 1 > priorfit.MAX_K == 8                      # fit_weights(scale_model=True) has one feature too many


class _Model:
    label_offset = 1
    out_proj = torch.nn.Linear(2, 400)


def test_what_the_visit_prior_refuses(log):
    sessions, mask, ds, mb, vp = log
    with pytest.raises(TypeError, match="a PrefixDataset holds every transition of a session once per prefix"):
        data.VisitPrior.fit(data.PrefixDataset(ds, device="cpu"), mask, device="cpu")
    with pytest.raises(TypeError, match="VisitPrior.fit: the sessions must be a data.SessionDataset"):
        data.VisitPrior.fit(sessions, mask, device="cpu")
    with pytest.raises(ValueError, match=r"POI id \d+ at check-in \d+ is not in 1 .. 399"):
        data.VisitPrior.fit(ds, mask, P=399, device="cpu")
    with pytest.raises(ValueError, match="train: a mask of 3 flags"):
        data.VisitPrior.fit(ds, np.ones(3, dtype=bool), device="cpu")
    far = vc.dataset(*vc.pack([(2 ** 40, [1, 2])]))
    with pytest.raises(ValueError, match=r"do not fit the key of the per-user table \(U \* P < 2\*\*62, U < 2\*\*31\)"):
        visitprior.visit_counts_host(far, [True], P=2)
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match=r"the weights \(visits, recency\) must be finite"):
            data.VisitPrior.fit(ds, mask, recency=bad, device="cpu")
    # the constructor: dtypes, devices, and the order the kernel's bisection relies on
    t = vp.tables()
    make = lambda **kw: visitprior.VisitPrior(**{**dict(P=400, rowptr=vp.rowptr, col=vp.col, cnt=vp.cnt, age=vp.age, tot=vp.tot, freq=t.freq,
                                                        rec=t.rec), **kw})
    assert make().col.tolist() == vp.col.tolist()
    with pytest.raises(TypeError, match="rowptr must be a torch.int64 tensor of one dimension, got torch.int32"):
        make(rowptr=vp.rowptr.int())
    with pytest.raises(TypeError, match="col must be a torch.int32 tensor of one dimension, got torch.int64"):
        make(col=vp.col.long())
    with pytest.raises(TypeError, match="col must be a torch.int32 tensor of one dimension, got ndarray"):
        make(col=t.col)
    with pytest.raises(ValueError, match="rowptr is on cpu, col on meta: the tables live on one device"):
        make(col=vp.col.to("meta"))
    swapped = vp.col.clone()
    r0 = int(vp.rowptr[5])
    swapped[r0], swapped[r0 + 1] = vp.col[r0 + 1], vp.col[r0]
    with pytest.raises(ValueError, match="col must ascend strictly inside every row"):
        make(col=swapped)
    twice = vp.col.clone()
    twice[r0 + 1] = twice[r0]
    with pytest.raises(ValueError, match="col must ascend strictly inside every row"):
        make(col=twice)
    beyond = vp.col.clone()
    beyond[-1] = 400
    with pytest.raises(ValueError, match=r"an entry of col is outside \[0, P\) = \[0, 400\)"):
        make(col=beyond)
    with pytest.raises(ValueError, match="rowptr must ascend from 0 to nnz"):
        make(rowptr=torch.flip(vp.rowptr, [0]))
    with pytest.raises(ValueError, match=r"rowptr \[U \+ 1\], tot \[U\] and col, cnt, age, freq, rec \[nnz\]"):
        make(freq=t.freq[:-1])
    # what every prior refuses, with this prior's name
    with pytest.raises(ValueError, match="must be finite"):
        vp.set_weights(visits=float("nan"))
    assert vp.weights.tolist() == [1.0, 1.0]
    with pytest.raises(ValueError, match="EvalLoop: the prior is on cpu, the loop on cuda:0: fit the prior on the loop's device"):
        vp.for_loop(_Model, "cuda:0", 16, "EvalLoop")
    vp.for_loop(_Model, "cpu", 16, "EvalLoop")
    with pytest.raises(ValueError, match="batch_size 65536"):
        vp.for_loop(_Model, "cpu", 65536, "PredictLoop")
    with pytest.raises(ValueError, match=r"POIs 1 .. 400, the model scores 399 columns"):
        vp.for_loop(types.SimpleNamespace(label_offset=1, out_proj=torch.nn.Linear(2, 399)), "cpu", 16, "EvalLoop")
    s, h, u = torch.zeros(2, 400), torch.zeros(2, 3, dtype=torch.int64), torch.ones(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="VisitPrior.blend: scores must be f32"):
        vp.blend(s.double(), (h, u), 1)
    with pytest.raises(TypeError, match="VisitPrior.blend: user must be int32 or int64 ids"):
        vp.blend(s, (h, u.float()), 1)
    with pytest.raises(ValueError, match="2 rows of scores, 2 of hist and 3 users"):
        vp.blend(s, (h, torch.ones(3, dtype=torch.int64)), 1)
    with pytest.raises(ValueError, match=r"weights must be a contiguous f32 \[2\]"):
        vp.blend(s, (h, u), 1, weights=torch.zeros(3))
    vp.status |= visitprior.SBADINDEX
    with pytest.raises(ValueError, match=rf"EvalLoop: the kernel skipped table rows or entries \(status {visitprior.SBADINDEX}\)"):
        vp.check("EvalLoop")
    vp.reset_status()
    vp.check()


def test_the_header_is_readable_without_the_built_library():
    sig = _visitprior.SIGNATURES
    assert list(sig) == ["mobgt_visitprior_abi_version", "mobgt_visitprior_keys", "mobgt_visitprior_fill", "mobgt_visitprior_blend_rows"]
    assert _visitprior.ABI_VERSION == 1 and [len(sig[k][1]) for k in list(sig)[1:]] == [15, 14, 25]
    c = _visitprior
    assert (c.EBADDIM, c.EALIGN, c.EDTYPE, c.SBADINDEX, c.SBADVALUE, c.I32, c.I64) == (-1, -2, -3, 1, 2, 0, 1)
    assert c.CHUNK % 4 == 0 and c.THREADS % 64 == 0 and c.MAX_G == 65535 and c.KEY_BITS == 62 and vc.LOG_P == 2 * c.CHUNK + 3
    assert vc.THREADS == c.THREADS
    from mobgt_amd import _ctxprior, _native, _prior
    assert not set(sig) & (set(_ctxprior.SIGNATURES) | set(_prior.SIGNATURES))
    assert "_visitprior" not in _native._MODULES and len(_native._MODULES) == 5
    assert c.LIBRARY.extra_inputs == _prior.LIBRARY.extra_inputs and c.LIBRARY.extra_inputs[0].endswith("blend_rows.h")


# ------------------------------------------------------------------------------------------------ the rule does something
def _zero_score_mrr(seed):
    """-> {(popularity, visits, recency): MRR} of all-zero scores over the held-out prefixes of favourites_log(seed), through the
    package's host path: MarkovBaseline.fit and VisitPrior.fit on the CPU, the priors' f32 CPU blends."""
    sessions, mask = vc.favourites_log(seed=seed)
    ds = data.SessionDataset(sessions)
    pop = baseline.MarkovBaseline.fit(ds, mask, P=400, device="cpu").prior(user=0.0, transition=0.0, popularity=1.0)
    vp = data.VisitPrior.fit(ds, mask, P=400, device="cpu")
    hist, user, y = vc.held_out_prefixes(sessions, mask)
    pair = (torch.from_numpy(hist), torch.from_numpy(user))
    base = pop.blend(torch.zeros(len(y), 400), pair, 1)
    out = {(1, 0, 0): vc.mrr(base.numpy(), y)}
    for wv, wr in ((3, 0), (0, 3), (3, 3)):
        out[(1, wv, wr)] = vc.mrr(vp.blend(base.clone(), pair, 1, weights=torch.tensor([wv, wr], dtype=torch.float32)).numpy(), y)
    return out, len(y)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_visits_and_recency_each_add_to_popularity(seed):
    """favourites_log(seed): 30 users, 400 POIs, 40 sessions of 3 .. 9 check-ins a user, 60 % of a user's check-ins from 8 slowly
    drifting favourites and the rest by popularity; the last 30 % of every user's sessions are held out, every prefix of them a
    sample, all model scores zero, ties lower POI first.  The MRR by (popularity, visits, recency) weights, as the f32 host form
    gives it, is printed -- seeds 0 / 1 / 2: (1, 0, 0) 0.0497 / 0.0440 / 0.0461, (1, 3, 0) 0.1606 / 0.1552 / 0.1393, (1, 0, 3)
    0.1202 / 0.1543 / 0.1378, (1, 3, 3) 0.1850 / 0.1859 / 0.1891 over 1 773 / 1 806 / 1 794 prefixes; asserted are the orderings only."""
    m, n = _zero_score_mrr(seed)
    print(f"seed {seed}: {n} held-out prefixes; MRR " + ", ".join(f"{k}: {v:.4f}" for k, v in m.items()))
    assert m[(1, 0, 0)] < m[(1, 3, 0)] < m[(1, 3, 3)]
    assert m[(1, 0, 3)] < m[(1, 3, 3)]


def test_the_weights_fitted_by_maximum_likelihood_beat_popularity_alone(log):
    """priorfit.fit_host on the held-out prefixes of favourites_log(seed=0), K = 3 features (popularity, visits, recency), from
    w = 0, l2 = 1e-3: it converges in 5 passes to about (0.26, 0.74, 0.43); the mean negative log-likelihood is 5.9915 (= log 400)
    at w = 0, 5.7722 at weights (1, 0, 0) and 5.0963 at the fitted ones."""
    sessions, mask, ds, mb, vp = log
    hist, user, y = vc.held_out_prefixes(sessions, mask)
    pair = (torch.from_numpy(hist), torch.from_numpy(user))
    n = len(y)
    feats = torch.zeros(3, n, 400)
    feats[0] = mb.prior().features(pair, 1, torch.zeros(3, n, 400))[2]
    vp.features(pair, 1, feats[1:])
    res = priorfit.fit_host(None, feats.numpy(), y, target_offset=-1, names=("popularity", "visits", "recency"), start=[0.0, 0.0, 0.0])
    terms, status = priorfit.terms_host(None, feats.numpy(), y, -1, [[1.0, 0.0, 0.0]])
    nll_pop = float(terms[0, :, 1].sum() / terms[0, :, 0].sum())
    print(f"fit: {res.weights}, passes {res.passes}, nll {res.nll_start:.4f} -> {res.nll:.4f}; popularity alone {nll_pop:.4f}")
    assert status == 0 and res.converged and res.n == n and res.nll_start == pytest.approx(np.log(400.0))
    assert res.nll < nll_pop < res.nll_start and all(res.weights[k] > 0.0 for k in ("visits", "recency"))
