"""The distance prior's rule on the host (mobgt_amd.geoprior: pair_hist_host, csr_hist_host, table_from_counts and blend_host, the
references of the kernels in csrc_geoprior/geoprior.hip; a DistancePrior fitted on the CPU; prior.Stack): the histograms against a
brute-force double loop, the table against its formula, the blend's untouched elements bit for bit, the stack against its
members applied in turn, every refusal, the header, and that the fitted rule ranks held-out transitions better than
popularity does."""
import numpy as np
import pytest
import torch

import geoprior_cases as gc
import prior_cases as pc
from mobgt_amd import _geoprior, baseline, data, geo, geoprior, prior

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dataset(sessions):
    return data.SessionDataset([(u, pc.as_checkins(p)) for u, p in sessions])


# ------------------------------------------------------------------------------------------------ the histograms
@pytest.mark.parametrize("P", (1, 2, 7))
def test_the_histograms_are_the_brute_force_counts(P):
    u = gc.unit(P, seed=P)
    thr = gc.thresholds(u, 9, seed=P)
    thr[5] = thr[4]                                                     # a repeated threshold: bin 5 is empty
    assert thr[0] == 0.0 and np.all(np.diff(thr) >= 0)
    b = gc.brute_bins(u, thr)
    n = geoprior.pair_hist_host(u, thr)
    assert n.dtype == np.int64 and n.shape == (10,) and n.tolist() == np.bincount(b.reshape(-1), minlength=10).tolist()
    assert int(n.sum()) == P * P and n[5] == 0 and n[0] == 0           # thresholds[0] = 0: every pair, duplicates included, is in a bin >= 1
    assert b.max() == 9                                                 # the farthest pair's c2 IS the last threshold: bin nthr
    if P >= 2:
        assert b[0, 1] >= 1 and np.array_equal(u[0], u[1])             # an exact duplicate
    rowptr, col, val = gc.csr(P, seed=P, full_row=P - 1)
    want = np.zeros(10, dtype=np.int64)
    for a in range(P):
        for e in range(rowptr[a], rowptr[a + 1]):
            want[b[a, col[e]]] += val[e]
    status = [0]
    t = geoprior.csr_hist_host(u, thr, rowptr, col, val, status=status)
    assert t.dtype == np.int64 and t.tolist() == want.tolist() and int(t.sum()) == int(val.sum()) and status == [0]
    assert (col[rowptr[P - 1]:rowptr[P]] == P - 1).any()               # a self-transition counted


def test_csr_hist_host_skips_and_flags_what_fit_did_not_make():
    P = 7
    u = gc.unit(P)
    thr = gc.thresholds(u, 6)
    rowptr, col, val = gc.csr(P, full_row=2)
    good = geoprior.csr_hist_host(u, thr, rowptr, col, val)
    b = gc.brute_bins(u, thr)

    def row_sum(a):
        out = np.zeros(7, dtype=np.int64)
        np.add.at(out, b[a, col[rowptr[a]:rowptr[a + 1]]], val[rowptr[a]:rowptr[a + 1]])
        return out
    down = rowptr.copy()
    down[3] = rowptr[2] - 1                                             # rows 2 and 3: row 2 descends; row 3 then starts early but is valid
    status = [0]
    got = geoprior.csr_hist_host(u, thr, down, col, val, status=status)
    assert status == [geoprior.SBADINDEX] and int(got.sum()) < int(good.sum())
    beyond = rowptr.copy()
    beyond[P] = len(col) + 3
    status = [0]
    got = geoprior.csr_hist_host(u, thr, beyond, col, val, status=status)
    assert status == [geoprior.SBADINDEX] and got.tolist() == (good - row_sum(P - 1)).tolist()
    bad = col.copy()
    e = int(rowptr[2])
    bad[e] = P
    status = [0]
    got = geoprior.csr_hist_host(u, thr, rowptr, bad, val, status=status)
    one = np.zeros(7, dtype=np.int64)
    one[b[2, col[e]]] = val[e]
    assert status == [geoprior.SBADINDEX] and got.tolist() == (good - one).tolist()


def test_table_from_counts_is_the_formula():
    n = np.array([0, 5, 100, 10 ** 12, 3], dtype=np.int64)
    t = np.array([7, 0, 2 ** 33, 1, 0], dtype=np.int64)
    B, N, T = 5, int(n.sum()), int(t.sum())
    want = [np.float32(np.log((float(t[b]) + 1) / (T + B)) - np.log((float(n[b]) + 1) / (N + B))) for b in range(B)]
    got = geoprior.table_from_counts(n, t)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(np.array(want)))
    zero = geoprior.table_from_counts(n, np.zeros(5, dtype=np.int64))   # no transition at all
    assert zero.dtype == np.float32 and np.isfinite(zero).all() and np.isfinite(got).all()
    assert np.array_equal(bits(zero), bits(np.float32(np.log(1.0 / 5) - np.log((n + 1.0) / (N + 5)))))
    with pytest.raises(ValueError, match="two integer histograms"):
        geoprior.table_from_counts(n, t[:4])
    with pytest.raises(ValueError, match="two integer histograms"):
        geoprior.table_from_counts(n.astype(np.float64), t)
    with pytest.raises(ValueError, match="negative"):
        geoprior.table_from_counts(n, -t)


# ------------------------------------------------------------------------------------------------ the blend
def _tables(P, nthr=11, seed=0):
    u = gc.unit(P, seed)
    thr = gc.thresholds(u, nthr, seed)
    table = (np.random.RandomState(seed).standard_normal(nthr + 1) * 3).astype(F)
    return geoprior.DistanceTables(u, thr, table, P)


@pytest.mark.parametrize("label_offset", (0, 1))
@pytest.mark.parametrize("V", (5, 10, 13))                             # P = 9: V < P, V = P + 1, V > P + 1
def test_blend_host_touches_exactly_what_the_rule_names(V, label_offset):
    P = 9
    t = _tables(P)
    hist = np.array([[3, 0, 5, 0], [0, 0, 0, 0], [4, 0, 0, 0], [2, -1, 0, 0], [2, P + 1, 0, 0], [0, 7, 0, 0], [P, 0, 0, 0], [1, 2, 3, 2 ** 40]])
    anchor = [5, None, 4, None, None, 7, P, None]
    scores = pc.scores(len(hist), V, seed=V)
    special = np.array([0x7F800000, 0xFF800000, 0x80000000, 0x7FC00001, 0xFFC12345], dtype=np.uint32)
    for g in (1, 2, 4):                                                 # +-inf, -0.0 and two NaN payloads in rows with and without an anchor
        scores[g, :5] = special.view(F)
    got = geoprior.blend_host(scores, hist, t, 0.75, label_offset)
    assert got.dtype == F and got.shape == scores.shape
    b = gc.brute_bins(t.unit, t.thresholds)
    w = F(0.75)
    for g, a in enumerate(anchor):
        for c in range(V):
            p = c + label_offset
            if a is None or not 1 <= p <= P:
                assert bits(got[g, c]) == bits(scores[g, c]), (g, c)   # copied bit for bit: -0.0, -inf and NaN payloads
            else:
                assert bits(got[g, c]) == bits(F(scores[g, c] + F(w * t.table[b[a - 1, p - 1]]))), (g, c)
    assert np.array_equal(bits(got[1, :5]), special) and np.array_equal(bits(got[4, :5]), special)
    # with weight 0 the term is still added: x + 0 * table turns -0.0 into +0.0 where the table entry is not negative (0 * a
    # negative entry is -0.0, and -0.0 + -0.0 stays), and changes nothing else
    zero = geoprior.blend_host(scores, hist, t, 0.0, label_offset)
    assert ((zero == scores) | (np.isnan(zero) & np.isnan(scores))).all()
    flipped = bits(zero) != bits(scores)
    rows = [g for g, a in enumerate(anchor) if a is not None]
    lo, hi = max(0, 1 - label_offset), min(V, P + 1 - label_offset)
    assert (bits(scores[rows, lo:hi]) == 0x80000000).any() and flipped.any()
    assert ((bits(scores)[flipped] == 0x80000000) & (bits(zero)[flipped] == 0)).all() and not flipped[[1, 3, 4, 7]].any()
    for g in rows:
        pos = b[anchor[g] - 1, lo + label_offset - 1:hi + label_offset - 1]
        assert np.array_equal(bits(zero[g, lo:hi]), bits(scores[g, lo:hi] + (F(0.0) * t.table[pos])))


# ------------------------------------------------------------------------------------------------ a CPU prior, the stack
@pytest.fixture(scope="module")
def walks():
    sessions = pc.walks()
    ds = dataset(sessions)
    train = np.arange(len(ds)) % 4 != 3
    mb = baseline.MarkovBaseline.fit(ds, train, P=30, device="cpu")
    pb = geo.pair_bins(gc.city(30, seed=2), edges=np.arange(0.0, 30.0, 2.5), device="cpu")
    return sessions, train, mb, pb


def test_a_prior_fitted_on_the_cpu(walks):
    _, _, mb, pb = walks
    dp = mb.distance_prior(pb, distance=0.5)
    assert isinstance(dp, geoprior.DistancePrior) and data.DistancePrior is geoprior.DistancePrior and dp.pair_bins is pb
    u, thr = pb.unit.numpy(), pb.thresholds.numpy()
    g = mb.graph
    assert dp.pair_counts.tolist() == geoprior.pair_hist_host(u, thr).tolist() and int(dp.pair_counts.sum()) == 900
    assert dp.transition_counts.tolist() == geoprior.csr_hist_host(u, thr, g.rowptr.numpy(), g.col.numpy(), g.val.numpy()).tolist()
    assert int(dp.transition_counts.sum()) == int(g.val.sum())
    want = geoprior.table_from_counts(dp.pair_counts, dp.transition_counts)
    assert dp.table.dtype == torch.float32 and np.array_equal(bits(dp.table.numpy()), bits(want)) and dp.status.tolist() == [0]
    assert dp.weights.tolist() == [0.5] and dp.get_weights() == {"distance": 0.5} and dp.n_weights == 1 and dp.WEIGHTS == ("distance",)
    assert dp.set_weights(distance=2.0).weights.tolist() == [2.0] and dp.set_weights().get_weights() == {"distance": 2.0}
    edges, n, t, table = dp.curve()
    assert len(edges) == len(n) == len(t) == len(table) == thr.size + 1 and edges[0] == 0.0 and np.isinf(edges[-1])
    np.testing.assert_allclose(edges[1:-1], np.arange(2.5, 30.0, 2.5), rtol=1e-9)
    # the public call of a CPU prior is the host form, in place by default and into `out` otherwise
    hist = torch.from_numpy(gc.hist_rows(6, 30, dtype=np.int64))
    scores = pc.scores(6, 31)
    want = geoprior.blend_host(scores, hist.numpy(), dp.tables(), 2.0, 1)
    s = torch.from_numpy(scores.copy())
    assert dp.blend(s, (hist, torch.ones(6, dtype=torch.int64)), 1) is s and np.array_equal(bits(s.numpy()), bits(want))
    out = torch.full((6, 33), 9.0)
    dp.blend(torch.from_numpy(scores.copy()), hist.int(), 1, out=out, weights=torch.tensor([2.0]))
    assert np.array_equal(bits(out[:, :31].numpy()), bits(want)) and bool((out[:, 31:] == 9.0).all())
    assert (bits(want) != bits(scores)).any()


class _Model:
    label_offset = 1
    out_proj = torch.nn.Linear(2, 30)


def test_what_the_distance_prior_refuses(walks):
    sessions, train, mb, pb = walks
    with pytest.raises(ValueError, match="fitted on 30 POIs, the bins hold 29"):
        mb.distance_prior(geo.pair_bins(gc.city(29), edges=[0.0, 1.0, 2.0], device="cpu"))
    with pytest.raises(ValueError, match="the baseline is on cpu, the bins on meta"):
        mb.distance_prior(geo.PairBins(30, pb.unit.to("meta"), pb.thresholds.to("meta"), pb.num_bins))
    with pytest.raises(TypeError, match="must be a geo.PairBins"):
        geoprior.DistancePrior.fit(mb, None)
    with pytest.raises(ValueError, match="thresholds"):
        mb.distance_prior(geo.PairBins(30, pb.unit, pb.thresholds[:1], 0))
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match=r"the weights \(distance\) must be finite"):
            mb.distance_prior(pb, distance=bad)
    dp = mb.distance_prior(pb)
    with pytest.raises(ValueError, match="must be finite"):
        dp.set_weights(distance=float("nan"))
    assert dp.weights.tolist() == [1.0]
    with pytest.raises(ValueError, match="EvalLoop: the prior is on cpu, the loop on cuda:0"):
        dp.for_loop(_Model, "cuda:0", 16, "EvalLoop")
    dp.for_loop(_Model, "cpu", 16, "EvalLoop")
    with pytest.raises(ValueError, match="batch_size 65536"):
        dp.for_loop(_Model, "cpu", 65536, "PredictLoop")
    s, h = torch.zeros(2, 30), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="scores must be f32"):
        dp.blend(s.double(), h, 1)
    with pytest.raises(ValueError, match="out must be f32"):
        dp.blend(s, h, 1, out=torch.zeros(2, 29))
    with pytest.raises(ValueError, match="label_offset must be 0 or 1"):
        dp.blend(s, h, 2)
    with pytest.raises(TypeError, match="hist must be int32 or int64"):
        dp.blend(s, h.float(), 1)
    with pytest.raises(ValueError, match="2 rows of scores, 3 of hist"):
        dp.blend(s, (torch.zeros(3, 3, dtype=torch.int64), torch.ones(3, dtype=torch.int64)), 1)
    with pytest.raises(ValueError, match=r"weights must be a contiguous f32 \[1\]"):
        dp.blend(s, h, 1, weights=torch.zeros(3))
    # a CSR that fit did not make is refused through check
    broken = baseline.MarkovBaseline.fit(dataset(sessions), train, P=30, device="cpu")
    broken.graph.col[0] = 30
    with pytest.raises(ValueError, match=rf"DistancePrior.fit: .*\(status {geoprior.SBADINDEX}\)"):
        broken.distance_prior(pb)


def test_the_stack(walks):
    _, _, mb, pb = walks
    mp, dp = mb.prior(0.75, 1.5, 0.3), mb.distance_prior(pb, 0.6)
    st = prior.Stack(mp, dp)
    assert st.WEIGHTS == ("user", "transition", "popularity", "distance") and st.n_weights == 4 and st.priors == (mp, dp)
    assert mp.n_weights == 3 and mp.WEIGHTS == prior.WEIGHTS and prior.Stack(dp, mp).WEIGHTS == ("distance", "user", "transition", "popularity")
    assert st.get_weights() == pytest.approx(dict(user=0.75, transition=1.5, popularity=0.3, distance=0.6)) and list(st.get_weights()) == list(st.WEIGHTS)
    hist = torch.from_numpy(gc.hist_rows(8, 30, dtype=np.int64))
    user = torch.arange(1, 9)
    scores = pc.scores(8, 31, seed=1)

    def in_turn(order, w_markov, w_dist):
        s = scores
        for which in order:
            if which == "m":
                s = prior.blend_host(s, hist.numpy(), user.numpy(), mp.tables(), w_markov, 1)
            else:
                s = geoprior.blend_host(s, hist.numpy(), dp.tables(), w_dist, 1)
        return s
    got = st.blend(torch.from_numpy(scores.copy()), (hist, user), 1)
    assert np.array_equal(bits(got.numpy()), bits(in_turn("md", (0.75, 1.5, 0.3), F(0.6))))
    out = torch.full((8, 34), 9.0)
    res = prior.Stack(dp, mp).blend(torch.from_numpy(scores.copy()), (hist, user), 1, out=out)
    assert res is out and np.array_equal(bits(out[:, :31].numpy()), bits(in_turn("dm", (0.75, 1.5, 0.3), F(0.6)))) and bool((out[:, 31:] == 9.0).all())
    assert not np.array_equal(bits(out[:, :31].numpy()), bits(got.numpy()))          # f32 sums: the order of the members counts
    # a weights view is split per member, in order
    W = torch.tensor([[9.0, 9.0, 9.0, 9.0], [0.5, 0.25, 2.0, -1.5]])
    got = st.blend(torch.from_numpy(scores.copy()), (hist, user), 1, weights=W[1])
    assert np.array_equal(bits(got.numpy()), bits(in_turn("md", (0.5, 0.25, 2.0), -1.5)))
    for bad in (torch.zeros(3), torch.zeros(5), torch.zeros(4, dtype=torch.float64), torch.zeros(4, 2)[:, 0], [0.0] * 4):
        with pytest.raises(ValueError, match=r"weights must be a contiguous f32 \[4\] view"):
            st.blend(torch.from_numpy(scores.copy()), (hist, user), 1, weights=bad)
    # a stack of one is its member
    one = prior.Stack(mp).blend(torch.from_numpy(scores.copy()), (hist, user), 1)
    assert np.array_equal(bits(one.numpy()), bits(mp.blend(torch.from_numpy(scores.copy()), (hist, user), 1).numpy()))
    assert prior.Stack(mp).WEIGHTS == prior.WEIGHTS and prior.Stack(mp).n_weights == 3
    one = prior.Stack(dp).blend(torch.from_numpy(scores.copy()), (hist, user), 1)
    assert np.array_equal(bits(one.numpy()), bits(dp.blend(torch.from_numpy(scores.copy()), (hist, user), 1).numpy()))
    # weights by name; nothing changes on a refusal
    st.set_weights(distance=2.0, user=0.0)
    assert mp.weights.tolist() == [0.0, 1.5, pytest.approx(0.3)] and dp.weights.tolist() == [2.0]
    for kw in (dict(distance=float("inf")), dict(user=1.0, distance=float("nan")), dict(speed=1.0)):
        with pytest.raises(ValueError):
            st.set_weights(**kw)
    assert st.get_weights() == pytest.approx(dict(user=0.0, transition=1.5, popularity=0.3, distance=2.0))
    # status and checks reach every member
    mp.status |= 1
    with pytest.raises(ValueError, match=r"EvalLoop: .*\(status 1\)"):
        st.check("EvalLoop")
    st.reset_status()
    st.check()
    assert mp.status.tolist() == [0] and dp.status.tolist() == [0]
    st.for_loop(_Model, "cpu", 16, "EvalLoop")
    with pytest.raises(ValueError, match="the prior is on cpu, the loop on cuda:0"):
        st.for_loop(_Model, "cuda:0", 16, "EvalLoop")
    with pytest.raises(ValueError, match="at least one prior"):
        prior.Stack()
    with pytest.raises(ValueError, match="user, transition, popularity belong to more than one member"):
        prior.Stack(mp, mb.prior())
    with pytest.raises(TypeError, match="is no prior"):
        prior.Stack(mp, object())
    with pytest.raises(ValueError, match=r"grid must be \[L >= 1, 4\]"):
        st.tune(None, None, None, np.ones((2, 3)))
    assert prior.sweep_weights(np.ones((2, 4)), names=st.WEIGHTS).shape == (2, 4)
    with pytest.raises(ValueError, match=r"\[L, 4\] rows of \(user, transition, popularity, distance\) weights, got shape"):
        prior.sweep_weights(np.ones((2, 3)), names=st.WEIGHTS)


def test_the_header_is_readable_without_the_built_library():
    sig = _geoprior.SIGNATURES
    assert list(sig) == ["mobgt_geoprior_abi_version", "mobgt_geoprior_pair_hist", "mobgt_geoprior_csr_hist", "mobgt_geoprior_blend_rows"]
    assert _geoprior.ABI_VERSION == 1 and [len(sig[k][1]) for k in list(sig)[1:]] == [6, 11, 18]
    assert (_geoprior.EBADDIM, _geoprior.EALIGN, _geoprior.EDTYPE, _geoprior.SBADINDEX, _geoprior.I32, _geoprior.I64) == (-1, -2, -3, 1, 0, 1)
    assert _geoprior.CHUNK % _geoprior.THREADS == 0 and _geoprior.TILE % 64 == 0 and _geoprior.MAX_G == 65535
    from mobgt_amd import _lib_bins, _native, _prior
    assert 2049 + 1 <= _geoprior.LDS_BINS < _lib_bins.MAX_THRESHOLDS + 1                 # nthr = 2049 counts in LDS, 32767 in global memory
    assert 8 * (2048 + 3 * _geoprior.TILE) + 4 * _geoprior.LDS_BINS <= 160 * 1024
    assert not set(sig) & set(_prior.SIGNATURES) and "_geoprior" not in _native._MODULES and len(_native._MODULES) == 5


# ------------------------------------------------------------------------------------------------ the rule does something
def _mrr(blended, targets):
    """baseline's tie rule: score descending, equal scores lower POI first"""
    rr = []
    for s, y in zip(blended, targets):
        order = np.lexsort((np.arange(s.size), -s.astype(np.float64)))
        rr.append(1.0 / (int(np.nonzero(order == y - 1)[0][0]) + 1))
    return float(np.mean(rr))


def test_the_fitted_distance_term_ranks_better_than_popularity():
    """400 POIs uniform in a 20 km box, the next POI drawn ~ popularity * exp(-d / 1.5 km), 3 000 train and 500 held-out
    transitions, edges every 0.5 km, all model scores zero, everything through the package's host path (SessionDataset,
    MarkovBaseline.fit, geo.pair_bins, DistancePrior.fit, the priors' CPU blends).  Measured MRR over the 500 held-out
    transitions: popularity alone 0.1407, the distance term alone 0.4248, both with weights 1 0.6146."""
    coords, sessions, train = gc.decay_log()
    ds = dataset(sessions)
    P = len(coords)
    mb = baseline.MarkovBaseline.fit(ds, train, P=P, device="cpu")
    assert int(mb.graph.val.sum()) == 3000
    pb = geo.pair_bins(coords, edges=np.arange(0.0, 30.0, 0.5), device="cpu")
    pop, dist = mb.prior(user=0.0, transition=0.0, popularity=1.0), mb.distance_prior(pb)
    held = [p for (_, p), tr in zip(sessions, train) if not tr]
    hist = torch.tensor([[a] for p in held for a in p[:-1]], dtype=torch.int64)
    y = [b for p in held for b in p[1:]]
    assert len(y) == 500
    rows = (hist, torch.ones(len(y), dtype=torch.int64))
    zeros = lambda: torch.zeros(len(y), P)
    mrr_pop = _mrr(pop.blend(zeros(), rows, 1).numpy(), y)
    mrr_dist = _mrr(dist.blend(zeros(), rows, 1).numpy(), y)
    mrr_both = _mrr(prior.Stack(pop, dist).blend(zeros(), rows, 1).numpy(), y)
    print(f"MRR: popularity {mrr_pop:.4f}, distance {mrr_dist:.4f}, both {mrr_both:.4f}")
    assert mrr_dist > mrr_pop and mrr_both > mrr_dist
