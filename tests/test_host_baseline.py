"""The Markov baseline's rule on the host (mobgt_amd.baseline: ranks_host / topk_host, the reference of the kernels in
csrc_baseline/baseline.hip, and MarkovBaseline fitted on the CPU): ranks written out by hand on a miniature, every TypeError /
ValueError of fit and ranks, the two host forms against each other, `evaluate` against metrics.restricted_sums on dense scores
that hold the same order, and the CPU-fitted tables against universe_counts_host and brute-force counters."""
import numpy as np
import pytest
import torch

import baseline_cases as bc
from mobgt_amd import _baseline, baseline, data, metrics


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("key", sorted(bc.MINI_LISTS))
def test_ranks_of_the_miniature_written_out(key):
    user, prev, order = key
    want = bc.MINI_LISTS[key]                                          # every POI, best first: t's rank is its position
    ds = bc.dataset(bc.MINI_TRAIN + bc.mini_samples(user, prev))
    train = np.arange(len(ds)) < len(bc.MINI_TRAIN)
    samples = bc.dataset(bc.mini_samples(user, prev))                  # targets 1 .. 6 in turn
    rank, revisit = baseline.ranks_host(ds, train, samples, order)
    assert rank.dtype == np.int32 and revisit.dtype == np.uint8
    assert rank.tolist() == [want.index(t) for t in range(1, bc.MINI_P + 1)]
    assert revisit.tolist() == [int(t == prev) for t in range(1, bc.MINI_P + 1)]
    for k in (1, 4, 6, 9):
        ids = baseline.topk_host(ds, train, samples, order, k)
        assert ids.dtype == np.int32 and ids.shape == (6, k)
        assert all(row.tolist() == (want + [-1] * 3)[:k] for row in ids)


def test_a_prefix_dataset_and_the_truncated_sessions_are_the_same_samples():
    c = bc.case("walks")
    rank, revisit = bc.host("walks", "user")
    pds = c.samples
    cut_sessions = bc.dataset([(int(pds.users[i]), pds[i].checkins[:, 0]) for i in range(len(pds))])
    again = baseline.ranks_host(c.ds, c.train, cut_sessions, "user", P=int(c.ds.seq[:, 0].max()))
    assert np.array_equal(rank, again[0]) and np.array_equal(revisit, again[1]) and 0 < revisit.sum() < len(revisit)


def test_the_crafted_cases_hold_what_their_docstrings_say():
    c = bc.case("rows")
    mb = baseline.MarkovBaseline.fit(c.ds, c.train, device="cpu")
    assert np.diff(mb.graph.rowptr.numpy())[:len(bc.ROW_LENGTHS)].tolist() == list(bc.ROW_LENGTHS)
    P = mb.P
    assert int(mb.ukey[0]) == int(mb.graph.col[0]) and int(mb.ukey[0]) < P             # user 0, POI 1: the table's first range
    assert int(mb.ukey[-1]) == (4 * P + bc.ROWS_P - 1) * P + 11 and bc.ROWS_P == P      # user 4, POI P -> 12: its last
    assert 9 in c.samples.users and 9 not in c.ds.users[c.train]
    _, a, t = bc.previous_and_target(c.samples)
    rowptr, col = mb.graph.rowptr.numpy(), mb.graph.col.numpy()
    first = sum(int(rowptr[x] > rowptr[x - 1] and col[rowptr[x - 1]] == y - 1) for x, y in zip(a, t))
    last = sum(int(rowptr[x] > rowptr[x - 1] and col[rowptr[x] - 1] == y - 1) for x, y in zip(a, t))
    absent = sum(int(rowptr[x] > rowptr[x - 1] and y - 1 not in col[rowptr[x - 1]:rowptr[x]]) for x, y in zip(a, t))
    assert first >= 9 and last >= 9 and absent >= 9 and int((rowptr[a] == rowptr[a - 1]).sum()) >= 9
    f = bc.case("fill")
    fb = baseline.MarkovBaseline.fit(f.ds, f.train, device="cpu")
    row = fb.graph.col[fb.graph.rowptr[39]:fb.graph.rowptr[40]].numpy()
    assert len(row) == 63 and set(row.tolist()) == set(fb.pop_order[:63].tolist()) and int(fb.pop_order[63]) == 63
    assert bc.host_lists("fill", "user", 64)[2].tolist()[-1] == 64 and int(bc.host("fill", "user")[0][5]) == 63
    assert len(bc.case("q41").samples) % _baseline.SAMPLES_PER_BLOCK == 1 and len(bc.case("empty").samples) == 0
    h = bc.case("history")
    assert sorted(set((np.diff(h.samples.offsets) - 1).tolist())) == [1, 64, 65, 4096]
    assert bc.host("history", "user")[1].tolist() == [0, 0, 1, 0, 1, 1, 0, 1, 1]


# ------------------------------------------------------------------------------------------------ validation
def test_what_fit_refuses():
    c = bc.case("mini")
    fit = lambda ds=c.ds, train=c.train, **kw: baseline.MarkovBaseline.fit(ds, train, device="cpu", **kw)
    with pytest.raises(TypeError, match=r"pds\.base"):
        fit(ds=data.PrefixDataset(c.ds, device="cpu"))
    with pytest.raises(TypeError, match="must be a data.SessionDataset, got list"):
        fit(ds=[(0, [[1, 0, 1], [2, 0, 1]])])
    with pytest.raises(ValueError, match=rf"train: a mask of 3 flags for {len(c.ds)} sessions"):
        fit(train=np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="train: a boolean mask of length .* or integer session indices, got float64"):
        fit(train=np.array([0.5]))
    with pytest.raises(ValueError, match=rf"train: session index {len(c.ds)} is not in 0 \.\. {len(c.ds) - 1}"):
        fit(train=np.array([0, len(c.ds)]))
    with pytest.raises(TypeError, match="P must be an integer, got float"):
        fit(P=6.0)
    with pytest.raises(ValueError, match="POI count 0, at least 1 is needed"):
        fit(P=0)
    with pytest.raises(ValueError, match=r"session 13: POI id 6 at check-in 1 is not in 1 \.\. 5 "):
        fit(P=5)
    zero = bc.dataset([(0, [1, 2]), (0, [2, 0, 1])])
    with pytest.raises(ValueError, match=r"session 1: POI id 0 at check-in 1 is not in 1 \.\. 2 "):
        fit(ds=zero, train=[0])
    with pytest.raises(ValueError, match="session 1: user -2 is negative"):
        fit(ds=bc.dataset([(0, [1, 2]), (-2, [2, 1])]), train=[0])
    with pytest.raises(ValueError, match=r"U \* P \* P < 2\*\*63"):
        fit(ds=bc.dataset([(0, [1, 2]), (2 ** 40, [2, 1])]), train=[0], P=4096)
    assert fit(ds=bc.dataset([(0, [1, 2]), (2 ** 38, [2, 1])]), train=[0], P=4096).U == 2 ** 38 + 1     # (2**62 and a bit: it fits)
    assert fit(P=9).P == 9 and fit(train=np.array([2, 0])).graph.nnz == 2


def test_what_ranks_and_recommend_refuse():
    c = bc.case("mini")
    mb = baseline.MarkovBaseline.fit(c.ds, c.train, device="cpu")
    for call in (mb.ranks, mb.evaluate, mb.recommend, lambda s, order: baseline.ranks_host(c.ds, c.train, s, order)):
        with pytest.raises(ValueError, match="order must be one of 'user', 'global', 'popularity', got 'markov'"):
            call(c.samples, order="markov")
        with pytest.raises(TypeError, match="must be a data.PrefixDataset or a data.SessionDataset, got list"):
            call([(0, [1, 2])], order="user")
        with pytest.raises(ValueError, match=r"session 1 of the samples: POI id 7 at check-in 0 is not in 1 \.\. 6"):
            call(bc.dataset([(0, [1, 2]), (0, [7, 1])]), order="user")
    for k in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="k must be an integer in 1 .. 64"):
            mb.recommend(c.samples, k=k)
        with pytest.raises(ValueError, match="k must be an integer in 1 .. 64"):
            baseline.topk_host(c.ds, c.train, c.samples, k=k)
    rank, revisit = mb.ranks(bc.dataset([(99, [1, 2])]))              # a user nobody has seen backs off: (0, 1, "global")
    assert rank.tolist() == [1] and revisit.tolist() == [0] and rank.dtype == torch.int32 and revisit.dtype == torch.uint8


def test_the_header_is_readable_without_the_built_library():
    sig = _baseline.SIGNATURES
    assert list(sig) == ["mobgt_baseline_abi_version", "mobgt_baseline_ranks", "mobgt_baseline_topk"] and _baseline.ABI_VERSION == 1
    assert len(sig["mobgt_baseline_ranks"][1]) == 23 and len(sig["mobgt_baseline_topk"][1]) == 24
    assert (_baseline.EBADDIM, _baseline.EALIGN, _baseline.SBADINDEX, _baseline.STOOLONG) == (-1, -2, 1, 2)
    assert (_baseline.MAX_L, _baseline.WAVE, _baseline.MAX_K) == (baseline.DEVICE_MAX_L, 64, baseline.MAX_K) == (4096, 64, 64)
    assert (_baseline.ORDER_USER, _baseline.ORDER_GLOBAL, _baseline.ORDER_POPULARITY) == tuple(baseline.ORDERS[o] for o in bc.ORDERS)
    from mobgt_amd import _native, _prefixes
    assert _baseline.MAX_L == _prefixes.MAX_L and len(_native._MODULES) == 5 and "_baseline" not in _native._MODULES
    assert data.MarkovBaseline is baseline.MarkovBaseline


# ------------------------------------------------------------------------------------------------ the two host forms
@pytest.mark.parametrize("order", bc.ORDERS)
@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_the_list_holds_the_target_at_its_rank(name, order):
    c = bc.case(name)
    rank, _ = bc.host(name, order)
    _, _, t = bc.previous_and_target(c.samples)
    P = baseline._prepare(c.ds, c.train, None, "test")[4]
    assert rank.shape == t.shape and np.all((rank >= 0) & (rank < P))
    for k in bc.KS:
        ids = bc.host_lists(name, order, k)
        assert ids.shape == (len(t), k)
        inside = rank < k
        assert np.array_equal(ids[inside, rank[inside]], t[inside]) and not (ids[~inside] == t[~inside, None]).any()
        assert np.all(ids[:, :min(k, P)] >= 1) and np.all(ids[:, min(k, P):] == -1)
        assert all(len(set(row[:min(k, P)].tolist())) == min(k, P) for row in ids)


def test_a_cpu_fitted_baseline_answers_with_the_host_forms():
    c = bc.case("walks")
    mb = data.MarkovBaseline.fit(c.ds, c.train, device="cpu")
    for order in bc.ORDERS:
        rank, revisit = mb.ranks(c.samples, order)
        assert np.array_equal(rank.numpy(), bc.host("walks", order)[0]) and np.array_equal(revisit.numpy(), bc.host("walks", order)[1])
        assert np.array_equal(mb.recommend(c.samples, 20, order).numpy(), bc.host_lists("walks", order, 20))


# ------------------------------------------------------------------------------------------------ the metric contract
def test_evaluate_is_restricted_sums_on_dense_scores_of_the_same_order():
    """order="global": the f32 score cg * P + (P - 1 - pop_rank) is exact (P = 30, counts <= 255: below 2**24) and orders the POIs
    as the key does, without ties -- so metrics.restricted_sums, the contract of EvalLoop's kernel, must count the same hits and
    sum the same gains; its slots 1 and 2, with the history POIs as hist, are the split."""
    c = bc.case("walks")
    mb = baseline.MarkovBaseline.fit(c.ds, c.train, device="cpu")
    P = mb.P
    base, a, t = bc.previous_and_target(c.samples)
    assert P <= 256 and int(mb.graph.val.max()) <= 255 and (t != 1).all()
    cg = torch.from_numpy(mb.graph.to_dense())
    scores = cg[torch.from_numpy(a - 1)] * P + (P - 1 - mb.pop_rank.float())[None, :]
    assert scores.dtype == torch.float32 and all(len(set(row.tolist())) == P for row in scores)
    Q = len(t)
    hist = np.zeros((Q, int(c.samples.cut.max())), dtype=np.int64)
    for q in range(Q):
        hist[q, :c.samples.cut[q]] = c.samples[q].checkins[:-1, 0]
    sums = metrics.restricted_sums(scores, torch.from_numpy(t), target_offset=-1, hist=torch.from_numpy(hist), hist_offset=1, split=True)
    assert sums[:, 10].tolist() == sums[:, 0].tolist() == [Q, Q - int(bc.host("walks", "global")[1].sum()), int(bc.host("walks", "global")[1].sum())]
    want = metrics.finalize_restricted(sums)
    got = mb.evaluate(c.samples, order="global", split_revisits=True)
    assert set(got) == set(metrics.finalize(metrics.new_accumulator("cpu"))) | {"new", "revisit"}
    assert set(mb.evaluate(c.samples, order="global")) == set(got) - {"new", "revisit"}
    for g, w in ((got, want), (got["new"], want["new"]), (got["revisit"], want["revisit"])):
        assert g["n"] == w["n"] > 0
        for k in (1, 5, 10, 20):
            assert round(g[f"acc@{k}"] * g["n"]) == round(w[f"acc@{k}"] * w["n"]) and g[f"acc@{k}"] == w[f"acc@{k}"]     # hit counts
            assert g[f"ndcg@{k}"] == pytest.approx(w[f"ndcg@{k}"], rel=1e-12, abs=0)    # (f64 sums of the same terms)
        assert g["mrr"] == pytest.approx(w["mrr"], rel=1e-12, abs=0)
    assert 0 < got["acc@1"] < got["acc@20"] < 1                      # (the case separates the cut-offs)


def test_evaluate_of_nothing():
    c = bc.case("empty")
    out = baseline.MarkovBaseline.fit(c.ds, c.train, device="cpu").evaluate(c.samples, split_revisits=True)
    assert out["n"] == out["new"]["n"] == out["revisit"]["n"] == 0 and out["acc@1"] == out["mrr"] == 0.0


# ------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_cpu_fitted_tables(name):
    c = bc.case(name)
    mb = baseline.MarkovBaseline.fit(c.ds, c.train, device="cpu")
    P = mb.P
    adj = data.universe_counts_host(c.ds, c.train, P=P).graph_adj
    for f in ("rowptr", "col", "val"):
        x, y = getattr(mb.graph, f), getattr(adj, f)
        assert x.dtype == y.dtype and torch.equal(x, y), f
    cu, pop = {}, np.zeros(P, dtype=np.int64)
    for s in np.nonzero(c.train)[0]:
        p = c.ds[int(s)].checkins[:, 0].astype(np.int64)
        np.add.at(pop, p - 1, 1)
        for x, y in zip(p[:-1], p[1:]):
            key = (int(c.ds.users[s]) * P + int(x) - 1) * P + int(y) - 1
            cu[key] = cu.get(key, 0) + 1
    assert mb.ukey.dtype == torch.int64 and mb.ukey.tolist() == sorted(cu) and mb.uval.tolist() == [cu[k] for k in sorted(cu)]
    assert mb.pop.tolist() == pop.tolist() and mb.U == (int(c.ds.users.max()) + 1 if len(c.ds) else 0)
    assert mb.pop_order.tolist() == sorted(range(P), key=lambda p: (-pop[p], p))
    assert mb.pop_rank[mb.pop_order.long()].tolist() == list(range(P))
    assert all(v.dtype == torch.int32 for v in (mb.uval, mb.pop, mb.pop_rank, mb.pop_order, mb.graph.col, mb.graph.val))
