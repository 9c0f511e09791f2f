"""The Markov prior's rule on the host (mobgt_amd.prior: blend_host, the reference of the kernel in csrc_prior/prior.hip, and a
MarkovPrior made of a CPU-fitted baseline): the miniature's rows written out by hand, blend_host against a brute-force form that
recounts the tables from the sessions, the log tables bit for bit, every refusal, the header, the anchor and the user a collated
batch carries, and the ranks of blended rows through metrics.restricted_sums."""
import numpy as np
import pytest
import torch

import prior_cases as pc
from mobgt_amd import _prior, baseline, data, metrics, prior

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dataset(sessions):
    return data.SessionDataset([(u, pc.as_checkins(p)) for u, p in sessions])


@pytest.fixture(scope="module")
def mini():
    ds = dataset(pc.MINI_TRAIN)
    mb = baseline.MarkovBaseline.fit(ds, np.ones(len(ds), dtype=bool), P=pc.MINI_P, device="cpu")
    return mb, mb.prior(*pc.MINI_WEIGHTS)


@pytest.fixture(scope="module")
def walks():
    sessions = pc.walks()
    ds = dataset(sessions)
    train = np.arange(len(ds)) % 4 != 3
    mb = baseline.MarkovBaseline.fit(ds, train, P=30, device="cpu")
    return sessions, ds, train, mb


# ------------------------------------------------------------------------------------------------ the rule
def test_the_miniature_counts_to_what_the_case_says(mini):
    mb, pr = mini
    rowptr, col, val = (v.numpy() for v in (mb.graph.rowptr, mb.graph.col, mb.graph.val))
    cg = {a: {int(col[e]) + 1: int(val[e]) for e in range(rowptr[a - 1], rowptr[a])} for a in range(1, 6) if rowptr[a] > rowptr[a - 1]}
    assert cg == pc.MINI_CG and mb.pop.tolist() == pc.MINI_POP and (mb.P, mb.U) == (5, 2)
    cu = {}
    for k, n in zip(mb.ukey.tolist(), mb.uval.tolist()):
        cu.setdefault((k // 25, k // 5 % 5 + 1), {})[k % 5 + 1] = n
    assert cu == pc.MINI_CU and pr.get_weights() == dict(zip(prior.WEIGHTS, pc.MINI_WEIGHTS))


def test_rows_of_the_miniature_written_out(mini):
    _, pr = mini
    hist = np.array([r[0] for r in pc.MINI_ROWS], dtype=np.int64)
    user = np.array([r[1] for r in pc.MINI_ROWS], dtype=np.int64)
    want = np.array([r[2] for r in pc.MINI_ROWS], dtype=F)
    scores = np.tile(pc.MINI_SCORES, (len(hist), 1))
    status = [0]
    got = prior.blend_host(scores, hist, user, pr.tables(), pc.MINI_WEIGHTS, 1, status=status)
    assert got.dtype == F and np.array_equal(bits(got), bits(want)) and status == [0]
    assert np.all(bits(got[:, 4]) == 0x80000000)                        # POI 5: nothing applies, -0.0 survives
    assert not np.array_equal(got[0], got[2]) and not np.array_equal(got[2], got[1])      # the user term and the transition term count
    # the public call of a CPU prior is the host form, in place by default and into `out` otherwise
    s = torch.from_numpy(scores.copy())
    assert pr.blend(s, (torch.from_numpy(hist), torch.from_numpy(user)), 1) is s and np.array_equal(bits(s.numpy()), bits(want))
    out = torch.full((len(hist), 7), 9.0)
    pr.blend(torch.from_numpy(scores.copy()), (torch.from_numpy(hist).int(), torch.from_numpy(user).int().reshape(-1, 1)), 1, out=out)
    assert np.array_equal(bits(out[:, :5].numpy()), bits(want)) and bool((out[:, 5:] == 9.0).all())
    # label_offset 0 with V = 6: column 0 is no POI and keeps its score, the others shift by one
    wide = np.concatenate([np.full((len(hist), 1), F(3.5)), scores], axis=1)
    got0 = prior.blend_host(wide, hist, user, pr.tables(), pc.MINI_WEIGHTS, 0)
    assert np.all(got0[:, 0] == F(3.5)) and np.array_equal(bits(got0[:, 1:]), bits(want))
    # V < P: the entries beyond the scores are skipped silently
    assert np.array_equal(bits(prior.blend_host(scores[:, :2], hist, user, pr.tables(), pc.MINI_WEIGHTS, 1)), bits(want[:, :2]))


def brute_force(sessions, train, P, scores, hist, user, weights, label_offset):
    """The rule column by column, the counts taken from the train sessions with dicts."""
    cg, cu, pop = {}, {}, {}
    for (u, p), tr in zip(sessions, train):
        if tr:
            for x in p:
                pop[x] = pop.get(x, 0) + 1
            for a, b in zip(p[:-1], p[1:]):
                cg[(a, b)] = cg.get((a, b), 0) + 1
                cu[(u, a, b)] = cu.get((u, a, b), 0) + 1
    wu, wg, wp = (F(w) for w in weights)
    out = np.array(scores, dtype=F)
    for g in range(out.shape[0]):
        ids = [int(x) for x in hist[g] if x != 0]
        a = ids[-1] if ids and 1 <= ids[-1] <= P else None
        u = int(user[g]) - 1
        for c in range(out.shape[1]):
            p, s = c + label_offset, out[g, c]
            if 1 <= p <= P and pop.get(p, 0) > 0:
                s = F(s + F(wp * pc.L(pop[p])))
            if a is not None and cg.get((a, p), 0) > 0:
                s = F(s + F(wg * pc.L(cg[(a, p)])))
                if cu.get((u, a, p), 0) > 0:
                    s = F(s + F(wu * pc.L(cu[(u, a, p)])))
            out[g, c] = s
    return out


@pytest.mark.parametrize("label_offset, V", [(1, 30), (0, 31), (1, 31), (1, 17)])
def test_blend_host_equals_the_brute_force_form(walks, label_offset, V):
    sessions, ds, train, mb = walks
    pr = mb.prior(user=0.75, transition=1.5, popularity=0.3)
    test = [s for s, tr in zip(sessions, train) if not tr]
    hist = np.zeros((len(test) + 2, 9), dtype=np.int64)
    user = np.zeros(len(test) + 2, dtype=np.int64)
    for g, (u, p) in enumerate(test):
        hist[g, :len(p) - 1], user[g] = p[:-1], u + 1
    hist[-2, :2], user[-2] = (3, 31), 1                                 # an anchor beyond P; then an all-pad row of an unseen user
    user[-1] = 40
    scores = pc.scores(len(hist), V, seed=V)
    got = prior.blend_host(scores, hist, user, pr.tables(), (0.75, 1.5, 0.3), label_offset)
    want = brute_force(sessions, train, 30, scores, hist, user, (0.75, 1.5, 0.3), label_offset)
    assert np.array_equal(bits(got), bits(want))
    changed = bits(got) != bits(scores)
    assert changed.any(axis=1)[:-2].all() and 0.3 < changed.mean() < 1.0  # (pop = 0 for some POIs: those columns keep their bits)


def test_the_log_tables_bit_for_bit(walks):
    _, _, _, mb = walks
    pr = mb.prior()
    for got, counts in ((pr.lg, mb.graph.val), (pr.lu, mb.uval), (pr.lp, mb.pop)):
        want = np.float32(np.log1p(counts.numpy().astype(np.float64)))
        assert got.dtype == torch.float32 and got.shape == counts.shape and np.array_equal(bits(got.numpy()), bits(want))
    assert np.array_equal(bits(prior.log_table(5)), bits(np.float32(np.log1p(np.arange(6, dtype=np.float64)))))
    assert pr.rowptr is mb.graph.rowptr and pr.col is mb.graph.col and pr.ukey is mb.ukey and (pr.P, pr.U) == (mb.P, mb.U)
    assert int(mb.pop.min()) == 0 and float(pr.lp.min()) == 0.0 and float(pr.lg.min()) > 0   # a count is > 0 exactly where its log is
    assert data.MarkovPrior is prior.MarkovPrior and pr.weights.tolist() == [1.0, 1.0, 1.0] and pr.status.tolist() == [0]


def test_all_weights_zero_change_nothing_but_the_sign_of_zero(walks):
    _, _, _, mb = walks
    pr = mb.prior(0, 0, 0)
    scores = pc.scores(4, 30)
    hist, user = np.array([[1, 2], [3, 0], [0, 0], [7, 9]]), np.array([1, 2, 3, 99])
    got = prior.blend_host(scores, hist, user, pr.tables(), (0, 0, 0), 1)
    same = (got == scores) | (np.isnan(got) & np.isnan(scores))
    assert same.all() and (bits(got) != bits(scores)).sum() == ((bits(scores) == 0x80000000) & (bits(got) == 0)).sum()


# ------------------------------------------------------------------------------------------------ refusals
class _Model:
    label_offset = 1
    out_proj = torch.nn.Linear(2, 30)


def test_what_the_prior_refuses(walks, mini):
    _, ds, train, mb = walks
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39):
        with pytest.raises(ValueError, match="must be finite"):
            mb.prior(transition=bad)
        pr = mb.prior(0.5, 0.25, 2.0)
        with pytest.raises(ValueError, match="must be finite"):
            pr.set_weights(popularity=bad)
        assert pr.weights.tolist() == [0.5, 0.25, 2.0] and pr.get_weights()["popularity"] == 2.0    # nothing was changed
    assert pr.set_weights(transition=3.0).weights.tolist() == [0.5, 3.0, 2.0]
    with pytest.raises(ValueError, match="must be numbers"):
        mb.prior(user="much")
    for L in (0, 17):
        with pytest.raises(ValueError, match=rf"{L} rows, one loop sweeps 1 \.\. 16"):
            prior.sweep_weights(np.ones((L, 3)))
    for shape in ((3,), (2, 2), (2, 3, 1)):
        with pytest.raises(ValueError, match=r"\[L, 3\] rows of \(user, transition, popularity\) weights, got shape"):
            prior.sweep_weights(np.ones(shape))
    with pytest.raises(ValueError, match="must be finite"):
        prior.sweep_weights([[1, 2, float("nan")]])
    assert prior.sweep_weights(torch.ones(16, 3)).shape == (16, 3) and prior.MAX_SWEEP == 16
    with pytest.raises(ValueError, match="grid must be"):
        pr.tune(None, None, None, np.ones((2, 2)))
    # a prior on another device than the loop's, a universe the model does not score, too many rows
    with pytest.raises(ValueError, match="EvalLoop: the prior is on cpu, the loop on cuda:0"):
        pr.for_loop(_Model, "cuda:0", 16, "EvalLoop")
    pr.for_loop(_Model, "cpu", 16, "EvalLoop")
    with pytest.raises(ValueError, match=r"POIs 1 \.\. 31, the model scores 30 columns for POIs 1 \.\. 30"):
        baseline.MarkovBaseline.fit(ds, train, P=31, device="cpu").prior().for_loop(_Model, "cpu", 16, "EvalLoop")
    with pytest.raises(ValueError, match="batch_size 65536"):
        pr.for_loop(_Model, "cpu", 65536, "PredictLoop")
    # a PrefixDataset handed to fit
    with pytest.raises(TypeError, match=r"pds\.base"):
        baseline.MarkovBaseline.fit(data.PrefixDataset(ds, device="cpu"), train, device="cpu")
    # blend's own arguments
    s, h, u = torch.zeros(2, 30), torch.zeros(2, 3, dtype=torch.int64), torch.ones(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="scores must be f32"):
        pr.blend(s.double(), (h, u), 1)
    with pytest.raises(ValueError, match="out must be f32"):
        pr.blend(s, (h, u), 1, out=torch.zeros(2, 29))
    with pytest.raises(ValueError, match="label_offset must be 0 or 1"):
        pr.blend(s, (h, u), 2)
    with pytest.raises(ValueError, match="2 rows of scores, 3 of hist"):
        pr.blend(s, (torch.zeros(3, 3, dtype=torch.int64), u), 1)
    with pytest.raises(TypeError, match="hist must be int32 or int64"):
        pr.blend(s, (h.float(), u), 1)
    with pytest.raises(ValueError, match="weights must be a contiguous f32"):
        pr.blend(s, (h, u), 1, weights=torch.zeros(4))


def test_a_status_is_kept_and_reported(mini):
    mb, _ = mini
    pr = mb.prior(*pc.MINI_WEIGHTS)
    t = pr.tables()
    hist, user = np.array([[1], [2]]), np.array([1, 1])
    scores = np.tile(pc.MINI_SCORES, (2, 1))
    good = prior.blend_host(scores, hist, user, t, pc.MINI_WEIGHTS, 1)
    for rowptr in ([0, 2, 1, 5, 6, 6], [0, 7, 7, 7, 7, 7]):             # row 2 descends; row 1 runs beyond nnz
        status = [0]
        got = prior.blend_host(scores, hist, user, t._replace(rowptr=np.array(rowptr)), pc.MINI_WEIGHTS, 1, status=status)
        assert status == [prior.SBADINDEX] and got.shape == good.shape
    col = t.col.copy()
    col[1] = 5                                                          # row 1's last entry: POI 6 of 5
    status = [0]
    got = prior.blend_host(scores, hist, user, t._replace(col=col), pc.MINI_WEIGHTS, 1, status=status)
    assert status == [prior.SBADINDEX] and np.array_equal(bits(got[1]), bits(good[1]))
    assert np.array_equal(bits(got[0, :2]), bits(good[0, :2])) and bits(got[0, 2]) == bits(pc._POP_ONLY[2])     # that entry dropped, the rest blended
    pr.col = torch.from_numpy(col)
    pr._host_tables = None
    pr.blend(torch.from_numpy(scores.copy()), (torch.from_numpy(hist), torch.from_numpy(user)), 1)
    with pytest.raises(ValueError, match=rf"MarkovPrior.blend: .*\(status {prior.SBADINDEX}\)"):
        pr.check()
    assert pr.status.tolist() == [prior.SBADINDEX]                      # sticky: check() leaves it


def test_the_header_is_readable_without_the_built_library():
    sig = _prior.SIGNATURES
    assert list(sig) == ["mobgt_prior_abi_version", "mobgt_prior_blend_rows"] and _prior.ABI_VERSION == 1
    assert len(sig["mobgt_prior_blend_rows"][1]) == 28
    assert (_prior.EBADDIM, _prior.EALIGN, _prior.EDTYPE, _prior.SBADINDEX, _prior.I32, _prior.I64) == (-1, -2, -3, 1, 0, 1)
    assert _prior.CHUNK == pc.CHUNK == 2048 and _prior.CHUNK % _prior.THREADS == 0 and _prior.MAX_G == 65535
    from mobgt_amd import _baseline, _checkins, _native, _pairbins, _prefixes, _universe
    others = [lib.SIGNATURES for lib in _native.LIBRARIES] + [m.SIGNATURES for m in (_baseline, _checkins, _pairbins, _prefixes, _universe)]
    assert len(others) == 10 and not any(set(sig) & set(o) for o in others)
    assert len(_native._MODULES) == 5 and "_prior" not in _native._MODULES
    assert list(_baseline.SIGNATURES) == ["mobgt_baseline_abi_version", "mobgt_baseline_ranks", "mobgt_baseline_topk"]


# ------------------------------------------------------------------------------------------------ what a batch carries
def test_the_anchor_and_the_user_of_a_collated_batch(walks):
    """Sessions and every prefix of them through the host collate path (sessions_to_trajectories + DeviceCollator.pack_host): the
    last entry of x that is not 0 is the last history check-in poi(r_{c-1}) -- also for A, B, A, t, whose nodes are B, A -- and
    user - 1 is the session's user."""
    sessions, ds, _, _ = walks
    assert any(len(p) == 4 and p[0] == p[2] != p[1] for _, p in sessions)
    pds = data.PrefixDataset(ds, device="cpu")
    coll = data.DeviceCollator("cpu")
    for samples in (ds, pds):
        recs = [samples[i] for i in range(len(samples))]
        h = coll.pack_host(data.sessions_to_trajectories(recs))
        hist = h["x"].reshape(len(recs), -1)
        for g, r in enumerate(recs):
            ids = hist[g][hist[g] != 0]
            assert int(ids[-1]) == int(r.checkins[-2, 0]) and int(h["user"][g, 0]) - 1 == int(r.user)
    assert len(pds) > len(ds)


# ------------------------------------------------------------------------------------------------ the metric contract
def test_ranks_of_blended_rows_through_restricted_sums(walks):
    sessions, ds, train, mb = walks
    pr = mb.prior(user=1.0, transition=2.0, popularity=0.5)
    test = [s for s, tr in zip(sessions, train) if not tr]
    G, V = len(test), 30
    hist, user, y = np.zeros((G, 9), dtype=np.int64), np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    for g, (u, p) in enumerate(test):
        hist[g, :len(p) - 1], user[g], y[g] = p[:-1], u + 1, p[-1]
    plain = np.random.RandomState(5).standard_normal((G, V)).astype(F)
    blended = prior.blend_host(plain, hist, user, pr.tables(), (1.0, 2.0, 0.5), 1)
    sums = metrics.restricted_sums(torch.from_numpy(blended), torch.from_numpy(y), target_offset=-1)[0]
    live = G if not (y == 1).any() else int(np.argmax(y == 1))          # get_acc stops at the first target of column 0
    rank = np.zeros(G, dtype=np.int64)
    for g in range(G):
        order = np.lexsort((np.arange(V), -blended[g].astype(np.float64)))     # score descending, equal scores lower column first
        rank[g] = int(np.nonzero(order == y[g] - 1)[0][0])
    assert int(sums[0]) == G and [int(sums[1 + i]) for i in range(4)] == [int((rank[:live] < k).sum()) for k in (1, 5, 10, 20)]
    assert len(set(blended[0].tolist())) == V                           # (no ties here: the MRR position is the same rank)
    np.testing.assert_allclose(float(sums[9]), float((1.0 / (rank + 1.0)).sum()), rtol=1e-12)
    np.testing.assert_allclose(float(sums[5 + 3]), float((1.0 / np.log2(rank[:live][rank[:live] < 20] + 2.0)).sum()), rtol=1e-12)
    plain_sums = metrics.restricted_sums(torch.from_numpy(plain), torch.from_numpy(y), target_offset=-1)[0]
    assert float(sums[9]) > float(plain_sums[9])                        # the habit of the walks is in the tables: the prior helps
