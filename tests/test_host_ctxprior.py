"""The context prior's rule on the host (mobgt_amd.ctxprior: slot_hist_host, tables_from_counts and blend_host, the references of
the kernels in csrc_ctxprior/ctxprior.hip; a ContextPrior fitted on the CPU; prior.Stack with it): the histogram against a plain
loop, the tables against their formula, the blend's untouched elements bit for bit, every invalid context, every refusal, the
header, and that the fitted terms rank held-out check-ins better than popularity does, alone and together."""
import types

import numpy as np
import pytest
import torch

import ctxprior_cases as cc
import prior_cases as pc
from mobgt_amd import _ctxprior, baseline, ctxprior, data, prior, priorfit, universe

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the histogram
def test_slot_hist_host_is_the_plain_loop():
    lengths = [2, 9, 2, 1, 5, 2, 30, 3, 2, 7, 0, 4]                     # one pair, longer, a single row, an empty session
    S, C = 6, 5
    seq, offsets, train = cc.packed(lengths, S, C, seed=1, train=np.arange(len(lengths)) % 3 != 1)
    assert seq[0, 1] == 0 and train[0] and not train.all() and train.any()
    status = [0]
    st = ctxprior.slot_hist_host(seq, offsets, train, S, C, status=status)
    assert st.dtype == np.int64 and st.shape == (S, C) and st.tolist() == cc.loop_hist(seq, offsets, train, S, C) and status == [0]
    transitions = int(sum(max(n - 1, 0) for n, t in zip(lengths, train) if t))
    assert int(st.sum()) == transitions and st[0].sum() >= 1            # the slot-0 row leaves its pair in row 0
    sessions = [(0, seq[offsets[i]:offsets[i + 1]]) for i in range(len(lengths)) if lengths[i] >= 2]
    mask = np.array([bool(train[i]) for i in range(len(lengths)) if lengths[i] >= 2])
    ds = data.SessionDataset(sessions)
    counts = universe.universe_counts_host(ds, mask, n_cat=C)
    again = ctxprior.slot_hist_host(ds.seq, ds.offsets, mask, S, C)
    assert again.tolist() == st.tolist() and int(counts.graph_cat.sum()) == transitions == counts.T
    assert again.sum(axis=0).tolist() == counts.graph_cat.sum(dim=0).tolist()          # both count the pairs by the category entered
    assert int(ctxprior.slot_hist_host(seq, offsets, np.zeros(len(lengths)), S, C).sum()) == 0
    assert ctxprior.slot_hist_host(seq[:0], [0], [], S, C).tolist() == [[0] * C] * S


def test_slot_hist_host_skips_and_flags():
    lengths = [4, 3, 5, 2]
    S, C = 4, 3
    seq, offsets, train = cc.packed(lengths, S, C, seed=2, train=np.ones(4))
    good = ctxprior.slot_hist_host(seq, offsets, train, S, C)

    def without(session):
        flags = train.copy()
        flags[session] = 0
        return ctxprior.slot_hist_host(seq, offsets, flags, S, C)
    down, beyond = offsets.copy(), offsets.copy()
    down[2] = offsets[1] - 1                                            # session 1 descends; session 2 starts early but is valid
    beyond[4] = len(seq) + 1
    for off, gone in ((beyond, 3),):
        status = [0]
        got = ctxprior.slot_hist_host(seq, off, train, S, C, status=status)
        assert status == [ctxprior.SBADINDEX] and got.tolist() == without(gone).tolist()
    status = [0]
    got = ctxprior.slot_hist_host(seq, down, train, S, C, status=status)
    assert status == [ctxprior.SBADINDEX] and got.tolist() == cc.loop_hist(seq, down, train, S, C)
    assert int(got.sum()) == int(good.sum()) - 2 + 4                    # session 1's 2 pairs are gone, session 2 gained 4 with its rows
    for column, value in ((1, -1), (1, S), (2, 0), (2, C + 1)):
        bad = seq.copy()
        k = 5                                                           # session 1's second row: second of one pair, first of the next
        bad[k, column] = value
        status = [7 & ~ctxprior.SBADVALUE]
        got = ctxprior.slot_hist_host(bad, offsets, train, S, C, status=status)
        one = np.zeros((S, C), dtype=np.int64)
        if column == 1:
            one[seq[k, 1], seq[k + 1, 2] - 1] = 1                       # the pair (k, k + 1) reads row k's slot
        else:
            one[seq[k - 1, 1], seq[k, 2] - 1] = 1                       # the pair (k - 1, k) reads row k's category
        assert status == [7] and got.tolist() == (good - one).tolist(), (column, value)     # ORed into, one pair skipped


# ------------------------------------------------------------------------------------------------ the tables
def test_tables_from_counts_is_the_formula():
    rng = np.random.RandomState(3)
    C, S = 5, 4
    gc = rng.randint(0, 50, size=(C, C)).astype(np.int64)
    gc[2] = 0                                                           # an empty row
    gc[:, 3] = 0                                                        # an empty column
    gc[0, 0] = 10 ** 12
    st = rng.randint(0, 9, size=(S, C)).astype(np.int64)
    st[1] = 0
    st[:, 3] = 0
    Tc, Tt = ctxprior.tables_from_counts(gc, st)
    assert Tc.dtype == F and Tt.dtype == F and Tc.shape == (C, C) and Tt.shape == (S, C) and np.isfinite(Tc).all() and np.isfinite(Tt).all()
    m = [sum(int(gc[a, b]) for a in range(C)) for b in range(C)]
    M = sum(m)
    base = [np.log((float(m[b]) + 1.0) / (float(M) + C)) for b in range(C)]
    for counts, table in ((gc, Tc), (st, Tt)):
        for r in range(counts.shape[0]):
            row = float(sum(int(v) for v in counts[r]))
            want = [np.float32(np.log((float(counts[r, b]) + 1.0) / (row + C)) - base[b]) for b in range(C)]
            assert np.array_equal(bits(table[r]), bits(np.array(want))), r
    # a row whose counts are proportional to the marginal lifts nothing
    gc = np.outer([1, 2, 3], [100, 200, 700]).astype(np.int64) * 50
    st = np.array([[1000, 2000, 7000], [0, 0, 0]], dtype=np.int64)
    Tc, Tt = ctxprior.tables_from_counts(gc, st)
    assert np.abs(Tc).max() < 2e-2 and np.abs(Tt[0]).max() < 2e-3
    assert Tt[1, 0] > 0 > Tt[1, 2]                                      # an empty row is uniform: rare categories lifted, common ones lowered
    for a, b in ((gc[:2], st), (gc, st[:, :2]), (gc.astype(np.float64), st), (gc, st[0])):
        with pytest.raises(ValueError, match=r"integer counts \[C, C\] and \[S, C\]"):
            ctxprior.tables_from_counts(a, b)
    with pytest.raises(ValueError, match="negative"):
        ctxprior.tables_from_counts(gc, -st)


# ------------------------------------------------------------------------------------------------ the blend
@pytest.mark.parametrize("label_offset", (0, 1))
@pytest.mark.parametrize("V", (5, 10, 13))                             # P = 9: V < P, V = P + 1, V > P + 1
def test_blend_host_touches_exactly_what_the_rule_names(V, label_offset):
    P, C, S = 9, 4, 6
    t = cc.tables(P, C, S, seed=V)
    assert (t.poi_cat == 0).any() or t.poi_cat[2] == C + 1
    G = len(cc.CONTEXTS)
    hist, time, cat = cc.sample_rows(G, P, C, S, seed=V, dtype=np.int64)
    scores = pc.scores(G, V, seed=V)
    special = np.array([0x7F800000, 0xFF800000, 0x80000000, 0x7FC00001, 0xFFC12345], dtype=np.uint32)
    for g in (0, 3, 5, 7):                                              # +-inf, -0.0 and two NaN payloads: valid, no anchor, no category, no slot
        scores[g, :5] = special.view(F)
    wc, wt = F(0.75), F(-1.25)
    got = ctxprior.blend_host(scores, hist, time, cat, t, (wc, wt), label_offset)
    assert got.dtype == F and got.shape == scores.shape
    rows = cc.anchors(hist, time, cat)
    cases = set()
    for g, anchor in enumerate(rows):
        for c in range(V):
            p = c + label_offset
            k = int(t.poi_cat[p - 1]) if 1 <= p <= P else 0
            if anchor is None or not 1 <= anchor[0] <= P or not 1 <= k <= C:
                assert bits(got[g, c]) == bits(scores[g, c]), (g, c)   # copied bit for bit
                continue
            _, ca, ta = anchor
            v = scores[g, c]
            if 1 <= ca <= C:
                v = F(v + F(wc * t.cat_table[ca - 1, k - 1]))
            if 0 <= ta < S:
                v = F(v + F(wt * t.slot_table[ta, k - 1]))
            assert bits(got[g, c]) == bits(v), (g, c)
            cases.add((1 <= ca <= C, 0 <= ta < S))
    assert cases == {(True, True), (True, False), (False, True), (False, False)}
    assert np.array_equal(bits(got[3, :5]), special)                    # no anchor: the specials survive
    assert rows[3] is None and rows[4][0] == P + 1 and rows[5][1] == 0 and rows[6][1] == C + 1 and rows[7][2] == -1 and rows[8][2] == S
    # [G, n, 1] as the collators leave them
    again = ctxprior.blend_host(scores, hist[:, :, None], time[:, :, None], cat[:, :, None], t, (wc, wt), label_offset)
    assert np.array_equal(bits(again), bits(got))
    # with weights 0 the terms are still added: -0.0 becomes +0.0 where a table entry is not negative, nothing else changes
    zero = ctxprior.blend_host(scores, hist, time, cat, t, (0.0, 0.0), label_offset)
    assert ((zero == scores) | (np.isnan(zero) & np.isnan(scores))).all()
    flipped = bits(zero) != bits(scores)
    assert ((bits(scores)[flipped] == 0x80000000) & (bits(zero)[flipped] == 0)).all() and not flipped[[3, 4, 9, 10, 11]].any()
    # one weight at 0 leaves the other term as it is, up to the sign of a zero
    only = ctxprior.blend_host(scores, hist, time, cat, t, (wc, 0.0), label_offset)
    no_time = ctxprior.blend_host(scores, hist, np.full_like(time, -1), cat, t, (wc, wt), label_offset)
    assert ((only == no_time) | (np.isnan(only) & np.isnan(no_time))).all()


# ------------------------------------------------------------------------------------------------ a CPU prior, the stack
@pytest.fixture(scope="module")
def log():
    sessions, mask, poi_cat = cc.context_log(seed=0)
    ds = data.SessionDataset(sessions)
    mb = baseline.MarkovBaseline.fit(ds, mask, P=400, device="cpu")
    cp = data.ContextPrior.fit(ds, mask, device="cpu")
    return sessions, mask, poi_cat, ds, mb, cp


def test_a_prior_fitted_on_the_cpu(log):
    sessions, mask, poi_cat, ds, mb, cp = log
    assert isinstance(cp, ctxprior.ContextPrior) and data.ContextPrior is ctxprior.ContextPrior
    counts = universe.universe_counts_host(ds, mask)
    assert (cp.P, cp.n_cat, cp.n_slots) == (400, 12, 48) and cp.device.type == "cpu"
    visited = counts.checkin_cnt.numpy() > 0
    assert np.array_equal(cp.poi_cat.numpy()[visited], poi_cat[visited]) and not cp.poi_cat.numpy()[~visited].any()
    assert cp.graph_cat.dtype == np.int64 and cp.graph_cat.tolist() == counts.graph_cat.tolist()
    st = ctxprior.slot_hist_host(ds.seq, ds.offsets, mask, 48, 12)
    assert cp.slot_cat.dtype == np.int64 and cp.slot_cat.tolist() == st.tolist() and int(st.sum()) == int(mask.sum()) * 8 == counts.T
    Tc, Tt = ctxprior.tables_from_counts(cp.graph_cat, st)
    assert cp.cat_table.dtype == torch.float32 and np.array_equal(bits(cp.cat_table.numpy()), bits(Tc))
    assert np.array_equal(bits(cp.slot_table.numpy()), bits(Tt)) and cp.status.tolist() == [0]
    t = cp.tables()
    assert np.array_equal(bits(t.cat_table), bits(Tc)) and np.array_equal(bits(t.slot_table), bits(Tt)) and t.poi_cat.tolist() == cp.poi_cat.tolist()
    assert (t.P, t.n_cat, t.n_slots) == (400, 12, 48)
    assert cp.lift("category")[0] is cp.graph_cat and np.array_equal(bits(cp.lift("category")[1]), bits(Tc))
    assert cp.lift("time")[0] is cp.slot_cat and np.array_equal(bits(cp.lift("time")[1]), bits(Tt))
    assert cp.weights.tolist() == [1.0, 1.0] and cp.get_weights() == {"category": 1.0, "time": 1.0} and cp.n_weights == 2
    assert cp.WEIGHTS == ("category", "time")
    given = data.ContextPrior.fit(ds, mask, counts=counts, n_slots=50, category=0.5, time=-2.0, device="cpu")
    assert given.slot_cat.shape == (50, 12) and given.slot_cat[:48].tolist() == st.tolist() and not given.slot_cat[48:].any()
    assert given.poi_cat is not None and given.weights.tolist() == [0.5, -2.0] and given.graph_cat.tolist() == cp.graph_cat.tolist()
    assert given.set_weights(time=3.0).weights.tolist() == [0.5, 3.0] and given.set_weights().get_weights() == {"category": 0.5, "time": 3.0}
    # the public call of a CPU prior is the host form, in place by default and into `out` otherwise
    hist, time, cat = cc.sample_rows(16, 400, 12, 48, dtype=np.int64)
    scores = pc.scores(16, 401)
    want = ctxprior.blend_host(scores, hist, time, cat, t, (1.0, 1.0), 1)
    th, tt, tc = (torch.from_numpy(v) for v in (hist, time, cat))
    s = torch.from_numpy(scores.copy())
    assert cp.blend(s, (th, tt, tc), 1) is s and np.array_equal(bits(s.numpy()), bits(want)) and (bits(want) != bits(scores)).any()
    out = torch.full((16, 403), 9.0)
    h32, t32, c32 = cc.sample_rows(16, 400, 12, 48, seed=1)             # int32 [G, n, 1] as the collators leave them ...
    batch = types.SimpleNamespace(x=torch.from_numpy(h32)[:, :, None], time=torch.from_numpy(t32)[:, :, None],
                                  cat=torch.from_numpy(c32).long()[:, :, None])               # ... and time and cat of two dtypes
    cp.blend(torch.from_numpy(scores.copy()), batch, 1, out=out, weights=torch.tensor([9.0, 1.0, 1.0])[1:])
    assert np.array_equal(bits(out[:, :401].numpy()), bits(ctxprior.blend_host(scores, h32, t32, c32, t, (1.0, 1.0), 1)))
    assert bool((out[:, 401:] == 9.0).all())
    # features: the table values themselves, 0 where the rule adds nothing
    feats = cp.features((th, tt, tc), 1, torch.full((2, 16, 401), 5.0))
    assert np.array_equal(bits(feats[0].numpy()), bits(ctxprior.blend_host(np.zeros((16, 401), F), hist, time, cat, t, (1.0, 0.0), 1)))
    assert np.array_equal(bits(feats[1].numpy()), bits(ctxprior.blend_host(np.zeros((16, 401), F), hist, time, cat, t, (0.0, 1.0), 1)))


def test_a_stack_with_the_markov_prior_is_the_host_rules_in_turn(log):
    _, _, _, _, mb, cp = log
    mp = mb.prior(0.75, 1.5, 0.3)
    cp = ctxprior.ContextPrior(cp.poi_cat, cp.graph_cat, cp.slot_cat, cp.tables().cat_table, cp.tables().slot_table, 0.6, -0.4)
    st = prior.Stack(mp, cp)
    assert st.WEIGHTS == ("user", "transition", "popularity", "category", "time") and st.n_weights == 5
    hist, time, cat = cc.sample_rows(16, 400, 12, 48, seed=4, dtype=np.int64)
    user = np.arange(1, 17)
    scores = pc.scores(16, 401, seed=4)
    batch = types.SimpleNamespace(**{k: torch.from_numpy(v) for k, v in dict(x=hist, user=user, time=time, cat=cat).items()})
    turn = lambda wm, wc: ctxprior.blend_host(prior.blend_host(scores, hist, user, mp.tables(), wm, 1), hist, time, cat, cp.tables(), wc, 1)
    got = st.blend(torch.from_numpy(scores.copy()), batch, 1)
    assert np.array_equal(bits(got.numpy()), bits(turn((0.75, 1.5, 0.3), (0.6, -0.4))))
    W = torch.tensor([[9.0] * 5, [0.5, 0.25, 2.0, -1.5, 3.0]])
    out = torch.full((16, 404), 9.0)
    assert st.blend(torch.from_numpy(scores.copy()), batch, 1, out=out, weights=W[1]) is out
    assert np.array_equal(bits(out[:, :401].numpy()), bits(turn((0.5, 0.25, 2.0), (-1.5, 3.0)))) and bool((out[:, 401:] == 9.0).all())
    st.set_weights(time=2.0, user=0.0)
    assert cp.weights.tolist() == [pytest.approx(0.6), 2.0] and mp.weights.tolist()[0] == 0.0
    st.check()
    with pytest.raises(ValueError, match=r"\[L, 5\] rows of \(user, transition, popularity, category, time\) weights, got shape"):
        prior.sweep_weights(np.ones((2, 4)), names=st.WEIGHTS)
    with pytest.raises(ValueError, match="category, time belong to more than one member"):
        prior.Stack(cp, cp)


class _Model:
    label_offset = 1
    out_proj = torch.nn.Linear(2, 400)


def test_what_the_context_prior_refuses(log):
    sessions, mask, _, ds, mb, cp = log
    with pytest.raises(TypeError, match="a PrefixDataset holds every transition of a session once per prefix"):
        data.ContextPrior.fit(data.PrefixDataset(ds, device="cpu"), mask, device="cpu")
    counts = universe.universe_counts_host(ds, mask)
    with pytest.raises(ValueError, match="the counts are on cpu, the prior is fitted on meta"):
        data.ContextPrior.fit(ds, mask, counts=counts, device="meta")
    with pytest.raises(TypeError, match="counts must be a data.UniverseCounts"):
        data.ContextPrior.fit(ds, mask, counts=mb, device="cpu")
    with pytest.raises(ValueError, match=r"time slot \d+ at check-in \d+ is not in 0 .. 46 \(n_slots = 47\)"):
        data.ContextPrior.fit(ds, mask, counts=counts, n_slots=47, device="cpu")
    with pytest.raises(ValueError, match=rf"n_slots = {ctxprior.MAX_SLOTS + 1} / n_cat = 12 outside the kernels' limits"):
        data.ContextPrior.fit(ds, mask, counts=counts, n_slots=ctxprior.MAX_SLOTS + 1, device="cpu")
    early = [(u, s.copy()) for u, s in sessions[:3]]
    early[1][1][2, 1] = -1
    with pytest.raises(ValueError, match=r"session 1: time slot -1 at check-in 2 is not in 0 .. \d+$"):
        data.ContextPrior.fit(early, [True, True, False], device="cpu")
    with pytest.raises(RuntimeError, match="the counts are not those of this ds and train"):
        data.ContextPrior.fit(ds, ~mask, counts=counts, device="cpu")
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match=r"the weights \(category, time\) must be finite"):
            data.ContextPrior.fit(ds, mask, counts=counts, time=bad, device="cpu")
    with pytest.raises(ValueError, match="must be finite"):
        cp.set_weights(category=float("nan"))
    assert cp.weights.tolist() == [1.0, 1.0]
    with pytest.raises(ValueError, match="kind must be one of category, time"):
        cp.lift("distance")
    with pytest.raises(ValueError, match="EvalLoop: the prior is on cpu, the loop on cuda:0"):
        cp.for_loop(_Model, "cuda:0", 16, "EvalLoop")
    cp.for_loop(_Model, "cpu", 16, "EvalLoop")
    with pytest.raises(ValueError, match="batch_size 65536"):
        cp.for_loop(_Model, "cpu", 65536, "PredictLoop")
    with pytest.raises(ValueError, match=r"POIs 1 .. 400, the model scores 399 columns"):
        cp.for_loop(types.SimpleNamespace(label_offset=1, out_proj=torch.nn.Linear(2, 399)), "cpu", 16, "EvalLoop")
    s, h = torch.zeros(2, 400), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="scores must be f32"):
        cp.blend(s.double(), (h, h, h), 1)
    with pytest.raises(ValueError, match="out must be f32"):
        cp.blend(s, (h, h, h), 1, out=torch.zeros(2, 399))
    with pytest.raises(ValueError, match="label_offset must be 0 or 1"):
        cp.blend(s, (h, h, h), 2)
    with pytest.raises(TypeError, match="cat must be int32 or int64"):
        cp.blend(s, (h, h, h.float()), 1)
    with pytest.raises(ValueError, match=r"a \(hist, user\) pair carries no slots or categories"):
        cp.blend(s, (h, torch.ones(2, dtype=torch.int64)), 1)
    with pytest.raises(TypeError, match=r"has no \.time, \.cat"):
        cp.blend(s, types.SimpleNamespace(x=h), 1)
    with pytest.raises(ValueError, match="2 rows of scores; hist"):
        cp.blend(s, (h, h, h[:, :2]), 1)
    with pytest.raises(ValueError, match=r"weights must be a contiguous f32 \[2\]"):
        cp.blend(s, (h, h, h), 1, weights=torch.zeros(3))
    with pytest.raises(ValueError, match=r"grid must be \[L >= 1, 2\]"):
        cp.tune(None, None, None, np.ones((2, 3)))
    cp.status |= ctxprior.SBADVALUE
    with pytest.raises(ValueError, match=rf"EvalLoop: .*\(status {ctxprior.SBADVALUE}\)"):
        cp.check("EvalLoop")
    cp.reset_status()
    cp.check()


def test_the_header_is_readable_without_the_built_library():
    sig = _ctxprior.SIGNATURES
    assert list(sig) == ["mobgt_ctxprior_abi_version", "mobgt_ctxprior_slot_hist", "mobgt_ctxprior_blend_rows"]
    assert _ctxprior.ABI_VERSION == 1 and [len(sig[k][1]) for k in list(sig)[1:]] == [10, 23]
    c = _ctxprior
    assert (c.EBADDIM, c.EALIGN, c.EDTYPE, c.SBADINDEX, c.SBADVALUE, c.I32, c.I64) == (-1, -2, -3, 1, 2, 0, 1)
    assert c.CHUNK % (4 * c.THREADS) == 0 and c.SESSIONS % (c.THREADS // 64) == 0 and c.MAX_G == 65535
    assert 4 * c.LDS_CELLS <= 160 * 1024 and 2 * 4 * c.MAX_CAT <= 64 * 1024 and c.LDS_CELLS < c.MAX_SLOTS * c.MAX_CAT < 2 ** 31
    from mobgt_amd import _geoprior, _native, _universe
    assert c.MAX_CAT == _universe.MAX_CAT                               # every UniverseCounts fits
    assert not set(sig) & set(_geoprior.SIGNATURES) and "_ctxprior" not in _native._MODULES and len(_native._MODULES) == 5


# ------------------------------------------------------------------------------------------------ the rule does something
def _mrr(blended, targets):
    """baseline's tie rule: score descending, equal scores lower POI first"""
    rr = []
    for s, y in zip(blended, targets):
        order = np.lexsort((np.arange(s.size), -s.astype(np.float64)))
        rr.append(1.0 / (int(np.nonzero(order == y - 1)[0][0]) + 1))
    return float(np.mean(rr))


def _held_out(log):
    sessions, mask, _, _, mb, cp = log
    hist, time, cat, user, y = cc.held_out_prefixes(sessions, mask)
    rows = tuple(torch.from_numpy(v) for v in (hist, time, cat))
    return rows, (rows[0], torch.from_numpy(user)), y, mb.prior(user=0.0, transition=0.0, popularity=1.0), cp


def test_each_fitted_term_ranks_better_than_popularity_and_both_better_than_either(log):
    """context_log(seed=0): 400 POIs, 12 categories, 48 slots, 720 sessions of 8 transitions, the next category drawn ~
    A[category] * T[slot] with Dirichlet(0.15) rows, the POI inside it by popularity; 493 train sessions, the 1 816 prefixes of the
    227 others held out; all model scores zero, everything through the package's host path (SessionDataset, MarkovBaseline.fit,
    ContextPrior.fit, the priors' CPU blends).  Measured MRR: popularity alone 0.1991, + category 0.3090, + time 0.3394,
    + both 0.4699.  Asserted: each term over popularity, both over either, by 0.01 at least."""
    rows, pair, y, pop, cp = _held_out(log)
    assert len(y) == 1816
    base = pop.blend(torch.zeros(len(y), 400), pair, 1)
    w = lambda *v: torch.tensor(v, dtype=torch.float32)
    mrr_pop = _mrr(base.numpy(), y)
    mrr_cat = _mrr(cp.blend(base.clone(), rows, 1, weights=w(1.0, 0.0)).numpy(), y)
    mrr_time = _mrr(cp.blend(base.clone(), rows, 1, weights=w(0.0, 1.0)).numpy(), y)
    mrr_both = _mrr(cp.blend(base.clone(), rows, 1, weights=w(1.0, 1.0)).numpy(), y)
    print(f"MRR: popularity {mrr_pop:.4f}, + category {mrr_cat:.4f}, + time {mrr_time:.4f}, + both {mrr_both:.4f}")
    margin = 0.01
    assert mrr_cat >= mrr_pop + margin and mrr_time >= mrr_pop + margin
    assert mrr_both >= mrr_cat + margin and mrr_both >= mrr_time + margin


def test_the_weights_fitted_by_maximum_likelihood_beat_popularity_alone(log):
    """priorfit.fit_host on the held-out prefixes of context_log(seed=0), K = 3 features (popularity, category, time), from
    w = 0, l2 = 1e-3: it converges in 8 passes to about (1.15, 1.41, 1.50); the mean negative log-likelihood is 5.9915 (= log 400)
    at w = 0, 4.3300 at weights (1, 0, 0) and 2.6862 at the fitted ones."""
    rows, pair, y, pop, cp = _held_out(log)
    n = len(y)
    feats = torch.zeros(3, n, 400)
    feats[0] = pop.features(pair, 1, torch.zeros(3, n, 400))[2]
    cp.features(rows, 1, feats[1:])
    res = priorfit.fit_host(None, feats.numpy(), y, target_offset=-1, names=("popularity", "category", "time"), start=[0.0, 0.0, 0.0])
    terms, status = priorfit.terms_host(None, feats.numpy(), y, -1, [[1.0, 0.0, 0.0]])
    nll_pop = float(terms[0, :, 1].sum() / terms[0, :, 0].sum())
    print(f"fit: {res.weights}, passes {res.passes}, nll {res.nll_start:.4f} -> {res.nll:.4f}; popularity alone {nll_pop:.4f}")
    assert status == 0 and res.converged and res.n == n and res.passes <= 12 and res.nll_start == pytest.approx(np.log(400.0))
    assert res.nll < nll_pop < res.nll_start and all(res.weights[k] > 0.0 for k in ("popularity", "category", "time"))
