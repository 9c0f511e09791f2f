"""What the three priors share (mobgt_amd.prior.Prior and Tuned): a minimal prior defined here, with one weight, one table and
nothing but the three pieces of blend that are a prior's own, goes through the weights, features, a sweep's check and a Stack; and
tune is one function for every prior and for a Stack.  CPU only."""
import numpy as np
import pytest
import torch

import geoprior_cases as gc
import prior_cases as pc
from mobgt_amd import baseline, ctxprior, data, geo, geoprior, prior, train

F = np.float32
P, G, V = 30, 3, 31


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bonus_host(scores, hist, table, w, label_offset):
    """scores[g, c] + w * table[p - 1] for the POIs p = c + label_offset in 1 .. P, in the rows that have an anchor (a last id that
    is not 0, in 1 .. P); the product and the sum each rounded to f32."""
    s = np.array(scores, dtype=F)
    c_lo, c_hi = max(0, 1 - label_offset), min(s.shape[1], len(table) + 1 - label_offset)
    term = (F(w) * table[c_lo + label_offset - 1:c_hi + label_offset - 1]).astype(F)
    for g in range(s.shape[0]):
        ids = hist[g][hist[g] != 0]
        if len(ids) and 1 <= int(ids[-1]) <= len(table):
            s[g, c_lo:c_hi] = (s[g, c_lo:c_hi] + term).astype(F)
    return s


class BonusPrior(prior.Prior):
    """One weight, a table of P floats, rows = hist (or a batch's .x): everything else is Prior's."""
    NAME, WEIGHTS = "BonusPrior", ("bonus",)

    def __init__(self, table, bonus=1.0):
        self.table, self.P = torch.from_numpy(table), len(table)
        super().__init__([bonus])

    device = property(lambda self: self.table.device)

    @staticmethod
    def _rows(rows, G, what):
        return (("hist", rows if isinstance(rows, torch.Tensor) else rows.x),)

    def _blend_host(self, scores, ids, w, label_offset):
        return bonus_host(scores, ids[0], self.table.numpy(), w[0], label_offset)


class _Batch:
    pass


@pytest.fixture(scope="module")
def case():
    table = np.random.RandomState(3).standard_normal(P).astype(F)
    hist = np.array([[4, 9, 0, 0], [0, 0, 0, 0], [7, 0, 30, 0]], dtype=np.int64)
    return table, hist, pc.scores(G, V)


def test_a_minimal_prior_has_the_whole_interface(case):
    table, hist, scores = case
    bp = BonusPrior(table, 0.5)
    assert bp.n_weights == 1 and bp.get_weights() == {"bonus": 0.5} and bp.weights.tolist() == [0.5] and bp.status.tolist() == [0]
    assert bp.set_weights(2.0).get_weights() == {"bonus": 2.0} and bp.set_weights(bonus=-1.5).weights.tolist() == [-1.5]
    assert bp.set_weights(None).get_weights() == bp.set_weights(bonus=None).get_weights() == bp.set_weights().get_weights() == {"bonus": -1.5}
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match=r"BonusPrior.set_weights: the weights \(bonus\) must be finite"):
            bp.set_weights(bad)
        assert bp.weights.tolist() == [-1.5] and bp.get_weights() == {"bonus": -1.5}     # nothing was changed
    for args, kw in (((1.0, 2.0), {}), ((), {"malus": 1.0}), ((1.0,), {"bonus": 2.0})):
        with pytest.raises(TypeError, match="BonusPrior.set_weights"):
            bp.set_weights(*args, **kw)
    assert bp.weights.tolist() == [-1.5]
    # blend: the frame is Prior's, the rule the class's own
    want = bonus_host(scores, hist, table, -1.5, 1)
    s = torch.from_numpy(scores.copy())
    assert bp.blend(s, torch.from_numpy(hist), 1) is s and np.array_equal(bits(s.numpy()), bits(want))
    assert np.array_equal(bits(want[1]), bits(scores[1])) and (bits(want[0]) != bits(scores[0])).any()
    out = torch.full((G, V + 2), 9.0)
    bp.blend(torch.from_numpy(scores.copy()), torch.from_numpy(hist), 0, out=out, weights=torch.tensor([0.25]))
    assert np.array_equal(bits(out[:, :V].numpy()), bits(bonus_host(scores, hist, table, 0.25, 0))) and bool((out[:, V:] == 9.0).all())
    with pytest.raises(ValueError, match="BonusPrior.blend: scores must be f32"):
        bp.blend(s.double(), torch.from_numpy(hist), 1)
    with pytest.raises(ValueError, match=r"BonusPrior.blend: weights must be a contiguous f32 \[1\] view"):
        bp.blend(s, torch.from_numpy(hist), 1, weights=torch.zeros(2))
    # features: the table where the rule adds it, 0 elsewhere
    feats = bp.features(torch.from_numpy(hist), 1, torch.full((1, G, V), 7.0))
    assert np.array_equal(bits(feats[0].numpy()), bits(bonus_host(np.zeros((G, V), dtype=F), hist, table, 1.0, 1)))
    assert bool((feats[0, 1] == 0).all()) and bp.weights.tolist() == [-1.5]
    # a sweep's rows are checked against the prior's names
    assert prior.sweep_weights([[1.0], [2.0]], names=bp.WEIGHTS).shape == (2, 1)
    with pytest.raises(ValueError, match=r"\[L, 1\] rows of \(bonus\) weights, got shape"):
        prior.sweep_weights(np.ones((2, 3)), names=bp.WEIGHTS)
    bp.check()
    bp.status |= 4
    bp.reset_status()
    assert bp.status.tolist() == [0]


def test_a_minimal_prior_in_a_stack(case):
    table, hist, scores = case
    ds = data.SessionDataset([(u, pc.as_checkins(p)) for u, p in pc.walks()])
    mb = baseline.MarkovBaseline.fit(ds, np.arange(len(ds)) % 4 != 3, P=P, device="cpu")
    mp, bp = mb.prior(0.5, 0.25, 2.0), BonusPrior(table, 0.75)
    st = prior.Stack(mp, bp)
    assert st.WEIGHTS == ("user", "transition", "popularity", "bonus") and st.n_weights == 4
    batch = _Batch()
    batch.x, batch.user = torch.from_numpy(hist), torch.tensor([1, 2, 3])
    want = prior.blend_host(scores, hist, batch.user.numpy(), mp.tables(), (0.5, 0.25, 2.0), 1)
    want = bonus_host(want, hist, table, 0.75, 1)
    s = torch.from_numpy(scores.copy())
    assert st.blend(s, batch, 1) is s and np.array_equal(bits(s.numpy()), bits(want))
    assert st.set_weights(bonus=3.0, user=-1.0).get_weights() == {"user": -1.0, "transition": 0.25, "popularity": 2.0, "bonus": 3.0}
    assert bp.weights.tolist() == [3.0] and mp.weights.tolist() == [-1.0, 0.25, 2.0]
    with pytest.raises(ValueError, match="must be finite"):
        st.set_weights(bonus=float("nan"), user=5.0)
    assert bp.weights.tolist() == [3.0] and mp.weights.tolist() == [-1.0, 0.25, 2.0]      # nothing was changed
    feats = st.features(batch, 1, torch.full((4, G, V), 7.0))
    assert np.array_equal(bits(feats[3].numpy()), bits(bonus_host(np.zeros((G, V), dtype=F), hist, table, 1.0, 1)))
    assert np.array_equal(bits(feats[:3].numpy()), bits(mp.features(batch, 1, torch.empty(3, G, V)).numpy()))


class _Loop:
    """train.EvalLoop as far as tune uses it: a result per weights row, the best the row whose first weight is largest."""
    seen = []

    def __init__(self, model, collator, val, prior=None, prior_weights=None, **kw):
        self.rows = np.asarray(prior_weights)
        _Loop.seen.append((type(prior).__name__, self.rows.shape))

    def run(self):
        return [{"mrr": float(r[0])} for r in self.rows]


def test_tune_is_one_function_for_every_prior_and_a_stack(case, monkeypatch):
    table = case[0]
    assert geoprior.DistancePrior.tune is prior.Stack.tune is prior.MarkovPrior.tune is ctxprior.ContextPrior.tune is prior.Tuned.tune
    assert geoprior.DistancePrior.fit_weights is prior.Stack.fit_weights is prior.Tuned.fit_weights
    ds = data.SessionDataset([(u, pc.as_checkins(p)) for u, p in pc.walks()])
    mb = baseline.MarkovBaseline.fit(ds, np.arange(len(ds)) % 4 != 3, P=P, device="cpu")
    dp = mb.distance_prior(geo.pair_bins(gc.city(P, seed=2), edges=np.arange(0.0, 30.0, 2.5), device="cpu"))
    st = prior.Stack(mb.prior(), dp)
    with pytest.raises(ValueError, match=r"DistancePrior.tune: grid must be \[L >= 1, 1\] rows of \(distance\) weights, got shape \(2, 2\)"):
        dp.tune(None, None, None, np.ones((2, 2)))
    with pytest.raises(ValueError, match=r"prior.Stack.tune: grid must be \[L >= 1, 4\] rows of \(user, transition, popularity, distance\) "
                                         r"weights, got shape \(2, 3\)"):
        st.tune(None, None, None, np.ones((2, 3)))
    with pytest.raises(ValueError, match=r"DistancePrior.tune: the weights \(distance\) must be finite"):
        dp.tune(None, None, None, [[float("inf")]])
    monkeypatch.setattr(train, "EvalLoop", _Loop)
    _Loop.seen.clear()
    grid = np.linspace(-1.0, 1.0, 20)[:, None] * np.array([[1.0]])
    grid[7, 0] = 5.0
    res = dp.tune(None, None, None, grid)
    assert len(res) == 20 and dp.get_weights() == {"distance": 5.0} and _Loop.seen == [("DistancePrior", (16, 1)), ("DistancePrior", (4, 1))]
    res = st.tune(None, None, None, [[0.0, 1.0, 2.0, 3.0], [4.0, 5.0, 6.0, 7.0], [4.0, 0.0, 0.0, 0.0]])
    assert len(res) == 3 and st.get_weights() == {"user": 4.0, "transition": 5.0, "popularity": 6.0, "distance": 7.0}     # the first of equal ones
    bp = BonusPrior(table)
    assert bp.tune(None, None, None, [[1.0], [2.5]])[1] == {"mrr": 2.5} and bp.get_weights() == {"bonus": 2.5}
