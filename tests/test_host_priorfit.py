"""The weight fit's rule on the host (mobgt_amd.priorfit: terms_host, the reference of the kernels in csrc_priorfit/fit.hip, and
fit_host, the Newton loop the device fit shares): the terms against brute-force central differences of their own nll, which rows
count and which raise SNONFINITE, a masked column, the fit on geoprior_cases.decay_log() against a grid and against weights 1 on
the other half of the held-out transitions, the write-back with the model's scale, the features of the priors, and the header."""
import itertools

import numpy as np
import pytest
import torch

import priorfit_cases as fc
from mobgt_amd import _priorfit, priorfit


# ------------------------------------------------------------------------------------------------ the terms
def test_the_terms_are_the_derivatives_of_their_own_nll():
    """G = 3, V = 7, K = 2.  Central differences with h = 1e-4 of an analytic function whose third derivatives are of order 1 are
    off by about h^2 = 1e-8 in truncation and 1e-16 / h = 1e-12 in rounding: the gate is 1e-6."""
    d = fc.batch(3, 7, 2, 1, seed=3)
    d["y"][2] = 4 - d["offset"]                                         # (all three rows count)
    base, feats = d["base"][:, :7], d["feats"][:, :, :7]
    w = d["W"][0]
    nll = lambda v: priorfit.terms_host(base, feats, d["y"], d["offset"], np.asarray(v)[None])[0][0, :, 1].sum()
    grad = lambda v: priorfit.terms_host(base, feats, d["y"], d["offset"], np.asarray(v)[None])[0][0, :, 2:4].sum(axis=0)
    terms, status = priorfit.terms_host(base, feats, d["y"], d["offset"], w[None])
    assert status == 0 and terms.shape == (1, 3, 7) and terms[0, :, 0].tolist() == [1.0, 1.0, 1.0]
    h = 1e-4
    e = np.eye(2) * h
    fd_grad = np.array([(nll(w + e[k]) - nll(w - e[k])) / (2 * h) for k in range(2)])
    fd_hess = np.array([(grad(w + e[k]) - grad(w - e[k])) / (2 * h) for k in range(2)])
    got = terms[0].sum(axis=0)
    assert np.abs(got[2:4] - fd_grad).max() <= 1e-6
    assert np.abs(np.array([[got[4], got[5]], [got[5], got[6]]]) - fd_hess).max() <= 1e-6
    # and nll is what it says: -log softmax(z)[t] by the textbook formula
    z = base.astype(np.float64) + w[0] * feats[0].astype(np.float64) + w[1] * feats[1].astype(np.float64)
    t = d["y"] + d["offset"]
    want = np.log(np.exp(z).sum(axis=1)) - z[np.arange(3), t]
    np.testing.assert_allclose(terms[0, :, 1], want, rtol=1e-12)
    # an absent base is a base of zeros
    a = priorfit.terms_host(None, feats, d["y"], d["offset"], d["W"])[0]
    b = priorfit.terms_host(np.zeros((3, 7), dtype=np.float32), feats, d["y"], d["offset"], d["W"])[0]
    assert np.array_equal(a, b)


def test_a_hessian_is_a_covariance():
    d = fc.batch(5, 33, 4, 3, seed=1)
    terms, _ = priorfit.terms_host(d["base"][:, :33], d["feats"][:, :, :33], d["y"], d["offset"], d["W"])
    for l, g in itertools.product(range(3), (0, 1, 3, 4)):
        n, _, _, H = priorfit.unpack(terms[l, g], 0.0, d["W"][l])
        assert n == 1.0 and np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() >= -1e-9 * np.abs(H).max()
    assert not terms[:, 2].any()                                        # row 2's target is out of range


@pytest.mark.parametrize("kind", fc.KINDS)
def test_a_row_that_breaks_a_finiteness_condition_is_left_out_and_flagged(kind):
    d, row = fc.broken(kind)
    V = d["V"]
    terms, status = priorfit.terms_host(d["base"][:, :V], d["feats"][:, :, :V], d["y"], d["offset"], d["W"])
    assert status == priorfit.SNONFINITE == 1
    assert not terms[:, row].any() and terms[:, [0, 2, 3], 0].tolist() == [[1.0] * 3] * 2
    keep = [0, 2, 3]
    alone, clean = priorfit.terms_host(d["base"][keep, :V], d["feats"][:, keep, :V], d["y"][keep], d["offset"], d["W"])
    assert clean == 0 and np.array_equal(alone, terms[:, keep])         # the other rows are what they are without it


def test_which_rows_count():
    d = fc.batch(4, 20, 2, 2, seed=0)
    base, feats = d["base"][:, :20], d["feats"][:, :, :20]
    terms, status = priorfit.terms_host(base, feats, d["y"], d["offset"], d["W"])
    assert status == 0 and terms[:, :, 0].tolist() == [[1.0, 1.0, 0.0, 1.0]] * 2 and not terms[:, 2].any()      # out of range: zeros, no flag
    for t in (-1, 20):
        y = d["y"].copy()
        y[3] = t - d["offset"]
        terms, status = priorfit.terms_host(base, feats, y, d["offset"], d["W"])
        assert status == 0 and terms[0, :, 0].tolist() == [1.0, 1.0, 0.0, 0.0]
    # a row breaks a condition under ONE weight row only: it is left out of every weight row
    f = feats.copy()
    f[0, 0, 5] = np.float32(3e38)
    W = np.array([[0.5, 0.5], [1e300, 0.5]])
    with np.errstate(over="ignore"):
        terms, status = priorfit.terms_host(base, f, d["y"], d["offset"], W)
    assert status == 1 and not terms[:, 0].any() and terms[:, 1, 0].tolist() == [1.0, 1.0]
    # out of range and broken: flagged
    b = base.copy()
    b[2, 0] = np.nan
    assert priorfit.terms_host(b, feats, d["y"], d["offset"], d["W"])[1] == 1
    # V = 0 and G = 0 are legal
    none, status = priorfit.terms_host(None, np.zeros((2, 3, 0)), [1, 2, 3], -1, d["W"])
    assert none.shape == (2, 3, 7) and not none.any() and status == 0
    none, status = priorfit.terms_host(None, np.zeros((2, 0, 4)), [], -1, d["W"])
    assert none.shape == (2, 0, 7) and status == 0
    with pytest.raises(ValueError, match=r"feats \[K, G, V\] and W \[L, K\]"):
        priorfit.terms_host(None, feats, d["y"], -1, np.zeros((2, 3)))


def test_a_masked_column_has_probability_zero():
    d = fc.batch(3, 12, 3, 2, seed=5)
    d["y"][2] = 7 - d["offset"]
    base, feats = d["base"][:, :12].copy(), d["feats"][:, :, :12].copy()
    base[:, 4] = -np.inf
    d["y"][d["y"] + d["offset"] == 4] = 5 - d["offset"]
    terms, status = priorfit.terms_host(base, feats, d["y"], d["offset"], d["W"])
    assert status == 0 and terms[:, :, 0].all()
    moved = feats.copy()
    moved[:, :, 4] = 1000.0                                             # what the column holds counts for nothing ...
    assert np.array_equal(priorfit.terms_host(base, moved, d["y"], d["offset"], d["W"])[0], terms)
    keep = [c for c in range(12) if c != 4]                             # ... and the rest is the problem without the column
    y = d["y"] - (d["y"] + d["offset"] > 4)
    without, _ = priorfit.terms_host(base[:, keep], feats[:, :, keep], y, d["offset"], d["W"])
    np.testing.assert_allclose(terms, without, rtol=1e-12, atol=1e-13)


# ------------------------------------------------------------------------------------------------ the fit
@pytest.fixture(scope="module")
def world():
    return fc.decay_world()


def _mean_nll(feats, y, w):
    terms, status = priorfit.terms_host(None, feats, y, -1, np.asarray(w, dtype=np.float64)[None])
    assert status == 0 and terms[0, :, 0].all()
    return float(terms[0, :, 1].mean())


def test_fit_host_on_the_decay_log(world):
    """All model scores zero, the stack's four features, the even held-out transitions to fit and the odd ones to check, the
    defaults l2 = 1e-3 (per sample), tol = 1e-7, max_passes = 12, Newton from w = 0.  Measured: 8 passes to max |grad J| =
    4.5e-12; weights (user, transition, popularity, distance) = (-0.3684, -0.0650, 1.0293, 0.8150); mean nll on the fitted half
    5.9915 at w = 0 and 2.3382 at the fit; on the other half 2.2124 at the fit against 3.0206 at weights 1; the smallest
    eigenvalue of hess J at the fit 0.1007."""
    feats, y = world["feats"], world["y"]
    assert feats.shape == (4, 500, 400) and np.isfinite(feats).all()
    fit_f, fit_y, chk_f, chk_y = feats[:, 0::2], y[0::2], feats[:, 1::2], y[1::2]
    res = priorfit.fit_host(None, fit_f, fit_y, target_offset=-1, names=world["stack"].WEIGHTS)
    w = np.array([res.weights[k] for k in world["stack"].WEIGHTS])
    assert res.converged and res.passes <= 12 and res.grad <= 1e-7 and res.n == 250 and res.scale == 1.0 and not res.applied
    assert len(res.history) == res.passes and res.history[0][0] == 0.0 and all(s in (1.0, 0.5, 0.25, 0.125) for s, _ in res.history[1:])
    assert all(b[1] < a[1] for a, b in zip(res.history, res.history[1:]))              # J falls at every pass
    assert res.nll_start == pytest.approx(np.log(400.0), rel=1e-12) and res.nll < res.nll_start
    J = lambda rows: priorfit.terms_host(None, fit_f, fit_y, -1, rows)[0][:, :, 1].mean(axis=1) + 0.5e-3 * (rows ** 2).sum(axis=1)
    grid = np.array(list(itertools.product((0.0, 1.0, 2.0), repeat=4)))
    at_fit = float(J(w[None])[0])
    assert at_fit == pytest.approx(res.history[-1][1], rel=1e-12) and (at_fit <= J(grid)).all()
    held_fit, held_ones = _mean_nll(chk_f, chk_y, w), _mean_nll(chk_f, chk_y, np.ones(4))
    terms = priorfit.terms_host(None, fit_f, fit_y, -1, w[None])[0].sum(axis=1)[0]
    lam = np.linalg.eigvalsh(priorfit.unpack(terms, 1e-3, w)[3]).min()
    print(f"passes {res.passes}, grad {res.grad:.3e}, weights {w.round(4).tolist()}, nll {res.nll_start:.4f} -> {res.nll:.4f}, "
          f"held-out nll {held_fit:.4f} (weights 1: {held_ones:.4f}), smallest eigenvalue {lam:.4f}")
    assert held_fit < held_ones
    # the stack is untouched without prior=; with it the start is the prior's weights and the fit is written
    st = world["stack"]
    assert st.get_weights() == dict(user=1.0, transition=1.0, popularity=1.0, distance=1.0)
    again = priorfit.fit_host(None, fit_f, fit_y, target_offset=-1, prior=st)
    assert again.applied and again.converged and again.history[0][1] == pytest.approx(float(J(np.ones((1, 4)))[0]), rel=1e-12)
    got = np.array([st.get_weights()[k] for k in st.WEIGHTS])
    assert np.abs(got - w).max() <= 1e-5 and np.array_equal(got, np.array([again.weights[k] for k in st.WEIGHTS], dtype=np.float32))
    # the features are the blend's terms: blend(0, w) = sum_k w_k F_k up to the f32 rounding of its four sums
    rows = (world["hist"][:50], world["user"][:50])
    blended = st.blend(torch.zeros(50, 400), rows, 1).numpy()
    np.testing.assert_allclose(blended, np.einsum("k,kgv->gv", got, feats[:, :50].astype(np.float64)), rtol=0, atol=4 * 2.0 ** -24 * np.abs(feats).max() * np.abs(got).sum())
    st.set_weights(user=1.0, transition=1.0, popularity=1.0, distance=1.0)


def test_the_models_scale_and_the_write_back(world):
    st, feats, y = world["stack"], world["feats"][:, 0::2], world["y"][0::2]
    rng = np.random.RandomState(4)
    scores = rng.standard_normal((250, 400)).astype(np.float32)
    scores[np.arange(250), y - 1] += 2.0                                # a model that knows something, on a scale of its own
    st.set_weights(user=0.5, transition=0.5, popularity=0.5, distance=0.5)
    res = priorfit.fit_host(scores, feats, y, target_offset=-1, prior=st, scale_model=True)
    assert res.converged and res.applied and res.scale > 0 and set(res.weights) == set(st.WEIGHTS)
    for k in st.WEIGHTS:
        assert st.get_weights()[k] == np.float32(res.weights[k] / res.scale)
    # as fitted: z = w_0 S + sum w_k F_k is the optimum of the five-feature problem
    five = priorfit.fit_host(None, np.concatenate([scores[None], feats]), y, target_offset=-1, start=[1.0, 0.5, 0.5, 0.5, 0.5])
    assert five.weights["w0"] == pytest.approx(res.scale, abs=1e-6) and five.weights["w4"] == pytest.approx(res.weights["distance"], abs=1e-6)
    # scale_model=False: the scores are the base, the weights are written as fitted
    st.set_weights(user=0.5, transition=0.5, popularity=0.5, distance=0.5)
    flat = priorfit.fit_host(scores, feats, y, target_offset=-1, prior=st, scale_model=False)
    assert flat.applied and flat.scale == 1.0 and st.get_weights()["distance"] == np.float32(flat.weights["distance"])
    # a model that ranks its targets last: w_0 <= 0, nothing is written
    st.set_weights(user=0.5, transition=0.25, popularity=0.125, distance=2.0)
    scores[np.arange(250), y - 1] -= 8.0
    neg = priorfit.fit_host(scores, feats, y, target_offset=-1, prior=st, scale_model=True)
    assert neg.scale <= 0 and not neg.applied and neg.converged
    assert st.get_weights() == dict(user=0.5, transition=0.25, popularity=0.125, distance=2.0)
    st.set_weights(user=1.0, transition=1.0, popularity=1.0, distance=1.0)
    with pytest.raises(ValueError, match="scale_model=True scales the model's scores, and base is None"):
        priorfit.fit_host(None, feats, y, target_offset=-1, scale_model=True)
    with pytest.raises(ValueError, match=r"not finite \(status 1\)"):
        priorfit.fit_host(np.full((250, 400), np.nan, dtype=np.float32), feats, y, target_offset=-1)
    with pytest.raises(ValueError, match="no sample counts"):
        priorfit.fit_host(None, feats, np.zeros(250, dtype=np.int64), target_offset=-1)


def test_the_priors_have_the_methods():
    from mobgt_amd import geoprior, prior
    for cls in (prior.MarkovPrior, geoprior.DistancePrior, prior.Stack):
        assert callable(cls.features) and callable(cls.fit_weights)
        doc = " ".join(cls.fit_weights.__doc__.split())
        assert "must be held out of the sessions" in doc and "not the test split" in doc


def test_the_header_is_readable_without_the_built_library():
    sig = _priorfit.SIGNATURES
    assert list(sig) == ["mobgt_priorfit_abi_version", "mobgt_priorfit_nt", "mobgt_priorfit_work_bytes", "mobgt_priorfit_terms"]
    assert _priorfit.ABI_VERSION == 1 and [len(sig[k][1]) for k in list(sig)[1:]] == [1, 4, 18]
    assert (_priorfit.EBADDIM, _priorfit.EALIGN, _priorfit.EDTYPE, _priorfit.SNONFINITE, _priorfit.I32, _priorfit.I64) == (-1, -2, -3, 1, 0, 1)
    assert (_priorfit.MAX_K, _priorfit.MAX_L, _priorfit.MAX_G) == (8, 16, 65535) == (priorfit.MAX_K, priorfit.MAX_L, 65535)
    assert _priorfit.MAX_NT == priorfit.nt_of(_priorfit.MAX_K) == 46 and _priorfit.MAX_NT - 1 <= _priorfit.WAVE == 64
    assert _priorfit.CHUNK == _priorfit.THREADS * _priorfit.COLS and _priorfit.COLS * 4 == 16 and _priorfit.THREADS % _priorfit.WAVE == 0
    from mobgt_amd import _baseline, _geoprior, _native, _prior
    others = set(_prior.SIGNATURES) | set(_geoprior.SIGNATURES) | set(_baseline.SIGNATURES)
    for lib in _native.LIBRARIES:
        others |= set(lib.SIGNATURES)
    assert not set(sig) & others and "_priorfit" not in _native._MODULES and len(_native._MODULES) == 5
