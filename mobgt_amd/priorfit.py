"""The weights of the priors (any prior.Prior, or a prior.Stack) fitted by maximum likelihood on held-out
samples, instead of a grid the caller has to invent (prior.tune).  Every prior is exactly linear in its weights,
blend(s, w) = s + sum_k w_k F_k with F_k the table value its rule adds (0 where the rule adds nothing), so the log-likelihood of
the targets under softmax(blend) is concave in w: its gradient is E_p[F] - F[y], its Hessian Cov_p[F], and a handful of Newton
passes finds the optimum.  The expensive part of a pass -- the softmax expectation of K features and their K (K + 1) / 2 products
over [G, V], for several candidate weight rows -- runs on the device (csrc_priorfit/fit.hip through _priorfit), inside
train.PriorFitLoop's captured graphs.

The rule (terms_host is it, in plain numpy; mobgt_priorfit_terms is checked against that).  One batch is

    base  [G, V] f32, or absent (then it counts as 0)          feats [K, G, V] f32
    y[g] integer targets and a target_offset                   W [L, K] f64 weight rows

Everything is converted to f64 when loaded and all arithmetic is f64.

  * z[l, g, c] = base[g, c] + W[l, 0] * feats[0, g, c] + ... + W[l, K - 1] * feats[K - 1, g, c], summed in this order, every
    product and every sum rounded on its own (no FMA).  This is the fit's own definition, deliberately not the f32 term-by-term
    bits of blend: the two differ by a few f32 ulps, which a fit does not see.
  * Row g COUNTS if its target column t = y[g] + target_offset is in [0, V), no z[l, g, :] of any l is NaN or +inf, no feature
    value of the row is non-finite, no z[l, g, :] is -inf throughout, and every z[l, g, t] is finite.  -inf in base is legal: a
    masked column of probability 0.  A row counts for every weight row or for none.  A row that breaks one of the finiteness
    conditions contributes zeros everywhere and ORs SNONFINITE into a sticky status word; a row whose target is out of range
    contributes zeros and raises no flag (a row that does both is flagged).
  * With p = softmax(z[l, g, :]) and mu_k = sum_c p_c F_kc, the terms of (l, g) are NT = 2 + K + K (K + 1) / 2 doubles:

        n      1 for a row that counts, else 0
        nll    logsumexp(z) - z[t]
        g_k    mu_k - F_k[t]                                      k in [0, K)
        H_kj   sum_c p_c F_kc F_jc - mu_k mu_j                    k <= j, row-major

The fit (fit_host on the host, fit with a model on the device; one Newton loop, newton(), serves both -- they differ only in who
supplies the terms summed over the samples).

  * Objective: J(w) = nll(w) / n + (l2 / 2) |w|^2 per counted sample; grad J = g / n + l2 w, hess J = H / n + l2 I.
  * Pass 0 evaluates one row, the starting weights: the prior's current ones, with 1 in front for the model's scale when
    scale_model is set.
  * Every later pass evaluates the 4 rows w + s d, s = 1, 1/2, 1/4, 1/8, with d = -(hess J)^-1 grad J at the current point, and
    moves to the row of lowest J: its gradient and Hessian came with it, so one pass is both line search and derivative.
  * It stops when max |grad J| <= tol, when no row lowers J (the fit is converged to rounding), or at max_passes.
  * Defaults: l2 = 1e-3, tol = 1e-7, max_passes = 12.

The model's scale.  With scale_model=True the model's own scores S are feature 0 and base is absent: z = w_0 S + sum w_k F_k.
A model trained with GradientTailLoss does not emit calibrated log-probabilities; w_0 relates its scale to the priors'.  The
weights written back to the prior are w_k / w_0, which rank exactly as the fitted blend does and leave the model's scores as
they are; with w_0 <= 0 nothing is written (FitResult.applied is False).  With scale_model=False base = S and the w_k are written
as fitted.  Weights are written through the prior's own set_weights, with its f32 and finiteness checks, so captured evaluation
graphs stay valid.

The samples must be held out of the sessions the priors' tables were fitted on -- on those the count features explain the
targets far too well -- and they are not the test split: the weights are fitted to them."""
import collections

import numpy as np
import torch

from . import _priorfit

SNONFINITE = _priorfit.SNONFINITE
MAX_K, MAX_L = _priorfit.MAX_K, _priorfit.MAX_L
STEPS = (1.0, 0.5, 0.25, 0.125)                                         # the rows of a pass after the first
SCALE = "scale"                                                         # the name of the model's weight w_0 in a fit

FitResult = collections.namedtuple("FitResult", "weights scale n nll_start nll grad passes converged applied history")
FitResult.__doc__ = """weights {name: w_k} as fitted (the coefficients of F_k in z); scale: w_0, 1.0 without scale_model -- what set_weights got
is w_k / scale; n: the samples that counted; nll_start, nll: mean negative log-likelihood at the starting and the fitted weights;
grad: max |grad J| at the fitted weights; passes: evaluations of the samples, pass 0 included; converged: grad <= tol or no row
lowered J; applied: the prior's weights were set; history: [(step, J)] per pass, step 0.0 for pass 0 and for a pass that moved nowhere"""


def nt_of(K):
    """NT, the doubles of one (l, g): n, nll, K gradient entries and the K (K + 1) / 2 entries of the Hessian's upper triangle."""
    return 2 + K + K * (K + 1) // 2


def terms_host(base, feats, y, target_offset, W):
    """The rule of the module's docstring -> (terms f64 [L, G, NT], status bits).  base [G, V] or None; feats [K, G, V]; y [G]
    integers; W [L, K]."""
    F = np.asarray(feats, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    if F.ndim != 3 or W.ndim != 2 or W.shape[1] != F.shape[0] or F.shape[0] < 1 or W.shape[0] < 1:
        raise ValueError(f"terms_host: feats [K, G, V] and W [L, K], got {F.shape} and {W.shape}")
    K, G, V = F.shape
    L = W.shape[0]
    b = np.zeros((G, V)) if base is None else np.asarray(base, dtype=np.float64)
    y = np.asarray(y).reshape(-1).astype(np.int64)
    if b.shape != (G, V) or y.shape != (G,):
        raise ValueError(f"terms_host: base {b.shape} and y {y.shape} for feats {F.shape}")
    t = y + int(target_offset)
    in_range = (t >= 0) & (t < V)
    tc = np.where(in_range, t, 0)
    rows = np.arange(G)
    with np.errstate(all="ignore"):
        z = np.empty((L, G, V))
        for l in range(L):
            acc = b.copy()
            for k in range(K):
                acc = acc + W[l, k] * F[k]
            z[l] = acc
        broken = np.zeros(G, dtype=bool)
        if V:
            broken |= (np.isnan(z) | (z == np.inf)).any(axis=(0, 2)) | ~np.isfinite(F).all(axis=(0, 2))
            broken |= (z == -np.inf).all(axis=2).any(axis=0)
            broken |= in_range & ~np.isfinite(z[:, rows, tc]).all(axis=0)
        counts = in_range & ~broken
        out = np.zeros((L, G, nt_of(K)))
        if not counts.any():
            return out, (SNONFINITE if broken.any() else 0)
        iu = np.triu_indices(K)
        Fc = np.where(counts[None, :, None], F, 0.0)                    # (rows that do not count: harmless numbers, zeroed below)
        for l in range(L):
            zz = np.where(counts[:, None], z[l], 0.0)
            m = zz.max(axis=1)
            e = np.exp(zz - m[:, None])                                 # (a masked column: exp(-inf) = 0)
            Z = e.sum(axis=1)
            p = e / Z[:, None]
            mu = np.einsum("kgv,gv->gk", Fc, p)
            second = np.einsum("kgv,jgv->gkj", Fc * p[None], Fc)
            cov = second - mu[:, :, None] * mu[:, None, :]
            out[l, :, 0] = 1.0
            out[l, :, 1] = (m + np.log(Z)) - zz[rows, tc]
            out[l, :, 2:2 + K] = mu - Fc[:, rows, tc].T
            out[l, :, 2 + K:] = cov[:, iu[0], iu[1]]
        out[:, ~counts, :] = 0.0
    return out, (SNONFINITE if broken.any() else 0)


def unpack(sums, l2, w):
    """Summed terms [NT] of one weight row w [K] -> (n, J, grad J [K], hess J [K, K]) of the module's objective."""
    K = len(w)
    n = float(sums[0])
    H = np.zeros((K, K))
    H[np.triu_indices(K)] = sums[2 + K:]
    H = H + np.triu(H, 1).T
    return n, sums[1] / n + 0.5 * l2 * float(w @ w), sums[2:2 + K] / n + l2 * w, H / n + l2 * np.eye(K)


def newton(evaluate, start, l2=1e-3, tol=1e-7, max_passes=12):
    """The Newton loop of the module's docstring.  evaluate(W [L, K] f64) -> the terms summed over every sample, f64 [L, NT]; it is
    called once per pass.  start [K].  -> (w [K], n, nll_start, nll, grad, passes, converged, history)."""
    w = np.array(start, dtype=np.float64).reshape(-1)
    if not (l2 >= 0.0 and tol >= 0.0 and max_passes >= 1) or not np.isfinite(w).all():
        raise ValueError(f"fit: l2 >= 0, tol >= 0, max_passes >= 1 and finite starting weights, got {l2}, {tol}, {max_passes}, {w.tolist()}")

    def look(W):
        sums = np.asarray(evaluate(W), dtype=np.float64)
        if sums.shape != (len(W), nt_of(len(w))):
            raise ValueError(f"fit: the terms of {len(W)} rows of {len(w)} weights are [{len(W)}, {nt_of(len(w))}], got {sums.shape}")
        if not sums[0, 0] > 0:
            raise ValueError("fit: no sample counts (every target is outside the scored columns)")
        return [unpack(s, l2, row) for s, row in zip(sums, W)]

    n, J, grad, hess = look(w[None, :])[0]
    nll_start = J - 0.5 * l2 * float(w @ w)
    history, passes, converged = [(0.0, float(J))], 1, False
    while True:
        if np.abs(grad).max() <= tol:
            converged = True
            break
        if passes >= max_passes:
            break
        d = -np.linalg.solve(hess, grad)
        W = np.stack([w + s * d for s in STEPS])
        rows = look(W)
        passes += 1
        best = min(range(len(STEPS)), key=lambda i: (rows[i][1], i))
        if not rows[best][1] < J:                                       # converged to rounding: no step lowers J
            history.append((0.0, float(J)))
            converged = True
            break
        w = W[best]
        n, J, grad, hess = rows[best]
        history.append((STEPS[best], float(J)))
    return w, int(round(n)), float(nll_start), float(J - 0.5 * l2 * float(w @ w)), float(np.abs(grad).max()), passes, converged, history


def _finish(prior, names, scale_model, solved):
    """newton()'s tuple -> FitResult, after writing the weights to `prior` (None: nothing to write)."""
    w, n, nll_start, nll, grad, passes, converged, history = solved
    scale = float(w[0]) if scale_model else 1.0
    fitted = dict(zip(names, (float(v) for v in (w[1:] if scale_model else w))))
    applied = False
    if prior is not None and scale > 0.0:
        prior.set_weights(**{k: v / scale for k, v in fitted.items()})
        applied = True
    return FitResult(fitted, scale, n, nll_start, nll, grad, passes, converged, applied, history)


def _start(prior, K, start, what):
    if start is None:
        start = [prior.get_weights()[k] for k in prior.WEIGHTS] if prior is not None else [0.0] * K
    start = np.asarray(start, dtype=np.float64).reshape(-1)
    if start.shape != (K,):
        raise ValueError(f"{what}: {K} starting weights, got {start.shape[0]}")
    return start


def fit_host(base, feats, y, target_offset=0, prior=None, names=None, start=None, l2=1e-3, tol=1e-7, max_passes=12, scale_model=False):
    """The fit of the module's docstring on the host, every pass one terms_host over all samples: the CPU form, and the use
    without a model.  base [G, V]: the model's scores (None: none; with scale_model they become feature 0 and must be given);
    feats [K, G, V]: the features, prior.features(rows, label_offset, out) of a prior on any device, downloaded; y [G] and
    target_offset as the loops give them (y, -model.label_offset).  prior: where the starting weights are read and the fitted
    ones written, its WEIGHTS the names; without one, names default to w0 .. and the start to zeros.  -> FitResult."""
    F = np.asarray(feats, dtype=np.float64)
    if F.ndim != 3 or F.shape[0] < 1:
        raise ValueError(f"fit_host: feats must be [K >= 1, G, V], got {F.shape}")
    K = F.shape[0]
    names = tuple(prior.WEIGHTS if prior is not None else names or (f"w{k}" for k in range(K)))
    if len(names) != K:
        raise ValueError(f"fit_host: {K} features and {len(names)} names ({', '.join(names)})")
    w0 = _start(prior, K, start, "fit_host")
    if scale_model:
        if base is None:
            raise ValueError("fit_host: scale_model=True scales the model's scores, and base is None")
        F = np.concatenate([np.asarray(base, dtype=np.float64)[None], F])
        base, w0 = None, np.r_[1.0, w0]

    def evaluate(W):
        terms, status = terms_host(base, F, y, target_offset, W)
        if status:
            raise ValueError(f"fit_host: scores or features that are not finite (status {status}): a row held NaN or +inf, a feature "
                             "that is not finite, nothing but -inf, or -inf at its target")
        return terms.sum(axis=1)
    return _finish(prior, names, scale_model, newton(evaluate, w0, l2, tol, max_passes))


def fit(prior, model, collator, val, l2=1e-3, tol=1e-7, max_passes=12, scale_model=True, **loop_kw):
    """The fit of the module's docstring with a model, on the device: one train.PriorFitLoop(model, collator, val, prior,
    scale_model=scale_model, **loop_kw), whose graphs are captured in pass 0 and replayed by every later pass with new weight
    rows.  Sets the prior's weights (see the module's docstring) and -> FitResult.  `val` must be held out of the sessions the
    prior's tables were fitted on, and is not the test split: the weights are fitted to it."""
    from .train import PriorFitLoop
    loop = PriorFitLoop(model, collator, val, prior, scale_model=scale_model, **loop_kw)

    def evaluate(W):
        loop.set_rows(W)
        return loop.run()
    return _finish(prior, prior.WEIGHTS, scale_model, newton(evaluate, loop.start, l2, tol, max_passes))


def work_bytes(K, G, V, L):
    """Bytes of the workspace terms() needs (mobgt_priorfit_work_bytes); sizes outside the limits: ValueError."""
    n = _priorfit.lib().mobgt_priorfit_work_bytes(int(K), int(G), int(V), int(L))
    if n < 0:
        raise ValueError(f"priorfit.work_bytes: K = {K}, G = {G}, V = {V}, L = {L} outside 1 .. {MAX_K} features, 1 .. {MAX_L} rows, "
                         f"0 .. {_priorfit.MAX_G} rows of scores, V < 2^31")
    return int(n)


def terms(base, feats, y, target_offset, W, V=None, work=None, out=None, status=None):
    """mobgt_priorfit_terms on the current stream: two launches, no allocation when work, out and status are given, no host read.

    base: f32 [G, >= V] with unit column stride, or None; feats: f32 [K, G, >= V] with unit column stride (any row and plane
    strides >= V); y: int32 / int64 [G] (or [G, 1]); W: f64 [L, K] contiguous, on the device; V: the scored columns (default
    feats.shape[2]).  work: uint8 of work_bytes(K, G, V, L); out: f64 [L, G, NT] contiguous; status: int32 [1], ORed into.
    -> out.  G = 0 or V = 0 launches nothing and leaves out as it is."""
    what = "priorfit.terms"
    if feats.dim() != 3 or feats.dtype != torch.float32 or (feats.shape[2] and feats.stride(2) != 1):
        raise ValueError(f"{what}: feats must be f32 [K, G, >= V] with unit column stride, got {feats.dtype} {tuple(feats.shape)}")
    K, G = feats.shape[:2]
    V = feats.shape[2] if V is None else int(V)
    if not 0 <= V <= feats.shape[2]:
        raise ValueError(f"{what}: V = {V} of {feats.shape[2]} columns")
    if base is not None and (base.dim() != 2 or base.dtype != torch.float32 or base.shape[0] != G or base.shape[1] < V
                             or (base.shape[1] and base.stride(1) != 1)):
        raise ValueError(f"{what}: base must be f32 [{G}, >= {V}] with unit column stride, got {base.dtype} {tuple(base.shape)}")
    y = y.reshape(-1)
    if y.dtype not in (torch.int32, torch.int64) or y.shape[0] != G:
        raise ValueError(f"{what}: y must be {G} int32 or int64 targets, got {y.dtype} {tuple(y.shape)}")
    if W.dim() != 2 or W.dtype != torch.float64 or W.shape[1] != K or not W.is_contiguous():
        raise ValueError(f"{what}: W must be a contiguous f64 [L, {K}], got {W.dtype} {tuple(W.shape)}")
    L = W.shape[0]
    if not (1 <= K <= MAX_K and 1 <= L <= MAX_L and G <= _priorfit.MAX_G):
        raise ValueError(f"{what}: K = {K}, L = {L}, G = {G}: one launch takes 1 .. {MAX_K} features, 1 .. {MAX_L} weight rows and "
                         f"up to {_priorfit.MAX_G} rows")
    dev = feats.device
    if dev.type != "cuda":
        raise ValueError(f"{what}: the launch runs on the GPU only (the host form is priorfit.terms_host)")
    NT = nt_of(K)
    need = work_bytes(K, G, V, L)
    with torch.cuda.device(dev):
        if work is None:
            work = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.zeros(L, G, NT, dtype=torch.float64, device=dev)
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
        if work.dtype != torch.uint8 or work.numel() < need or not work.is_contiguous():
            raise ValueError(f"{what}: work must be {need} contiguous bytes (priorfit.work_bytes), got {work.dtype} {tuple(work.shape)}")
        if out.dtype != torch.float64 or tuple(out.shape) != (L, G, NT) or not out.is_contiguous():
            raise ValueError(f"{what}: out must be a contiguous f64 [{L}, {G}, {NT}], got {out.dtype} {tuple(out.shape)}")
        if status.dtype != torch.int32 or status.numel() != 1:
            raise ValueError(f"{what}: status must be int32 [1], got {status.dtype} {tuple(status.shape)}")
        for name, v in (("base", base), ("y", y), ("W", W), ("work", work), ("out", out), ("status", status)):
            if v is not None and v.device != dev:
                raise ValueError(f"{what}: {name} is on {v.device}, feats on {dev}")
        from .ops import _p, _stream
        ld = lambda v, d: v.stride(d) if v.shape[d] > 1 else max(V, 1)   # (the stride of a dimension of one element means nothing)
        if min(ld(feats, 0), ld(feats, 1), ld(base, 0) if base is not None else V) < V:
            raise ValueError(f"{what}: rows and planes must lie at least V = {V} elements apart")
        _priorfit.launch("mobgt_priorfit_terms", _p(base), ld(base, 0) if base is not None else V, _p(feats), ld(feats, 1), ld(feats, 0),
                         K, G, V, _p(y), _priorfit.I64 if y.dtype == torch.int64 else _priorfit.I32, max(y.stride(0), 1) if G > 1 else 1,
                         int(target_offset), _p(W), L, _p(work), _p(out), _p(status), _stream())
    return out
