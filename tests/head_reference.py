"""A float64 restatement of what the classifier head and the two loss kernels compute (csrc/skinny.hip's training section;
gtl_kernel and cross_entropy_kernel of csrc/layer.hip), the case builders of tests/test_gpu_head_matrix.py and the verdicts.

Products (nn.Linear on G <= 16 rows, model_fqandtoyo.py:1394, and its backward):
    y = x w^T + b [G,V]      dx = dy w [G,K]      dW = dy^T x [V,K]      db = column sums of dy [V]
GradientTailLoss (model_fqandtoyo.py:545-550, beta = k = 1), p = sigmoid(z), one_hot[g][c] = (class of row g == c):
    loss = mean( -alpha (1 - p) one_hot log p - (1 - one_hot) p log(1 - p) );  a class < 0 or >= V matches no column: all negatives
Cross entropy (F.cross_entropy(ignore_index), mean): over the rows with target != ignore_index; a target outside [0, V) is
counted in that divisor but adds nothing to the sum and has a zero gradient row (include/mobgt_hip.h).

Two input families.  EXACT: integers in [-3, 3], so every product and partial sum is an integer below 2^24 (|y| <= 9 K + 3,
|dx| <= 9 V, |dW|, |db| <= 9 G) and every form must return the reference's bits whatever its split, slice, wave or atomic order.
ROUNDING: real operands whose logits satisfy |z| <= 8 in float64 (the bias is drawn after the products are scaled), checked
within (n + 8) 2^-24 sum |a||b| per element, n the dot length: (n - 1) u covers any summation order of n products in f32, the rest
the bias add and the cross-slice atomics.  Loss and dlogits: the project's gate 2e-5 max |ref|, the loss with the fixed-point term of
the header on top; each is also compared with the distance of an f32 restatement of the same formulas from float64."""
import numpy as np

U = 2.0 ** -24
GATE = 2e-5
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ the operations, float64
def products(x, w, b, dy):
    x, w, dy = x.astype(F64), w.astype(F64), dy.astype(F64)
    return dict(y=x @ w.T + (b.astype(F64) if b is not None else 0.0), dx=dy @ w, dW=dy.T @ x, db=dy.sum(0))


def product_bounds(x, w, b, dy):
    ax, aw, ady = np.abs(x.astype(F64)), np.abs(w.astype(F64)), np.abs(dy.astype(F64))
    G, K = x.shape
    V = w.shape[0]
    return dict(y=(K + 8) * U * (ax @ aw.T + (np.abs(b.astype(F64)) if b is not None else 0.0)), dx=(V + 8) * U * (ady @ aw),
                dW=(G + 8) * U * (ady.T @ ax), db=(G + 8) * U * ady.sum(0))


def one_hot(cls, G, V):
    oh = np.zeros((G, V), dtype=bool)
    ok = (cls >= 0) & (cls < V)
    oh[np.nonzero(ok)[0], cls[ok]] = True
    return oh


def gtl(z, targets, target_offset, alpha, dt=F64, defect=None):
    """(loss, d loss / d z) in precision `dt` -- float64: the reference; float32: the same formulas as the kernels evaluate them
    (p = 1 / (1 + exp(-z)), q = 1 - p, log p, log q), which is also the emulation the planted defects go into."""
    z = z.astype(dt)
    G, V = z.shape
    cls = np.asarray(targets, dtype=np.int64)[:G] + (0 if defect == "target_offset ignored" else int(target_offset))
    oh = one_hot(cls, G, V)
    a, one = dt(alpha), dt(1)
    p = one / (one + np.exp(-z))
    q = one - p
    with np.errstate(divide="ignore", invalid="ignore"):
        lp, lq = np.log(p), np.log(q)
        an = a if defect == "alpha on the negative branch" else one
        el = np.where(oh, -a * q * lp, -an * p * lq)
        d = np.where(oh, a * p * q * lp - a * q * q, an * (-p * q * lq + p * p))
    n = dt(V if defect == "inv_n over V only" else G * V)
    return dt(el.sum(dtype=dt) / n), (d / n).astype(dt)


def cross_entropy(z, targets, ignore_index, dt=F64, defect=None):
    z = z.astype(dt)
    G, V = z.shape
    t = np.asarray(targets, dtype=np.int64)
    counted = t != ignore_index
    live = counted & (t >= 0) & (t < V)
    n = {None: counted.sum(), "live-row count omits out-of-range rows": live.sum(), "live-row count omits no row": G}[defect]
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True, dtype=dt)
    tc = np.clip(t, 0, V - 1)
    nll = (m + np.log(s))[:, 0] - z[np.arange(G), tc]
    if n == 0:
        return dt(np.nan), np.zeros((G, V), dt)
    oh = one_hot(np.where(live, t, -1), G, V)
    return dt(nll[live].sum(dtype=dt) / dt(n)), ((e / s - oh) * live[:, None] / dt(n)).astype(dt)


def gtl_blocks(V):
    """Workgroups of mobgt_skinny_linear_gtl (32 columns each, at most 1024)."""
    return min(1024, (V + 31) // 32)


def gtl_fixed_point(G, V):
    """The header's absolute resolution of the fused loss: one 2^-24 per workgroup and per cell, over G V."""
    return (gtl_blocks(V) + 9) * U / (G * V)


def dx_slices(V):
    return 32 if V >= 32768 else 8


# ------------------------------------------------------------------------------------------------ case builders
def targets_for(G, V, target_offset):
    """targets [G] int64 whose classes (targets + target_offset) are, row by row: column 0, -1 (no column; with target_offset
    = -1 this is the padding y = 0), column V - 1, V + 2 (no column), a middle column -- so a 16-column tile that holds a class
    has both branches in it."""
    pattern = [0, -1, V - 1, V + 2, V // 2]
    cls = np.array([pattern[g % 5] for g in range(G)], dtype=np.int64)
    return cls - target_offset


def build_case(G, K, V, family, bias=True, seed=0):
    rng = np.random.default_rng(1000003 * G + 1009 * K + V + 7 * seed + (family == "round"))
    if family == "exact":
        x, w, b, dy = (rng.integers(-3, 4, size=s).astype(F32) for s in ((G, K), (V, K), (V,), (G, V)))
    else:
        x, w = rng.standard_normal((G, K)).astype(F32), rng.standard_normal((V, K)).astype(F32)
        z0 = np.abs(x.astype(F64) @ w.astype(F64).T).max()
        w = (w * (3.9 / max(z0, 1e-30))).astype(F32)                # |x w^T| <= 3.9 (1 + 2^-24) in float64
        b = rng.uniform(-3.9, 3.9, size=V).astype(F32)
        dy = rng.standard_normal((G, V)).astype(F32)
    b = b if bias else None
    case = dict(G=G, K=K, V=V, family=family, x=x, w=w, b=b, dy=dy, ref=products(x, w, b, dy))
    if family == "round":
        case["bound"] = product_bounds(x, w, b, dy)
    check_case(case)
    return case


def check_case(case):
    """The builders' own conditions: the exact family's integers stay below 2^24, the rounding family's logits within 8."""
    G, K, V, ref = case["G"], case["K"], case["V"], case["ref"]
    if case["family"] == "exact":
        assert 9 * K + 3 < 2 ** 24 and 9 * V < 2 ** 24 and 9 * G < 2 ** 24
        for k in ("x", "w", "b", "dy"):
            t = case[k]
            assert t is None or (np.array_equal(t, np.round(t)) and np.abs(t).max() <= 3)
        for k, lim in (("y", 9 * K + 3), ("dx", 9 * V), ("dW", 9 * G), ("db", 3 * G)):
            assert np.abs(ref[k]).max() <= lim and np.array_equal(ref[k], np.round(ref[k]))
    else:
        assert np.abs(ref["y"]).max() <= 8.0 and np.isfinite(ref["y"]).all()


# ------------------------------------------------------------------------------------------------ verdicts
def exact_verdict(got, ref):
    """Bit for bit (the reference's values are integers below 2^24: float32 holds them exactly)."""
    got = np.asarray(got)
    return got.shape == ref.shape and bool(np.array_equal(got.astype(F64), ref))


def round_verdict(got, ref, bound):
    """(within the bound everywhere, worst error / bound); an element whose bound is 0 must be exact."""
    got = np.asarray(got)
    if got.shape != ref.shape:
        return False, float("inf")
    err = np.abs(got.astype(F64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    ratio = float(r.max()) if r.size else 0.0
    return bool(ratio <= 1.0), ratio


def product_verdict(case, name, got):
    if case["family"] == "exact":
        return exact_verdict(got, case["ref"][name]), 0.0
    return round_verdict(got, case["ref"][name], case["bound"][name])


def loss_verdict(loss, dz, ref_loss, ref_dz, fixed_abs=0.0):
    """(ok, |loss error|, max |dlogits error|) under the gate 2e-5 max |ref| (+ the loss's absolute fixed-point term)."""
    e_loss = abs(float(loss) - float(ref_loss))
    e_dz = float(np.abs(np.asarray(dz).astype(F64) - ref_dz).max())
    ok = e_loss <= GATE * abs(float(ref_loss)) + fixed_abs and e_dz <= GATE * float(np.abs(ref_dz).max())
    return bool(ok), e_loss, e_dz            # (a nan compares false)


def f32_ratio(err, err32, scale):
    """A kernel's error as a multiple of the f32 restatement's (floored at one 2^-24 of scale, where the restatement is exact)."""
    floor = max(err32, U * scale)
    return err / floor if floor > 0 else (0.0 if err == 0 else float("inf"))


# ------------------------------------------------------------------------------------------------ an emulation with planted defects
SENT = -12345.0
PRODUCT_DEFECTS = ("dropped last column tile", "dropped V-slice of dx", "doubled V-slice of dx", "db over the wrong axis", "bias added twice")
GTL_DEFECTS = ("target_offset ignored", "alpha on the negative branch", "inv_n over V only")
CE_DEFECTS = ("live-row count omits out-of-range rows", "live-row count omits no row")


def emulate_products(case, defect=None):
    """The four products in float32 the way the kernels lay them out: y by 16-column tiles, dx as the sum of dx_slices(V) slices
    of vper = (ceil(V / slices) + 3) & ~3 rows, into destinations that start as the GPU test's do."""
    x, w, b, dy, G, K, V = (case[k] for k in ("x", "w", "b", "dy", "G", "K", "V"))
    y = np.full((G, V), SENT, F32)
    tiles = (V + 15) // 16
    for t in range(tiles - (defect == "dropped last column tile")):
        c = slice(16 * t, min(V, 16 * t + 16))
        y[:, c] = x @ w[c].T + (0 if b is None else b[c] * F32(2 if defect == "bias added twice" else 1))
    dx = np.zeros((G, K), F32)
    ns = dx_slices(V)
    vper = ((V + ns - 1) // ns + 3) & ~3
    for s in range(ns):
        r = slice(s * vper, min(V, (s + 1) * vper))
        if r.start >= V or (s == 1 and defect == "dropped V-slice of dx"):
            continue
        dx += (dy[:, r] @ w[r]) * F32(2 if (s == 1 and defect == "doubled V-slice of dx") else 1)
    db = dy.sum(0, dtype=F32)
    if defect == "db over the wrong axis":
        db = dy.sum(1, dtype=F32)[np.arange(V) % G]
    return dict(y=y, dx=dx, dW=dy.T @ x, db=db)


# ------------------------------------------------------------------------------------------------ the GPU matrix's shapes
# (G, K, V): every G of {1, 3, 4, 5, 15, 16}, every K of {4, 16, 48, 64, ..., 508, 512} and every V of {1, 3, ..., 32769} at least
# once -- each runs with both families --, every KT = K / 64 of fwd_mfma / gtl at a V below 256 and at V = 32769 (1024
# workgroups whose first waves walk a second tile), the dx-MFMA slice counts on both sides of V = 32768.
PRODUCT_SHAPES = [
    (16, 64, 1), (3, 64, 32769), (1, 128, 3), (16, 128, 32769), (4, 192, 5), (5, 192, 32769), (5, 256, 15), (15, 256, 32769),
    (15, 320, 16), (1, 320, 32769), (16, 384, 17), (4, 384, 32769), (3, 448, 31), (16, 448, 32769),
    (16, 4, 32), (1, 16, 33), (4, 48, 255), (5, 252, 256), (15, 260, 257), (3, 508, 513), (16, 512, 1030),
    (16, 448, 2047), (5, 64, 2048), (3, 16, 2049), (4, 512, 4097), (16, 320, 32767), (16, 320, 32768), (15, 512, 32768),
]
# fused loss: workgroup counts 1, 2, 7, 8, 9, 1024 (no second tile) and 1024 (second tile); every KT once more
GTL_SHAPES = [(16, 64, 1), (3, 128, 33), (5, 192, 200), (16, 256, 256), (4, 320, 257), (15, 384, 32768), (16, 448, 32769)]
CE_SHAPES = [(1, 1), (3, 2), (16, 255), (257, 256), (4095, 257), (3, 1000), (257, 1000), (16, 10239), (1, 10240), (257, 10240)]


def forms_for(K):
    """The entries whose documented conditions accept K (all take G <= 16, K <= 512, K % 4 == 0)."""
    f = ["fwd", "bwd"]
    if K % 16 == 0:
        f += ["dx", "bwd_both"]
    if K % 64 == 0 and K <= 448:
        f += ["fwd_mfma", "gtl"]
    return f
