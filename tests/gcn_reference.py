"""Reference side of the one-launch GCN / CSR SpMM matrix (tests/test_gpu_gcn_matrix.py, tests/test_host_gcn_reference.py): the
case list as plain data, a case builder for two input families, a float64 restatement of the contracts of include/mobgt_hip.h that
csrc/smallgcn.hip (mobgt_small_gcn_fwd / _fwd_pack / _bwd) and csrc/spmm.hip (mobgt_spmm_csr / _t_rows / _t_rows_gather)
implement, the defects the verdicts must reject, and the rounding family's per-element tolerance.  NumPy only; the dropout keep
mask is the host replay of the bias-act site's hash (ops.dropout_site_mask(seed + seed_dev, salt, n, 64, p)).

Exact family.  AX has three entries of +-1 per row, A at most four entries per row from {1, 1/2}, weights are in {-1, 0, 1},
biases integers in [-2, 2], g in {-1, 0, 1}, the gradient buffers start as small integers, the slope is 1/2 and p = 0.5 (inv_keep
exactly 2); the SpMM operands are small integers with values from {1, 1/2, -1, 2}.  Every stage's outputs are then multiples of a
dyadic unit (STAGE_UNIT), and the builder asserts for every output of every product that the sum of the magnitudes of its terms,
in that unit, stays below 2^24: full-f32 MFMA products, fmaf chains and f32 atomics are exact in any order, and the device must
return the float64 result bit for bit (+0 and -0 compare equal).

Rounding family.  Real operands, A row-normalised, slope 0.2, p = 0.1 (or no dropout).  Tolerance, per element, with u = 2^-24
and gamma(m) = m u / (1 - m u) (the forward error of m f32 roundings on one path, any order):
    tile_product    (K-deep, chunks of KC = 304): m = sum over the chunks of (kc rounded up to 16) + 4 wave partials per chunk;
                    an operand error d propagates as |L| d:   err <= |L| d + gamma(m) |L| (|R| + d)
    mfma_tile<J>    (the little products t W1, t2 W2, g W2^T, du W1^T): m = J, + 1 where a bias is added
    pointwise       every further f32 multiply (slope, inv_keep, keep * m(h)) adds u (|value| + d); LeakyReLU has Lipschitz
                    constant 1; a dropped element is exactly 0
    gradients       16 rows per workgroup on the matrix core, then one f32 atomic per workgroup onto what the buffer held:
                    m = 16 + ceil(n / 16), over sum |terms| + |initial value|
    spmm            a chain of deg fmafs (narrow kernels: + log2(lane groups) shuffle adds + the bias add): m = deg + 4;
                    t_rows: one rounded product and one atomic per term: m = terms + 1 over sum |terms| + |initial value|
The forward's saved activations are judged twice: each against its stage function applied to the DEVICE's previous stage (one
stage's bound), and `out` end to end against float64 with the propagated bound.  The bounds are derived from the code, not tuned
on device output."""
import zlib

import numpy as np

import maskgemm_reference as mr
from maskgemm_reference import U, cdiv, gamma, inv_keep, leaky

KC, RB = 304, 16                                        # csrc/smallgcn.hip: k-chunk of a staged product, rows per workgroup
H1, H2, H3 = 16, 64, 32
WIDTHS = (H1, H2, H3)
SEED, SEED_DEV, SALT = 0x51F15EED1234, 77, 0x2000 + H3

# (n, K0, also in the rounding family)
GCN_CASES = ((1, 1, False), (15, 5, False), (16, 16, False), (17, 303, True), (304, 304, True), (300, 300, True), (305, 40, True),
             (320, 305, False), (609, 320, True), (300, 400, True), (37, 609, False), (1024, 64, False))
PACK_CASES = ((305, 40), (300, 400))
DROPS = (0, 1, 2)                                       # off | on, seed_dev null | on, seed_dev given
CSR_C = (4, 60, 64, 128, 132, 256, 260, 516)
CSR_DEGS = (0, 1, 3, 4, 5, 12, 13, 15, 16, 17, 33)
CSR_ROWS, CSR_COLS = 23, 41
ROWS_KINDS = ("null", "subset", "repeat")
GATHER_C = (4, 128, 256, 260, 512)
GATHER_DEGS = (0, 1, 63, 64, 65, 130)
GATHER_P, GATHER_R = 135, 21

GCN_MUTANTS = ("stale_L_after_layer1", "drop_chunk_tail", "drop_wave", "clamp_last_row", "a_for_at", "hash_without_salt",
               "slope_for_dropped", "overwrite", "b2_missing")
SPMM_MUTANTS = ("drop_unroll_tail", "drop_lane_group", "repeat_once", "bias_every_group", "second_float4_dropped", "head_threaded",
                "overwrite")


def S(entry, family, name, **kw):
    return dict(kw, entry=entry, family=family, id=f"{entry}-{family}-{name}")


def matrix_specs():
    specs = []
    for fam in ("exact", "round"):
        for n, K0, both in GCN_CASES:
            if fam == "round" and not both:
                continue
            for entry in ("fwd", "bwd"):
                for d in DROPS:
                    specs.append(S(entry, fam, f"n{n}-K{K0}-d{d}", n=n, K0=K0, drop=d))
        k = 0
        for C in CSR_C:
            for rk in ROWS_KINDS:
                for entry in ("csr", "t_rows"):
                    specs.append(S(entry, fam, f"C{C}-{rk}-o{k % 4}", C=C, rows=rk, bias=bool(k & 1), wide=bool(k & 2)))
                k += 1
        for C in GATHER_C:
            for wide in (False, True):
                specs.append(S("gather", fam, f"C{C}-w{int(wide)}", C=C, wide=wide, R=GATHER_R))
        for wide in (False, True):
            specs.append(S("gather", fam, f"C128-R0-w{int(wide)}", C=128, wide=wide, R=0))
    check_coverage(specs)
    return specs


def chunks(K):
    """[(k0, kc, kcp)] of tile_product's loop over K."""
    return [(k0, min(KC, K - k0), (min(KC, K - k0) + 15) & ~15) for k0 in range(0, K, KC)]


def kterms(K):
    return sum(kcp for _, _, kcp in chunks(K)) + 4 * len(chunks(K))


def fwd_form(n, K0):
    """Which staging the forward takes: "early" (both operands of layer 1 and the rows of A in the first burst), "restage" (layer 1
    streams AX through the L area, the rows of A are staged after it) or "stream" (n > KC: every product stages its own chunks)."""
    if n <= KC and K0 <= KC:
        return "early"
    return "restage" if n <= KC else "stream"


def check_coverage(specs):
    for fam in ("exact", "round"):
        of = lambda *e: [s for s in specs if s["entry"] in e and s["family"] == fam]          # noqa: E731
        g = of("fwd", "bwd")
        shapes = {(s["n"], s["K0"]) for s in g}
        assert shapes == {(n, k) for n, k, both in GCN_CASES if both or fam == "exact"}
        assert {fwd_form(*x) for x in shapes} == {"early", "restage", "stream"}
        assert {len(chunks(n)) for n, _ in shapes} >= {1, 2, 3} and {len(chunks(k)) for _, k in shapes} >= {1, 2}
        assert any(n % RB for n, _ in shapes) and any(n % RB == 0 for n, _ in shapes)
        for x in shapes:
            assert {(s["entry"], s["drop"]) for s in g if (s["n"], s["K0"]) == x} == {(e, d) for e in ("fwd", "bwd") for d in DROPS}
        assert max(cdiv(n, RB) for n, _ in shapes) <= 64
        for e in ("csr", "t_rows"):
            c = of(e)
            assert {(s["C"], s["rows"]) for s in c} == {(C, r) for C in CSR_C for r in ROWS_KINDS}
            for C in CSR_C:
                assert {s["bias"] for s in c if s["C"] == C} == {False, True}
            assert {(s["bias"], s["wide"]) for s in c} == {(a, b) for a in (False, True) for b in (False, True)}
        ga = of("gather")
        assert {s["C"] for s in ga} == set(GATHER_C) and {(s["R"], s["wide"]) for s in ga} == {(r, w) for r in (0, GATHER_R) for w in (False, True)}
    assert CSR_ROWS % 4 and GATHER_P % 4 and set(CSR_DEGS) >= {0, 1, 3, 4, 5, 12, 13, 15, 16, 17, 33}


# ------------------------------------------------------------------------------------------------ case builder
def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def family_consts(family):
    exact = family == "exact"
    slope, p = (0.5, 0.5) if exact else (0.2, 0.1)
    return exact, slope, p, inv_keep(p)


_GCN = {}


def gcn_inputs(family, n, K0):
    """The operands of an (n, K0) network, shared by its forward and backward specs (built once, never modified)."""
    key = (family, n, K0)
    if key in _GCN:
        return _GCN[key]
    rng = _rng("gcn", *key)
    exact, slope, p, ik = family_consts(family)
    f = np.float32
    if exact:
        ax = np.zeros((n, K0), dtype=f)
        a = np.zeros((n, n), dtype=f)
        for r in range(n):
            ax[r, rng.choice(K0, min(3, K0), replace=False)] = rng.choice(f([-1, 1]), min(3, K0))
            cols = rng.choice(n, rng.integers(1, min(4, n) + 1), replace=False)
            if r == 0:
                cols[0] = n - 1
            if r == n - 1:
                cols[0] = 0
            a[r, cols] = rng.choice(f([1, 0.5]), cols.size)
        a[n - 1, n - 1] = 0.5                          # (row n - 1 has at most four entries: column 0, this one, two others)
        if np.count_nonzero(a[n - 1]) > 4:
            a[n - 1, np.flatnonzero(a[n - 1, 1:n - 1])[0] + 1] = 0
        ints = lambda lim, *shape: rng.integers(-lim, lim + 1, shape).astype(f)            # noqa: E731
        w0, b0, w1, b1, w2, b2 = ints(1, K0, H1), ints(2, H1), ints(1, H1, H2), ints(2, H2), ints(1, H2, H3), ints(2, H3)
        g = ints(1, n, H3)
    else:
        m = (rng.random((n, n)) < min(1.0, 8.0 / n)) | np.eye(n, dtype=bool)
        a64 = m * rng.uniform(0.2, 1.0, (n, n))
        a = (a64 / a64.sum(1, keepdims=True)).astype(f)
        ax = (a.astype(np.float64) @ rng.uniform(0, 1, (n, K0))).astype(f)
        nrm = lambda s, *shape: (rng.standard_normal(shape) * s).astype(f)                 # noqa: E731
        w0, b0, w1, b1, w2, b2 = nrm(0.3, K0, H1), nrm(0.1, H1), nrm(0.3, H1, H2), nrm(0.1, H2), nrm(0.3, H2, H3), nrm(0.1, H3)
        g = nrm(1.0, n, H3)
    init = {k: rng.integers(-3, 4, s).astype(f) for k, s in (("dw0", (K0, H1)), ("db0", (H1,)), ("dw1", (H1, H2)), ("db1", (H2,)),
                                                             ("dw2", (H2, H3)), ("db2", (H3,)))}
    c = dict(family=family, n=n, K0=K0, exact=exact, slope=slope, p=p, inv_keep=ik, ax=ax, a=a, a_t=np.ascontiguousarray(a.T),
             ws=(w0, b0, w1, b1, w2, b2), g=g, init=init, seed=SEED + n, salt=SALT, _v={})
    if exact:
        for d in DROPS:
            assert_exact_gcn(c, d)
        v = variant(c, 1)
        if n >= 15:
            assert (v["fwd"]["h1"][0] == 0).any() and (~v["keep"]).any() and ((v["fwd"]["h2"][0] != 0) & v["keep"]).any()
    _GCN[key] = c
    return c


def variant(c, drop, mut=None):
    """A drop variant of a network: the keep mask, the float64 forward (name -> (ref, propagated bound)), the saved activations as
    the f32 arrays the backward is handed, and the float64 backward.  Cached for mut = None."""
    if mut is None and drop in c["_v"]:
        return c["_v"][drop]
    seed_dev = SEED_DEV if drop == 2 else None
    keep = None
    if drop:
        salt = 0 if mut == "hash_without_salt" else c["salt"]
        keep = mr.keep_mask(c["seed"] + (seed_dev or 0), salt, c["n"], H2, c["p"])
    v = dict(drop=drop, seed_dev=seed_dev, keep=keep, p=c["p"] if drop else 0.0, ik=c["inv_keep"] if drop else 1.0)
    v["fwd"] = forward(c, v, mut)
    clean = v if mut is None else variant(c, drop)
    v["saved"] = {k: clean["fwd"][k][0].astype(np.float32) for k in ("h1", "t", "h2", "t2")}
    v["bwd"] = backward(c, v, clean["keep"], mut)
    if mut is None:
        c["_v"][drop] = v
    return v


def build_case(spec):
    """The inputs and references of a spec.  The exact family's exactness condition is asserted here."""
    e = spec["entry"]
    if e in ("fwd", "bwd"):
        c = gcn_inputs(spec["family"], spec["n"], spec["K0"])
        return dict(spec=spec, net=c, v=variant(c, spec["drop"]))
    return _build_spmm(spec)


# ------------------------------------------------------------------------------------------------ the network, restated
def _product(L, R, mut, stale=None):
    """L [rows, K] times R [K, C] as tile_product computes it; (value, the L actually used)."""
    K = L.shape[1]
    L = L.astype(np.float64)
    if stale is not None:
        L = stale
    k0, kc, kcp = chunks(K)[-1]
    if mut == "drop_chunk_tail":
        L = L.copy()
        L[:, k0 + 16 * ((kc - 1) // 16):] = 0
    elif mut == "drop_wave":
        per = kcp // 4
        w = 1 if kc > per else 0
        L = L.copy()
        L[:, k0 + w * per:k0 + (w + 1) * per] = 0
    return L @ R, L


def _stale_rows(c):
    """What the L area holds after layer 1 streamed AX through it (n <= KC < K0): the last chunk of AX, zero up to its padded
    width, the chunk before it beyond -- read as this workgroup's rows of A."""
    ax, n = c["ax"].astype(np.float64), c["n"]
    lc = np.zeros((n, KC))
    for k0, kc, kcp in chunks(c["K0"]):
        lc[:, :kcp] = 0
        lc[:, :kc] = ax[:, k0:k0 + kc]
    return lc[:, :n]


def s_h1(c, mut=None):
    ax, w0, b0 = c["ax"].astype(np.float64), c["ws"][0].astype(np.float64), c["ws"][1].astype(np.float64)
    acc, L = _product(ax, w0, mut)
    pre = acc + b0
    d = gamma(kterms(c["K0"]) + 1) * (np.abs(L) @ np.abs(w0) + np.abs(b0))
    return leaky(pre, c["slope"]), d + U * (np.abs(pre) + d)


def s_adj(c, h, dh, mut=None):
    """t = A h1 and t2 = A h2."""
    stale = _stale_rows(c) if mut == "stale_L_after_layer1" and fwd_form(c["n"], c["K0"]) == "restage" else None
    acc, L = _product(c["a"], h, mut, stale)
    return acc, np.abs(L) @ dh + gamma(kterms(c["n"])) * (np.abs(L) @ (np.abs(h) + dh))


def s_h2(c, v, t, dt):
    w1, b1 = c["ws"][2].astype(np.float64), c["ws"][3].astype(np.float64)
    pre = t @ w1 + b1
    d = dt @ np.abs(w1) + gamma(H1 + 1) * ((np.abs(t) + dt) @ np.abs(w1) + np.abs(b1))
    y = leaky(pre, c["slope"])
    d = d + U * (np.abs(pre) + d)
    if v["keep"] is not None:
        d = np.where(v["keep"], (d + U * (np.abs(y) + d)) * v["ik"], 0.0)
        y = np.where(v["keep"], y * v["ik"], 0.0)
    return y, d


def s_out(c, t2, dt2, mut=None):
    w2, b2 = c["ws"][4].astype(np.float64), c["ws"][5].astype(np.float64)
    if mut == "b2_missing":
        b2 = np.zeros_like(b2)
    return t2 @ w2 + b2, dt2 @ np.abs(w2) + gamma(H2 + 1) * ((np.abs(t2) + dt2) @ np.abs(w2) + np.abs(b2))


def forward(c, v, mut=None):
    """{h1, t, h2, t2, out: (float64 reference, bound propagated from the inputs)}."""
    h1 = s_h1(c, mut)
    t = s_adj(c, *h1, mut)
    h2 = s_h2(c, v, *t)
    t2 = s_adj(c, *h2, mut)
    return dict(h1=h1, t=t, h2=h2, t2=t2, out=s_out(c, *t2, mut))


def sharp(c, v, got):
    """{h1, t, h2, t2, out: (reference, one stage's bound)} from the DEVICE's own previous stage `got` (f32 arrays)."""
    z = lambda a: (a.astype(np.float64), np.zeros(a.shape))                                # noqa: E731
    return dict(h1=s_h1(c), t=s_adj(c, *z(got["h1"])), h2=s_h2(c, v, *z(got["t"])), t2=s_adj(c, *z(got["h2"])),
                out=s_out(c, *z(got["t2"])))


def backward(c, v, keep, mut=None):
    """{dw0 .. db2: (float64 reference, bound)} from g, the saved activations (f32) and a_t, accumulated onto c["init"].
    m(h) = h > 0 ? 1 : slope; a dropped element's factor is 0."""
    f = np.float64
    n, slope = c["n"], float(np.float32(c["slope"]))
    sv = {k: x.astype(f) for k, x in v["saved"].items()}
    g, ax = c["g"].astype(f), c["ax"].astype(f)
    w1, w2 = c["ws"][2].astype(f), c["ws"][4].astype(f)
    at = (c["a"] if mut == "a_for_at" else c["a_t"])
    rw = np.ones((n, 1))
    if mut == "clamp_last_row":                         # rows beyond n repeat row n - 1 instead of reading as zero
        rw[-1] = 1 + (-n) % RB
    gm = gamma(RB + cdiv(n, RB))
    out = {}

    def grads(wname, bname, S, G, dG):
        i_w, i_b = (np.zeros_like(c["init"][k], dtype=f) if mut == "overwrite" else c["init"][k].astype(f) for k in (wname, bname))
        Sw = S * rw
        out[wname] = (i_w + Sw.T @ G, np.abs(Sw).T @ dG + gm * (np.abs(Sw).T @ (np.abs(G) + dG) + np.abs(i_w)))
        out[bname] = (i_b + (G * rw).sum(0), (dG * rw).sum(0) + gm * (((np.abs(G) + dG) * rw).sum(0) + np.abs(i_b)))

    grads("dw2", "db2", sv["t2"], g, np.zeros_like(g))
    dt2 = g @ w2.T
    d = gamma(H3) * (np.abs(g) @ np.abs(w2).T)
    dh2, L = _product(at, dt2, mut)
    d = np.abs(L) @ d + gamma(kterms(n)) * (np.abs(L) @ (np.abs(dt2) + d))
    m2 = np.where(sv["h2"] > 0, 1.0, slope)
    fac = m2 if keep is None else np.where(keep, v["ik"] * m2, slope if mut == "slope_for_dropped" else 0.0)
    du = dh2 * fac
    d = (d + 2 * U * (np.abs(dh2) + d)) * np.abs(fac)
    grads("dw1", "db1", sv["t"], du, d)
    dt = du @ w1.T
    d = d @ np.abs(w1).T + gamma(H2) * ((np.abs(du) + d) @ np.abs(w1).T)
    dh1, L = _product(at, dt, mut)
    d = np.abs(L) @ d + gamma(kterms(n)) * (np.abs(L) @ (np.abs(dt) + d))
    m1 = np.where(sv["h1"] > 0, 1.0, slope)
    dpre = dh1 * m1
    d = (d + U * (np.abs(dh1) + d)) * m1
    grads("dw0", "db0", ax, dpre, d)
    out["_stages"] = dict(dt2=dt2, dh2=dh2, du=du, dt=dt, dh1=dh1, dpre=dpre)
    return out


GRADS = ("dw0", "db0", "dw1", "db1", "dw2", "db2")
# the dyadic unit every value of a stage is a multiple of in the exact family
STAGE_UNIT = dict(h1=2.0 ** -1, t=2.0 ** -2, h2=2.0 ** -3, t2=2.0 ** -4, out=2.0 ** -4, dt2=1.0, dh2=2.0 ** -1, du=2.0 ** -2,
                  dt=2.0 ** -2, dh1=2.0 ** -3, dpre=2.0 ** -4, dw2=2.0 ** -4, db2=1.0, dw1=2.0 ** -4, db1=2.0 ** -2, dw0=2.0 ** -4,
                  db0=2.0 ** -4)


def exact_terms(c, v):
    """{output: (value, sum of the magnitudes of its terms)} of every product of both passes."""
    f = np.float64
    A = np.abs
    ax, a, at = (A(c[k]).astype(f) for k in ("ax", "a", "a_t"))
    w0, b0, w1, b1, w2, b2 = (A(w).astype(f) for w in c["ws"])
    g, init = A(c["g"]).astype(f), {k: A(x).astype(f) for k, x in c["init"].items()}
    fw = {k: x[0] for k, x in v["fwd"].items()}
    bw, st = v["bwd"], v["bwd"]["_stages"]
    sv = {k: A(x).astype(f) for k, x in v["saved"].items()}
    return dict(h1=(fw["h1"], ax @ w0 + b0), t=(fw["t"], a @ A(fw["h1"])), h2=(fw["h2"], (A(fw["t"]) @ w1 + b1) * v["ik"]),
                t2=(fw["t2"], a @ A(fw["h2"])), out=(fw["out"], A(fw["t2"]) @ w2 + b2),
                dt2=(st["dt2"], g @ w2.T), dh2=(st["dh2"], at @ A(st["dt2"])), du=(st["du"], A(st["dh2"]) * v["ik"]),
                dt=(st["dt"], A(st["du"]) @ w1.T), dh1=(st["dh1"], at @ A(st["dt"])), dpre=(st["dpre"], A(st["dh1"])),
                dw2=(bw["dw2"][0], sv["t2"].T @ g + init["dw2"]), db2=(bw["db2"][0], g.sum(0) + init["db2"]),
                dw1=(bw["dw1"][0], sv["t"].T @ A(st["du"]) + init["dw1"]), db1=(bw["db1"][0], A(st["du"]).sum(0) + init["db1"]),
                dw0=(bw["dw0"][0], ax.T @ A(st["dpre"]) + init["dw0"]), db0=(bw["db0"][0], A(st["dpre"]).sum(0) + init["db0"]))


def assert_exact_gcn(c, drop):
    """Every output of every product: a multiple of its stage's unit, the sum of the magnitudes of its terms below 2^24 units."""
    v = variant(c, drop)
    worst = 0.0
    for name, (val, mag) in exact_terms(c, v).items():
        unit = STAGE_UNIT[name]
        q = val / unit
        assert np.array_equal(q, np.round(q)), (c["n"], c["K0"], drop, name)
        w = float(max(mag.max(initial=0.0), np.abs(val).max(initial=0.0))) / unit
        assert w < 2.0 ** 24, (c["n"], c["K0"], drop, name, w)
        worst = max(worst, w)
    c["_exact_worst"] = max(c.get("_exact_worst", 0.0), worst)
    return worst


# ------------------------------------------------------------------------------------------------ SpMM
def _csr(rng, n_rows, n_cols, degs, exact, last_col_row):
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(degs)
    col = np.concatenate([rng.choice(n_cols, d, replace=False) for d in degs] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    e = rowptr[last_col_row]
    if n_cols - 1 not in col[e:rowptr[last_col_row + 1]]:
        col[e] = n_cols - 1                              # a column index equal to the last row of the dense operand
    if exact:
        val = rng.choice(np.float32([1, 0.5, -1, 2]), col.size)
    else:
        val = (rng.uniform(0.5, 1.5, col.size) / (np.repeat(degs, degs) + 1.0)).astype(np.float32)
    erow = np.repeat(np.arange(n_rows), degs)
    epos = np.arange(col.size) - rowptr[erow]
    return dict(rowptr=rowptr, col=col, val=val, erow=erow, epos=epos, degs=np.asarray(degs), shape=(n_rows, n_cols))


def dense(g, emask=None, absval=False):
    m = np.zeros(g["shape"])
    val = np.abs(g["val"]) if absval else g["val"]
    val = val.astype(np.float64) * (1.0 if emask is None else emask)
    np.add.at(m, (g["erow"], g["col"]), val)
    return m


def _operand(rng, shape, exact, lim=8):
    return rng.integers(-lim, lim + 1, shape).astype(np.float32) if exact else rng.standard_normal(shape).astype(np.float32)


def _build_spmm(spec):
    rng = _rng("spmm", spec["id"])
    exact = spec["family"] == "exact"
    C, e = spec["C"], spec["entry"]
    c = dict(spec=spec, exact=exact)
    if e in ("csr", "t_rows"):
        degs = [CSR_DEGS[i % len(CSR_DEGS)] for i in range(CSR_ROWS)]
        c["graph"] = g = _csr(rng, CSR_ROWS, CSR_COLS, degs, exact, 1)
        first = rng.permutation(len(CSR_DEGS))                 # every neighbour count is in every subset
        r17 = CSR_DEGS.index(17)
        c["rows"] = {"null": None, "subset": np.concatenate([first, [12, 21]]),
                     "repeat": np.concatenate([first, [r17, 15, r17]])}[spec["rows"]]
        if c["rows"] is not None:
            c["rows"] = c["rows"].astype(np.int64)
        R = CSR_ROWS if c["rows"] is None else c["rows"].size
        assert R % 4 != 0
        c["R"] = R
        if e == "csr":
            c["b"] = _operand(rng, (CSR_COLS, C), exact)
            c["bias"] = _operand(rng, (C,), exact) if spec["bias"] else None
        else:
            c["g"] = _operand(rng, (R, C), exact, 2)
            c["g"][rng.random((R, C)) < 0.2] = 0.0
            c["init"] = rng.integers(-3, 4, (CSR_COLS, C)).astype(np.float32)
    else:
        P, R = GATHER_P, spec["R"]
        degs = list(GATHER_DEGS) + list(rng.integers(0, 6, P - len(GATHER_DEGS)))
        c["graph"] = _csr(rng, P, P, degs, exact, 1)            # the CSR of the transpose: row j lists the sources i of its in-edges
        rows = rng.choice(P, max(R - 2, 0), replace=False).astype(np.int64)
        if R:
            rows[:2] = (0, P - 1)
            rows = np.concatenate([rows, rows[3:4], rows[3:4]])   # one row three times
            rows = rows[rng.permutation(R)]
        c["rows"], c["R"], c["P"] = rows, R, P
        c["g"] = _operand(rng, (max(R, 1), C), exact, 2)
    if exact:
        for name, (ref, bound, mag) in restate_spmm(c, with_mag=True).items():
            q = ref * 2
            assert np.array_equal(q, np.round(q)) and float(mag.max(initial=0.0)) * 2 < 2.0 ** 24, (spec["id"], name)
    return c


def narrow_groups(C):
    """Lane groups of the narrow kernels (mobgt_spmm_csr's dispatch), or 0 for the generic kernel."""
    return {64: 4, 128: 2}.get(C, 0)


def _sel(c, mut=None):
    """(dense [R, n_cols] of the selected rows, the same of |values|) with a defect's edges dropped."""
    g, C = c["graph"], c["spec"]["C"]
    ngr = narrow_groups(C)
    emask = np.ones(g["col"].size)
    if mut == "drop_unroll_tail":
        step = 4 * ngr if ngr else 4
        emask = (g["epos"] < step * (g["degs"][g["erow"]] // step)).astype(np.float64)
    elif mut == "drop_lane_group" and ngr:
        emask = (g["epos"] % ngr != 1).astype(np.float64)
    d, da = dense(g, emask), dense(g, emask, absval=True)
    return (d, da) if c["rows"] is None else (d[c["rows"]], da[c["rows"]])


def restate_spmm(c, mut=None, with_mag=False):
    """{output: (float64 reference, bound)} of a SpMM case (with_mag: also the sum of the magnitudes of the terms)."""
    s = c["spec"]
    e, C, f = s["entry"], s["C"], np.float64
    out = {}
    if e == "csr":
        sel, sela = _sel(c, mut)
        bias = c["bias"].astype(f) if c["bias"] is not None else np.zeros(C)
        if mut == "bias_every_group" and narrow_groups(C):
            bias = bias * narrow_groups(C)
        ref = sel @ c["b"].astype(f) + bias
        mag = sela @ np.abs(c["b"]).astype(f) + np.abs(bias)
        m = (sela != 0).sum(1, keepdims=True) + 4
        out["out"] = (ref, gamma(m) * mag, mag)
    elif e == "t_rows":
        sel, sela = _sel(c)
        g = c["g"].astype(f)
        if mut == "repeat_once":
            first = np.zeros(c["R"], dtype=bool)
            first[np.unique(c["rows"] if c["rows"] is not None else np.arange(c["R"]), return_index=True)[1]] = True
            g = g * first[:, None]
        init = np.zeros_like(c["init"], dtype=f) if mut == "overwrite" else c["init"].astype(f)
        ref = init + sel.T @ g
        mag = np.abs(init) + sela.T @ np.abs(g)
        m = (sela.T != 0) @ (g != 0).astype(f) + 1
        out["db"] = (ref, gamma(m) * mag, mag)
    else:
        P, R = c["P"], c["R"]
        T, Ta = dense(c["graph"]), dense(c["graph"], absval=True)
        onehot = np.zeros((P, max(R, 1)))
        if R:
            rows = c["rows"]
            if mut == "repeat_once":                     # head[i] = the last k that names i; its list is not followed
                last = {int(r): k for k, r in enumerate(rows)}
                onehot[list(last.keys()), list(last.values())] = 1
            else:
                onehot[rows, np.arange(R)] = 1
        g = c["g"].astype(f) if R else np.zeros((1, C))
        ref = T @ (onehot @ g)
        mag = Ta @ (onehot @ np.abs(g))
        if mut == "second_float4_dropped":
            ref[:, 256:] = 0
        m = ((Ta != 0) @ onehot.sum(1, keepdims=True)) + 1
        out["db"] = (ref, gamma(m) * mag, mag)
        head = np.full(P, -1, dtype=f)
        if mut == "head_threaded" and R:
            head[c["rows"][0]] = 0
        out["head"] = (head, np.zeros(P), np.abs(head))
    return out if with_mag else {k: x[:2] for k, x in out.items()}


# ------------------------------------------------------------------------------------------------ emulation and verdicts
def emulate(c, mut=None):
    """What kernels with defect `mut` (None: correct ones) would leave, as float32 arrays."""
    e = c["spec"]["entry"]
    if e in ("fwd", "bwd"):
        v = c["v"] if mut is None else variant(c["net"], c["spec"]["drop"], mut)
        names = ("h1", "t", "h2", "t2", "out") if e == "fwd" else GRADS
        return {k: v[e][k][0].astype(np.float32) for k in names}
    return {k: x[0].astype(np.float32) for k, x in restate_spmm(c, mut).items()}


def _judge(family, refs, got):
    case = dict(spec=dict(family=family), _ref={k: dict(kind="f32", ref=r, bound=b) for k, (r, b) in refs.items()})
    return mr.verdict(case, got)


def verdict(c, got):
    """(ok, worst error / bound) of an entry's outputs `got` (emulate's layout).  Exact family: every output equals the float64
    restatement as a value.  Rounding family: every element within its bound; the forward's saved activations against their stage
    function applied to the device's own previous stage as well as end to end."""
    s = c["spec"]
    e, fam = s["entry"], s["family"]
    if e == "fwd":
        ok, worst = _judge(fam, c["v"]["fwd"], got)
        if fam == "round":
            ok2, w2 = _judge(fam, sharp(c["net"], c["v"], got), got)
            ok, worst = ok and ok2, max(worst, w2)
        return ok, worst
    if e == "bwd":
        return _judge(fam, {k: c["v"]["bwd"][k] for k in GRADS}, got)
    return _judge(fam, restate_spmm(c), got)


# the defects an entry can show at all; where a defect needs a shape or an option, `applies` says which
APPLIES = dict(fwd=("stale_L_after_layer1", "drop_chunk_tail", "drop_wave", "hash_without_salt", "b2_missing"),
               bwd=("drop_chunk_tail", "drop_wave", "clamp_last_row", "a_for_at", "slope_for_dropped", "overwrite"),
               csr=("drop_unroll_tail", "drop_lane_group", "bias_every_group"), t_rows=("repeat_once", "overwrite"),
               gather=("repeat_once", "second_float4_dropped", "head_threaded"))


def applies(spec, mut):
    e = spec["entry"]
    if mut not in APPLIES[e]:
        return False
    if e in ("fwd", "bwd"):
        n, K0 = spec["n"], spec["K0"]
        return dict(stale_L_after_layer1=fwd_form(n, K0) == "restage", hash_without_salt=spec["drop"] > 0 and n >= 15,
                    slope_for_dropped=spec["drop"] > 0 and n >= 15, clamp_last_row=n % RB != 0,
                    drop_chunk_tail=n >= 15, drop_wave=n >= 15, a_for_at=n >= 15).get(mut, True)
    if e == "csr":
        return dict(drop_lane_group=narrow_groups(spec["C"]) > 0,
                    bias_every_group=narrow_groups(spec["C"]) > 0 and spec["bias"]).get(mut, True)
    if e == "t_rows":
        return mut != "repeat_once" or spec["rows"] == "repeat"
    return spec["R"] > 0 and (mut != "second_float4_dropped" or spec["C"] > 256)
