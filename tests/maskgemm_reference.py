"""Reference side of the bitmask GCN matrix (tests/test_gpu_maskgemm_matrix.py, tests/test_host_maskgemm_reference.py): the case
list as plain data, a case builder for two input families, a float64 restatement of every contract of include/mobgt_hip.h that
csrc/maskgemm.hip, mobgt_small_gemm_f32_act (csrc/sgemm.hip, csrc/sgemm_body.h) and mobgt_bias_act_fwd_t (csrc/layer.hip)
implement, the defects the verdicts must reject, and the rounding family's per-element tolerance.  NumPy only; the dropout keep
mask is the host replay of the device hash (ops.dropout_site_mask).

Exact family.  Operands are integers (|v| <= 8, weights |v| <= 3), scales come from {2, 1, 1/2, 1/4}, the slope is 1/2 and dropout
is p = 0.5 (inv_keep exactly 2), so m(y) takes the values (2, 1, 0).  A mask bit times a bf16 value and a full-f32 MFMA product of
such numbers are exact; the builder asserts for every output that the sum of the magnitudes of its terms, in units of the smallest
operand unit, stays below 2^24.  Every partial sum in any order is then a representable f32, and the kernels must return the
float64 result bit for bit (+0 and -0 compare equal); bf16 outputs compare as bit patterns.

Rounding family.  Real operands, rscale = 1 / (deg + 1), slope 0.2, p = 0.3.  The reference rounds where the kernels round
operands (f32 product with a scale or mask factor, then round-to-nearest-even to bf16) and is float64 elsewhere.  Tolerance, per
element, with u = 2^-24 and gamma(n) = n u / (1 - n u) (the forward error of n f32 roundings on one path, any order):
    product sums   gamma(n) * sum |terms|,  n = k-terms (K rounded up to whole MFMA steps) + wave partials + epilogue roundings:
                   mask_gemm        n = K32 + NWAVE + 2    (+ the fmaf with rscale and bias)
                   l1 / rows t, u   n = K32 + 16 + 1       (16 waves, the multiply by rscale)
                   rows_bwd dy1     n = R32 + 8            (8 waves)
                   small gemm       n = K16 + 4 + 1        (split-K: four partial tiles; the bias add)
    fmaf chains    an input error d propagates as (d |W|) (1 + gamma(c)) and the chain of c fmafs adds gamma(c) (|x| |W| + |b|):
                   c = 16 for t W1 + b1 and u W2 + b2, c = 64 for (dy1 m) W1^T;
    pointwise      every further f32 multiply (slope, inv_keep, mask factor, row scale) adds u (|value| + d); LeakyReLU has
                   Lipschitz constant 1, so an error in front of it passes through unchanged;
    bf16 outputs   pass if bf16(ref - bound) <= got <= bf16(ref + bound) (rounding is monotone), no element exempt.
The bounds are derived from the code, not tuned on device output."""
import zlib

import numpy as np

U = 2.0 ** -24
EXACT_SCALES = (2.0, 1.0, 0.5, 0.25)
GH, GI = 64, 16                                       # csrc/maskgemm.hip: widths of the two hidden layers
MAX_NO = 192                                          # MASK_ROWS_MAX_NO
LDS_LIMIT = 120 * 1024                                # mobgt_mask_rows_bwd's dynamic LDS ceiling
F32C, BF16C = 0, 1                                    # MOBGT_F32, MOBGT_BF16

MUTANTS = ("drop_kstep", "drop_wave", "mask_for_mask_t", "clamp_last_row", "swap_parts", "b2_every_part", "rscale_after_bias",
           "round_before_scale", "truncate", "hash_without_salt", "mzero_for_negative", "kb_ignored")
ROUNDING_MUTANTS = ("round_before_scale", "truncate")   # power-of-two scales commute with rounding, integers are bf16 values


def cdiv(a, b):
    return (a + b - 1) // b


def roundup(a, b):
    return cdiv(a, b) * b


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------ helpers
def pack_bits(b, words=None):
    """Bool [M, K] -> uint32 [M, words]: bit k & 31 of word k >> 5, rows padded to whole groups of four words, bits >= K zero."""
    M, K = b.shape
    words = roundup(K, 128) // 32 if words is None else words
    padded = np.zeros((M, words * 32), dtype=np.uint64)
    padded[:, :K] = b
    return (padded.reshape(M, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def bf16_bits(v, truncate=False):
    """float -> uint16 bf16 patterns, round-to-nearest-even on the f32 bit pattern (or truncation)."""
    u = np.ascontiguousarray(np.asarray(v, dtype=np.float32)).view(np.uint32)
    if not truncate:
        u = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    return (u >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def bf16(v):
    return bf16_value(bf16_bits(v))


def dropout_threshold(p):
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))          # csrc/common.h


def inv_keep(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(dropout_threshold(p)) / np.float32(65536.0)))


def keep_mask(seed, salt, R, C, p):
    from mobgt_amd import ops
    return ops.dropout_site_mask(seed, salt, R, C, p)


def act_mask(y, vals, mut=None):
    pos, neg, zer = vals
    if mut == "mzero_for_negative":
        neg = zer
    return np.where(y > 0, pos, np.where(y < 0, neg, zer)).astype(np.float64)


def leaky(a, slope):
    return np.where(a > 0, a, float(np.float32(slope)) * a)


# ------------------------------------------------------------------------------------------------ launch regimes, restated
MASK_GEMM_FORM = {16: (1, 16), 32: (2, 16), 48: (3, 8), 64: (4, 8)}       # N -> (NB, NWAVE): the dispatch of mobgt_mask_gemm


def wave_slices(K, nwave):
    """[(s0, s1)] of 32-deep k-steps per wave: per = roundup(ceil(nsteps / NWAVE), 4) (every mask kernel of maskgemm.hip)."""
    nsteps = (K + 31) >> 5
    per = (cdiv(nsteps, nwave) + 3) & ~3
    return [(w * per, min(nsteps, w * per + per)) for w in range(nwave)]


def prefetches(K, nwave):
    """Some wave runs `if (ks + 4 < s1) load(nxt, ks + 4)`: a wave owns more than one group of four steps."""
    return any(s1 - s0 > 4 for s0, s1 in wave_slices(K, nwave))


def sgemm_vec(K, lda, ldb, b_is_nk, a_off_bytes=0, b_off_bytes=0):
    return K % 16 == 0 and lda % 4 == 0 and a_off_bytes % 16 == 0 and (not b_is_nk or (ldb % 4 == 0 and b_off_bytes % 16 == 0))


def sgemm_branch(M, N, K, b_is_nk, vec):
    """"splitk" or the NB of the one-wave kernel: run() of csrc/sgemm.hip."""
    rows16 = cdiv(M, 16)
    if not b_is_nk and vec and N <= 16 and 128 <= K <= 512 and rows16 >= 64:
        return "splitk"
    nb = 4
    while nb > 1 and (rows16 * cdiv(N, 16 * nb) < 256 or N <= 16 * (nb // 2)):
        nb >>= 1
    return nb


def rows_bwd_nw(R):
    return roundup(R, 128) // 32                      # words of r-bits per k-row: wave w takes the steps w, w + 8, ...


def rows_bwd_lds_bytes(ldm, R):
    ldg = roundup(R, 128)
    region = max(32 * (ldm + 1) * 4, 8 * 32 * (GH + 4) * 4)
    return region + ldg * 4 + 32 * (ldg // 32 + 1) * 4


def rows_bwd_max_R(ldm):
    R = 128
    while rows_bwd_lds_bytes(ldm, R + 128) <= LDS_LIMIT:
        R += 128
    return R


# ------------------------------------------------------------------------------------------------ the matrix
MG_16 = ((1, 1), (31, 33), (32, 128), (33, 129), (77, 1000), (40, 2048), (45, 2049), (64, 2081))
MG_8 = ((17, 31), (32, 1024), (33, 1025), (50, 1057))
L1_MK = ((1, 33), (31, 128), (32, 129), (33, 1000), (63, 2049), (64, 2081))
RF_R, RF_K, RF_NO = (1, 15, 16, 17, 48, 203), (33, 129, 1000, 2049), (4, 64, 128, 188, 192)
RF_CASES = ((1, 33, 4), (15, 129, 64), (16, 1000, 128), (17, 2049, 188), (48, 33, 192), (203, 129, 4), (203, 1000, 192),
            (17, 129, 128), (1, 2049, 64), (48, 1000, 188), (16, 33, 64), (15, 2049, 192))
RB_R, RB_P = (1, 16, 127, 128, 129, 257, 300), (31, 32, 33, 777, 1003)
RB_CASES = ((1, 31), (16, 32), (127, 33), (128, 777), (129, 1003), (257, 33), (300, 777), (300, 31), (257, 1003), (1, 1003),
            ("max", 33))
# (name, M, N, K, k_b, b_is_nk, how vec is switched off or None)
SG_BRANCHES = (("nb4-kn", 4096, 64, 32, 0, 0, None), ("nb4-nk", 4096, 64, 32, 0, 1, None),
               ("nb2-kn-K20", 4096, 32, 20, 0, 0, "K"), ("nb2-nk-K20", 4096, 32, 20, 0, 1, "K"),
               ("nb1-kn-stride", 37, 17, 48, 40, 0, "stride"), ("nb1-nk-stride", 37, 17, 48, 0, 1, "stride"),
               ("splitk-128", 1009, 16, 128, 128, 0, None), ("splitk-304", 1030, 16, 304, 303, 0, None),
               ("splitk-512", 1025, 5, 512, 500, 0, None), ("fallback-528", 1030, 16, 528, 528, 0, None))
# (a_mask, act: 0 none | 1 leaky | 2 leaky + dropout, c_dtype, ct: None | "beside" | "only", ct_scale, bias, seed_dev)
SG_OPTIONS = ((0, 0, F32C, None, 0, 1, 0), (1, 1, BF16C, "beside", 0, 0, 0), (0, 2, F32C, "only", 1, 1, 1),
              (1, 2, BF16C, "beside", 1, 1, 0), (1, 0, F32C, "only", 0, 0, 0), (0, 1, BF16C, None, 0, 1, 0))
BA_C, BA_R = (16, 64, 192, 260), (1, 777)


def S(entry, family, name, **kw):
    return dict(kw, entry=entry, family=family, id=f"{entry}-{family}-{name}")


def matrix_specs():
    specs = []
    for fam in ("exact", "round"):
        k = 0
        for N, shapes in ((16, MG_16), (32, MG_16), (48, MG_8), (64, MG_8)):
            for j, (M, K) in enumerate(shapes):              # every flag takes both values within four consecutive shapes
                flip = j >= 4
                specs.append(S("mask_gemm", fam, f"M{M}-K{K}-N{N}-o{j}", M=M, K=K, N=N, rscale=bool(j & 1), bscale=bool(j & 2),
                               bias=(j % 4 in (1, 2)) != flip, x_null=(j % 4 in (0, 3)) != flip, wide=j % 2 == 0))
        k = 0
        for M, K in L1_MK:
            for drop in (0, 1, 2):                       # off | on, seed_dev null | on, seed_dev given
                specs.append(S("l1", fam, f"M{M}-K{K}-d{drop}-z{(k + drop) % 3}", M=M, K=K, drop=drop, zero=(k + drop) % 3,
                               wide=k % 2 == 1))
            k += 1
        for k, (R, K, NO) in enumerate(RF_CASES):
            specs.append(S("rows_fwd", fam, f"R{R}-K{K}-NO{NO}-o{k % 4}", R=R, K=K, NO=NO, b2=bool(k & 1), rs_rows=bool(k & 2),
                           wide=k % 3 == 1))
        for k, (R, P) in enumerate(RB_CASES):
            ldm = cdiv(P, 32) + (3 if k % 2 else 0)
            Rv = rows_bwd_max_R(ldm) if R == "max" else R
            specs.append(S("rows_bwd", fam, f"R{R}-P{P}-ldm{ldm}", R=Rv, P=P, ldm=ldm, is_max=R == "max"))
        for name, M, N, K, k_b, nk, novec in SG_BRANCHES:
            for o, (am, act, cdt, ct, cts, bias, sd) in enumerate(SG_OPTIONS):
                specs.append(S("sgemm", fam, f"{name}-o{o}", branch=name, M=M, N=N, K=K, k_b=k_b, b_is_nk=nk, novec=novec, a_mask=am,
                               act=act, c_dtype=cdt, ct=ct, ct_scale=cts, bias=bias, seed_dev=sd))
        k = 0
        for C in BA_C:
            for R in BA_R:
                for drop in (0, 1):
                    specs.append(S("bias_act", fam, f"R{R}-C{C}-d{drop}-t{(k + drop) % 2}", R=R, C=C, drop=drop, y_t=(k + drop) % 2 == 0,
                                   bias=k % 3 != 2))
                k += 1
    check_coverage(specs)
    return specs


def sgemm_layout(spec):
    """(lda, a column offset, ldb, b column offset) of the staged operands: views into wider buffers; "stride" makes the row pitch
    odd, which switches the 16-byte loads off."""
    K, N, nk = spec["K"], spec["N"], spec["b_is_nk"]
    bw = K if nk else N
    if spec["novec"] == "stride":
        return K + 5, 4, bw + 5, 4
    return K + 8, 4, bw + 8, 4


def sgemm_regime(spec):
    lda, _, ldb, _ = sgemm_layout(spec)
    vec = sgemm_vec(spec["K"], lda, ldb, spec["b_is_nk"])
    return vec, sgemm_branch(spec["M"], spec["N"], spec["K"], spec["b_is_nk"], vec)


def check_coverage(specs):
    """Every dispatch branch of the entries under test is reached by at least one case of each family."""
    for fam in ("exact", "round"):
        of = lambda e: [s for s in specs if s["entry"] == e and s["family"] == fam]          # noqa: E731
        mg = of("mask_gemm")
        forms = {(MASK_GEMM_FORM[s["N"]], prefetches(s["K"], MASK_GEMM_FORM[s["N"]][1])) for s in mg}
        assert forms == {(f, p) for f in MASK_GEMM_FORM.values() for p in (False, True)}, forms
        assert {(s["M"], s["K"]) for s in mg if s["N"] in (16, 32)} == set(MG_16) and all(s["M"] != s["K"] or s["M"] == 1 for s in mg)
        assert {(s["M"], s["K"]) for s in mg if s["N"] in (48, 64)} == set(MG_8)
        for key in ("rscale", "bscale", "bias", "x_null", "wide"):
            for N in MASK_GEMM_FORM:
                assert {s[key] for s in mg if s["N"] == N} == {False, True}, (key, N)
        # several waves with work, waves without work, a last wave with a partial group
        assert any(sum(s1 > s0 for s0, s1 in wave_slices(s["K"], 16)) == 1 for s in mg if s["N"] == 16)
        assert any(sum(s1 > s0 for s0, s1 in wave_slices(s["K"], 16)) == 16 for s in mg if s["N"] == 16)
        l1 = of("l1")
        assert {(s["M"], s["K"]) for s in l1} == set(L1_MK) and {prefetches(s["K"], 16) for s in l1} == {False, True}
        assert {(s["drop"], s["zero"]) for s in l1} == {(d, z) for d in range(3) for z in range(3)}
        assert {s["M"] % 2 for s in l1} == {0, 1}
        rf = of("rows_fwd")
        assert {s["R"] for s in rf} == set(RF_R) and {s["K"] for s in rf} == set(RF_K) and {s["NO"] for s in rf} == set(RF_NO)
        assert {(s["b2"], s["rs_rows"]) for s in rf} == {(a, b) for a in (False, True) for b in (False, True)}
        assert {prefetches(s["K"], 16) for s in rf} == {False, True}
        rb = of("rows_bwd")
        assert {s["R"] for s in rb if not s["is_max"]} == set(RB_R) and {s["P"] for s in rb} == set(RB_P)
        assert {rows_bwd_nw(s["R"]) for s in rb} >= {4, 8, 12} and {s["ldm"] > cdiv(s["P"], 32) for s in rb} == {False, True}
        mx = [s for s in rb if s["is_max"]]
        assert mx and all(rows_bwd_lds_bytes(s["ldm"], s["R"]) <= LDS_LIMIT < rows_bwd_lds_bytes(s["ldm"], s["R"] + 1) for s in mx)
        sg = of("sgemm")
        reg = {s["branch"]: sgemm_regime(s) for s in sg}
        assert {reg[n] for n in ("nb4-kn", "nb4-nk")} == {(True, 4)} and {reg[n] for n in ("nb2-kn-K20", "nb2-nk-K20")} == {(False, 2)}
        assert {reg[n] for n in ("nb1-kn-stride", "nb1-nk-stride")} == {(False, 1)}
        assert {reg[n] for n in ("splitk-128", "splitk-304", "splitk-512")} == {(True, "splitk")} and reg["fallback-528"] == (True, 1)
        for name in reg:
            mine = [s for s in sg if s["branch"] == name]
            assert {s["a_mask"] for s in mine} == {0, 1} and {s["act"] for s in mine} == {0, 1, 2}
            assert {s["c_dtype"] for s in mine} == {F32C, BF16C} and {s["ct"] for s in mine} == {None, "beside", "only"}
            assert {s["ct_scale"] for s in mine if s["ct"]} == {0, 1}
        assert {(s["M"], s["N"], s["K"], s["k_b"]) for s in sg if s["branch"].startswith("splitk")} == \
            {(1009, 16, 128, 128), (1030, 16, 304, 303), (1025, 5, 512, 500)}
        ba = of("bias_act")
        assert {(s["R"], s["C"]) for s in ba} == {(r, c) for r in BA_R for c in BA_C}
        assert {(s["drop"], s["y_t"]) for s in ba} == {(d, t) for d in (0, 1) for t in (False, True)}


# ------------------------------------------------------------------------------------------------ case builder
SEED, SEED_DEV = 0x51F15EED1234, 77


def _rng(spec, salt=""):
    return np.random.default_rng(zlib.crc32((spec["id"] + "/" + salt).encode()))


def _vals(rng, shape, exact, lim=8):
    """f32 operands that are bf16 values: integers, or reals rounded to bf16."""
    if exact:
        return rng.integers(-lim, lim + 1, shape).astype(np.float32)
    return bf16(rng.standard_normal(shape)).astype(np.float32)


def _f32(rng, shape, exact, lim=8):
    """f32 operands the kernels round themselves: integers, or reals with all 24 bits."""
    if exact:
        return rng.integers(-lim, lim + 1, shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _scales(rng, n, exact, deg=None):
    if exact:
        return rng.choice(np.array(EXACT_SCALES, dtype=np.float32), n)
    deg = rng.integers(0, 50, n) if deg is None else deg
    return (1.0 / (deg.astype(np.float64) + 1.0)).astype(np.float32)


def _bits(rng, M, K):
    """A non-symmetric 0/1 matrix of random density whose first and last columns are populated."""
    b = rng.random((M, K)) < rng.uniform(0.05, 0.6)
    b[:, K - 1] = rng.random(M) < 0.7
    b[:, 0] = rng.random(M) < 0.7
    b[M - 1, K - 1] = True
    return b


def _act_out(rng, shape):
    """An activation output: positive, negative, +0.0 and -0.0 entries."""
    kinds = np.array([1.5, -2.0, 0.0, -0.0], dtype=np.float32)
    m = kinds[rng.choice(4, size=shape, p=[0.4, 0.4, 0.1, 0.1])]
    flat = m.reshape(-1)
    flat[:min(4, flat.size)] = kinds[:min(4, flat.size)]
    return m


def _rows(rng, R, K):
    rows = rng.integers(0, K, R).astype(np.int64)
    if R >= 2:
        rows[rng.integers(0, R)] = 0
        rows[0 if R == 2 else R // 2] = K - 1
    if R == 1:
        rows[0] = K - 1
    if R >= 4:
        rows[R - 1] = rows[1]                            # a repeat
    return rows


def family_consts(spec):
    exact = spec["family"] == "exact"
    slope, p = (0.5, 0.5) if exact else (0.2, 0.3)
    ik = inv_keep(p)
    return exact, slope, p, ik, (ik, float(np.float32(slope) * np.float32(ik)), 0.0)     # m(y) of a dropout(leaky) output


def build_case(spec):
    """NumPy inputs of a spec.  The exact family's exactness condition is asserted here, on the reference's own magnitudes."""
    rng = _rng(spec)
    exact, slope, p, ik, mvals = family_consts(spec)
    e = spec["entry"]
    c = dict(spec=spec, slope=slope, p=p, inv_keep=ik, mask_vals=mvals)
    if e == "mask_gemm":
        M, K, N = spec["M"], spec["K"], spec["N"]
        c["bits"] = _bits(rng, M, K)
        c["x"] = _f32(rng, (K, N), exact)
        c["bscale"] = _scales(rng, K, exact) if spec["bscale"] else None
        c["rscale"] = _scales(rng, M, exact, c["bits"].sum(1)) if spec["rscale"] else None
        c["bias"] = _f32(rng, (N,), exact) if spec["bias"] else None
    elif e == "l1":
        M, K = spec["M"], spec["K"]
        c["bits"] = _bits(rng, M, K)
        c["y0"] = _vals(rng, (K, GI), exact, 4)
        c["rscale"] = _scales(rng, M, exact, c["bits"].sum(1))
        c["w1"], c["b1"] = _f32(rng, (GI, GH), exact, 3), _f32(rng, (GH,), exact)
        c["drop"], c["salt"] = spec["drop"], 0x2040
        c["seed"], c["seed_dev"] = SEED + M, (SEED_DEV if spec["drop"] == 2 else None)
    elif e == "rows_fwd":
        R, K, NO = spec["R"], spec["K"], spec["NO"]
        c["bits"] = _bits(rng, K, K)
        c["rows"] = _rows(rng, R, K)
        c["y1"] = _vals(rng, (K, GH), exact)
        c["rscale"] = _scales(rng, K, exact, c["bits"].sum(1))
        c["w2"] = _f32(rng, (GH, NO), exact, 3)
        c["b2"] = _f32(rng, (NO,), exact) if spec["b2"] else None
    elif e == "rows_bwd":
        R, P = spec["R"], spec["P"]
        c["bits"] = _bits(rng, P, P)                     # A; the kernel is handed the bitmask of A^T
        c["rows"] = _rows(rng, R, P)
        c["gu"] = _vals(rng, (R, GH), exact, 2)
        c["y1"] = _act_out(rng, (P, GH))
        c["w1"] = _f32(rng, (GI, GH), exact, 2)
        c["bscale"] = _scales(rng, P, exact)
    elif e == "sgemm":
        M, N, K, nk = spec["M"], spec["N"], spec["K"], spec["b_is_nk"]
        c["a"] = _f32(rng, (M, K), exact)
        c["a_mask"] = _act_out(rng, (M, K)) if spec["a_mask"] else None
        b = _f32(rng, (N, K) if nk else (K, N), exact, 3)
        if not nk and spec["k_b"] and spec["k_b"] < K:
            b[spec["k_b"]:] = 1000.0                     # rows that do not exist for the kernel: junk it must not read
        c["b"] = b
        c["bias"] = _f32(rng, (N,), exact) if spec["bias"] else None
        c["ct_scale"] = _scales(rng, M, exact) if spec["ct_scale"] else None
        c["drop"], c["salt"] = spec["act"] == 2, 0x2000 + N
        c["seed"], c["seed_dev"] = SEED + K, (SEED_DEV if spec["seed_dev"] else None)
    elif e == "bias_act":
        R, C = spec["R"], spec["C"]
        c["x"] = _f32(rng, (R, C), exact)
        c["bias"] = _f32(rng, (C,), exact) if spec["bias"] else None
        c["drop"], c["salt"], c["seed"], c["seed_dev"] = bool(spec["drop"]), 0x2000 + C, SEED + C, (SEED_DEV if C == 64 else None)
    else:
        raise KeyError(e)
    if exact:
        assert_exact(c)
    return c


# ------------------------------------------------------------------------------------------------ float64 restatement
def _keep(c, R, C, mut):
    """(bool keep mask, factor) of a case's dropout site, or (None, 1)."""
    if not c.get("drop"):
        return None, 1.0
    seed = c["seed"] + (c["seed_dev"] or 0)
    return keep_mask(seed, 0 if mut == "hash_without_salt" else c["salt"], R, C, c["p"]), c["inv_keep"]


def _drop_k(b, K, nwave, mut, strided=False):
    """A copy of the 0/1 matrix b [M, K] with the k-range a defective kernel would skip zeroed."""
    b = b.astype(np.float64)
    if mut == "drop_kstep":
        b[:, 32 * ((K - 1) // 32):] = 0
    elif mut == "drop_wave":
        nsteps = cdiv(K, 32)
        if strided:                                      # rows_bwd: wave w takes the steps w, w + NWAVE, ...
            w = 1 if nsteps > 1 else 0
            for s in range(w, nsteps, nwave):
                b[:, 32 * s:32 * s + 32] = 0
        else:
            sl = [x for x in wave_slices(K, nwave) if x[1] > x[0]]
            s0, s1 = sl[1] if len(sl) > 1 else sl[0]
            b[:, 32 * s0:32 * s1] = 0
    return b


def _clamp(acc, mut):
    if mut == "clamp_last_row" and acc.shape[0] >= 2:
        acc = acc.copy()
        acc[-1] = acc[-2]
    return acc


def _out(kind, ref, bound):
    return dict(kind=kind, ref=ref, bound=bound)


def restate(c, mut=None):
    """{output name: dict(kind "f32" | "bf16", ref float64 (a bf16 output's value BEFORE its rounding), bound float64)}: every
    output the entry writes.  `mut` plants one defect (the bounds are then meaningless)."""
    return _RESTATE[c["spec"]["entry"]](c, mut)


def _r_mask_gemm(c, mut):
    s = c["spec"]
    M, K, N = s["M"], s["K"], s["N"]
    nwave = MASK_GEMM_FORM[N][1]
    x32 = c["x"] * c["bscale"][:, None] if c["bscale"] is not None else c["x"]        # f32 product, as xt_kernel's
    xs = bf16(x32)
    if mut == "round_before_scale" and c["bscale"] is not None:
        xs = bf16(c["x"]) * c["bscale"][:, None].astype(np.float64)
    b = _drop_k(c["bits"], K, nwave, mut)
    acc = _clamp(b @ xs, mut)
    rs = c["rscale"].astype(np.float64)[:, None] if c["rscale"] is not None else 1.0
    bias = c["bias"].astype(np.float64) if c["bias"] is not None else 0.0
    out = rs * (acc + bias) if mut == "rscale_after_bias" else rs * acc + bias
    mag = np.abs(rs) * (b @ np.abs(xs)) + np.abs(bias)
    work = np.zeros((N, roundup(K, 128)))
    work[:, :K] = x32.T
    return dict(out=_out("f32", out, gamma(roundup(K, 32) + nwave + 2) * mag), work=_out("bf16", work, np.zeros_like(work)))


def _act_bound(d, pre, n_mul):
    return d + n_mul * U * (np.abs(pre) + d)


def _r_l1(c, mut):
    s = c["spec"]
    M, K = s["M"], s["K"]
    b = _drop_k(c["bits"], K, 16, mut)
    y0, w1, b1 = c["y0"].astype(np.float64), c["w1"].astype(np.float64), c["b1"].astype(np.float64)
    rs = c["rscale"].astype(np.float64)[:, None]
    t = rs * _clamp(b @ y0, mut)
    a = t @ w1 + b1
    keep, ik = _keep(c, M, GH, mut)
    y = leaky(a, c["slope"])
    if keep is not None:
        y = np.where(keep, y * ik, 0.0)
    bt = gamma(roundup(K, 32) + 17) * rs * (b @ np.abs(y0))
    da = (bt @ np.abs(w1)) * (1 + gamma(16)) + gamma(16) * (np.abs(t) @ np.abs(w1) + np.abs(b1))
    dy = _act_bound(da, a, 2) * (ik if keep is not None else 1.0)
    if keep is not None:
        dy = np.where(keep, dy, 0.0)
    return dict(t=_out("f32", t, bt), y=_out("f32", y, dy), yt=_out("bf16", y.T.copy(), dy.T.copy()))


def _r_rows_fwd(c, mut):
    s = c["spec"]
    R, K, NO = s["R"], s["K"], s["NO"]
    rows = c["rows"]
    b = _drop_k(c["bits"][rows], K, 16, mut)
    y1, w2 = c["y1"].astype(np.float64), c["w2"].astype(np.float64)
    b2 = c["b2"].astype(np.float64) if c["b2"] is not None else np.zeros(NO)
    rs = c["rscale"].astype(np.float64)[rows][:, None]
    u = rs * _clamp(b @ y1, mut)
    bu = gamma(roundup(K, 32) + 17) * rs * (b @ np.abs(y1))
    parts, bp = np.zeros((4, R, NO)), np.zeros((4, R, NO))
    for q in range(4):
        blk = slice(16 * q, 16 * q + 16)
        add = b2 if (q == 0 or mut == "b2_every_part") else 0.0
        parts[q] = u[:, blk] @ w2[blk] + add
        bp[q] = (bu[:, blk] @ np.abs(w2[blk])) * (1 + gamma(16)) + gamma(16) * (np.abs(u[:, blk]) @ np.abs(w2[blk]) + np.abs(add))
    if mut == "swap_parts":
        parts[[1, 2]] = parts[[2, 1]]
    out = dict(u=_out("f32", u, bu), parts=_out("f32", parts, bp))
    if s["rs_rows"]:
        out["rs_rows"] = _out("f32", rs[:, 0].copy(), np.zeros(R))
    return out


def _r_rows_bwd(c, mut):
    s = c["spec"]
    R, P = s["R"], s["P"]
    A = c["bits"].T if mut == "mask_for_mask_t" else c["bits"]
    sel = _drop_k(A[c["rows"]].T, R, 8, mut, strided=True)                             # [P, R]: bit (k, r) = A[rows[r], k]
    gu, w1 = c["gu"].astype(np.float64), c["w1"].astype(np.float64)
    bs = c["bscale"].astype(np.float64)[:, None]
    dy1 = _clamp(sel @ gu, mut)
    m = act_mask(c["y1"], c["mask_vals"], mut)
    gs = dy1 * m
    sm = gs @ w1.T
    dt = bf16(sm) * bs if mut == "round_before_scale" else sm * bs
    bd = gamma(roundup(R, 32) + 8) * (sel @ np.abs(gu))
    dgs = _act_bound(bd, dy1, 1) * np.abs(m)
    ds = (dgs @ np.abs(w1).T) * (1 + gamma(64)) + gamma(64) * (np.abs(gs) @ np.abs(w1).T)
    ddt = _act_bound(ds, sm, 1) * np.abs(bs)
    return dict(dy1=_out("f32", dy1, bd), dtt=_out("bf16", dt.T.copy(), ddt.T.copy()))


def _r_sgemm(c, mut):
    s = c["spec"]
    M, N, K = s["M"], s["N"], s["K"]
    kb = K if (mut == "kb_ignored" or not s["k_b"]) else s["k_b"]
    a = c["a"]
    if c["a_mask"] is not None:
        a = a * act_mask(c["a_mask"], c["mask_vals"], mut).astype(np.float32)          # f32 product, as the prologue's
    a = a.astype(np.float64)
    bm = c["b"].astype(np.float64).T if s["b_is_nk"] else c["b"].astype(np.float64)  # [K, N]
    a, bm = a[:, :kb], bm[:kb]
    if mut == "drop_kstep":
        a = a.copy()
        a[:, 16 * ((kb - 1) // 16):] = 0
    bias = c["bias"].astype(np.float64) if c["bias"] is not None else np.zeros(N)
    pre = _clamp(a @ bm, mut) + bias
    d = gamma(roundup(K, 16) + 5) * (np.abs(a) @ np.abs(bm) + np.abs(bias))
    o = pre
    keep, ik = _keep(c, M, N, mut)
    if s["act"]:
        o = leaky(pre, c["slope"])
        d = _act_bound(d, pre, 1)
        if keep is not None:
            o = np.where(keep, o * ik, 0.0)
            d = np.where(keep, _act_bound(d, o / ik, 1) * ik, 0.0)
    out = {}
    if s["ct"] != "only":
        out["c"] = _out("f32" if s["c_dtype"] == F32C else "bf16", o, d)
    if s["ct"]:
        if c["ct_scale"] is not None:
            sc = c["ct_scale"].astype(np.float64)[:, None]
            v = bf16(o) * sc if mut == "round_before_scale" else o * sc
            dv = _act_bound(d, o, 1) * sc
        else:
            v, dv = o, d
        out["ct"] = _out("bf16", v.T.copy(), dv.T.copy())
    return out


def _r_bias_act(c, mut):
    s = c["spec"]
    R, C = s["R"], s["C"]
    pre = c["x"].astype(np.float64) + (c["bias"].astype(np.float64) if c["bias"] is not None else 0.0)
    y = leaky(pre, c["slope"])
    keep, ik = _keep(c, R, C, mut)
    if keep is not None:
        y = np.where(keep, y * ik, 0.0)
    d = gamma(3) * np.abs(y)
    out = dict(y=_out("f32", y, d))
    if s["y_t"]:
        out["y_t"] = _out("bf16", y.T.copy(), d.T.copy())
    return out


_RESTATE = dict(mask_gemm=_r_mask_gemm, l1=_r_l1, rows_fwd=_r_rows_fwd, rows_bwd=_r_rows_bwd, sgemm=_r_sgemm, bias_act=_r_bias_act)
# the defects an entry can have at all (the others leave its restatement unchanged)
APPLIES = dict(
    mask_gemm=("drop_kstep", "drop_wave", "clamp_last_row", "rscale_after_bias", "round_before_scale"),
    l1=("drop_kstep", "drop_wave", "clamp_last_row", "truncate", "hash_without_salt"),
    rows_fwd=("drop_kstep", "drop_wave", "clamp_last_row", "swap_parts", "b2_every_part"),
    rows_bwd=("drop_kstep", "drop_wave", "mask_for_mask_t", "clamp_last_row", "round_before_scale", "truncate", "mzero_for_negative"),
    sgemm=("drop_kstep", "clamp_last_row", "round_before_scale", "truncate", "hash_without_salt", "mzero_for_negative", "kb_ignored"),
    bias_act=("truncate", "hash_without_salt"))


def emulate(c, mut=None):
    """What a kernel with defect `mut` (None: a correct one) would leave: {name: float32 array | uint16 bf16 patterns}."""
    got = {}
    for name, o in restate(c, mut).items():
        if o["kind"] == "f32":
            got[name] = o["ref"].astype(np.float32)
        else:
            got[name] = bf16_bits(o["ref"], truncate=mut == "truncate" and name != "work")
    if c["spec"]["entry"] == "rows_fwd" and c["spec"]["family"] == "exact":
        p = got["parts"]
        got["sum"] = ((p[0] + p[1]) + p[2]) + p[3]
    return got


# ------------------------------------------------------------------------------------------------ exactness of the exact family
# the finest unit a product of an entry's operands can have: integers, scales down to 1/4, slope 1/2, inv_keep 2
UNIT = dict(mask_gemm=2.0 ** -4, l1=2.0 ** -3, rows_fwd=2.0 ** -2, rows_bwd=2.0 ** -2, sgemm=2.0 ** -3, bias_act=2.0 ** -1)


def assert_exact(c):
    """Every output's sum of |terms| in units of the entry's finest operand unit stays below 2^24, and every output is an integer
    multiple of that unit: every partial sum, in any order, is then a representable f32."""
    worst, unit = 0.0, UNIT[c["spec"]["entry"]]
    for name, o in restate(c).items():
        mag = np.abs(o["ref"])
        worst = max(worst, float(_term_magnitude(c, name).max(initial=0.0)), float(mag.max(initial=0.0)))
        q = o["ref"] / unit
        assert np.array_equal(q, np.round(q)), (c["spec"]["id"], name)
    assert worst / unit < 2.0 ** 24, (c["spec"]["id"], worst)
    c["_exact_worst"] = worst / unit
    return worst / unit


def _term_magnitude(c, name):
    """sum |terms| of output `name`: the same restatement on |operands| with every mask factor, scale and bias made positive."""
    e = c["spec"]["entry"]
    f = np.float64
    if e == "mask_gemm":
        x32 = np.abs(c["x"] * c["bscale"][:, None] if c["bscale"] is not None else c["x"]).astype(f)
        rs = c["rscale"].astype(f)[:, None] if c["rscale"] is not None else 1.0
        return rs * (c["bits"].astype(f) @ x32) + (np.abs(c["bias"]).astype(f) if c["bias"] is not None else 0.0)
    if e == "l1":
        t = c["rscale"].astype(f)[:, None] * (c["bits"].astype(f) @ np.abs(c["y0"]).astype(f))
        return t if name == "t" else (t @ np.abs(c["w1"]).astype(f) + np.abs(c["b1"]).astype(f)) * c["inv_keep"]
    if e == "rows_fwd":
        u = c["rscale"].astype(f)[c["rows"]][:, None] * (c["bits"][c["rows"]].astype(f) @ np.abs(c["y1"]).astype(f))
        if name in ("u", "rs_rows"):
            return u
        return u @ np.abs(c["w2"]).astype(f) + (np.abs(c["b2"]).astype(f) if c["b2"] is not None else 0.0)
    if e == "rows_bwd":
        dy = c["bits"][c["rows"]].T.astype(f) @ np.abs(c["gu"]).astype(f)
        if name == "dy1":
            return dy
        return (dy * max(c["mask_vals"])) @ np.abs(c["w1"]).astype(f).T * c["bscale"].astype(f)[:, None]
    if e == "sgemm":
        s = c["spec"]
        kb = s["k_b"] or s["K"]
        bm = np.abs(c["b"]).astype(f).T if s["b_is_nk"] else np.abs(c["b"]).astype(f)
        m = np.abs(c["a"]).astype(f)[:, :kb] * max(c["mask_vals"]) @ bm[:kb]
        m = (m + (np.abs(c["bias"]).astype(f) if c["bias"] is not None else 0.0)) * c["inv_keep"]
        return m * (c["ct_scale"].astype(f)[:, None] if c["ct_scale"] is not None else 1.0)
    return (np.abs(c["x"]).astype(f) + (np.abs(c["bias"]).astype(f) if c["bias"] is not None else 0.0)) * c["inv_keep"]


# ------------------------------------------------------------------------------------------------ verdicts
def _canon(bits):
    bits = np.asarray(bits, dtype=np.uint16)
    return np.where(bits == 0x8000, np.uint16(0), bits)


def verdict(c, got):
    """(ok, worst error / bound) of an entry's outputs `got` (emulate's layout).  Exact family: every f32 output equals the float64
    restatement as a value, every bf16 output its round-to-nearest-even bit pattern (the ratio is 0 or inf).  Rounding family:
    every f32 element within its bound, every bf16 element inside [bf16(ref - bound), bf16(ref + bound)]; an output whose bound
    is zero (rs_rows, the operand copy `work`) is exact in both."""
    if "_ref" not in c:
        c["_ref"] = restate(c)
    exact = c["spec"]["family"] == "exact"
    worst = 0.0
    for name, o in c["_ref"].items():
        g = np.asarray(got[name])
        if g.shape != o["ref"].shape:
            return False, float("inf")
        tight = exact or not np.any(o["bound"])
        if o["kind"] == "f32":
            g = g.astype(np.float64)
            if tight:
                r = 0.0 if np.array_equal(g, o["ref"]) else float("inf")
            else:
                err = np.abs(g - o["ref"])
                err = np.where(np.isnan(err), np.inf, err)
                with np.errstate(divide="ignore", invalid="ignore"):
                    q = np.where(o["bound"] > 0, err / o["bound"], np.where(err > 0, np.inf, 0.0))
                r = float(q.max(initial=0.0))
        elif tight:
            r = 0.0 if np.array_equal(_canon(g), _canon(bf16_bits(o["ref"]))) else float("inf")
        else:
            v = bf16_value(g)
            pad = 1e-12 * np.abs(o["ref"])                                              # float64 noise of the restatement itself
            lo, hi = bf16(o["ref"] - o["bound"] - pad), bf16(o["ref"] + o["bound"] + pad)
            inside = (v >= lo) & (v <= hi)
            # the figure reported: 0 where got is the rounding of ref itself, else the share of the bound the f32 value in front of
            # the cast needs to cross the rounding boundary between bf16(ref) and got (their midpoint) -- at most 1 inside
            near = bf16(o["ref"])
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(v == near, 0.0, np.abs((v + near) / 2 - o["ref"]) / o["bound"])
            r = float(np.where(inside, np.minimum(q, 1.0), np.inf).max(initial=0.0))
        worst = max(worst, r)
    if exact and "sum" in got:
        p = c["_ref"]["parts"]["ref"]
        worst = max(worst, 0.0 if np.array_equal(np.asarray(got["sum"]).astype(np.float64), p[0] + p[1] + p[2] + p[3]) else float("inf"))
    return worst <= 1.0, worst
