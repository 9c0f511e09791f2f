"""Reference side of the weight-gradient matrix (tests/test_gpu_wgrad_matrix.py, tests/test_host_wgrad_reference.py): the case
list as plain data, a case builder for two input families, a float64 restatement of every contract of include/mobgt_hip.h that
csrc/wgrad.hip, csrc/wgradbig.hip and csrc/hop_body.h implement, a CPU emulation of the kernels' rounding points and launch
structure with the mutants the tests must reject, and the rounding family's per-element tolerance.  CPU torch only.

Exact family: operands are integers |v| <= 3 (zeros included), mask factors {2, -0.5, 0}, integer out_bias and pre-loads.  Every
operand, masked operand, product and partial sum is a multiple of 0.25 below 2^24 * 0.25, so f32 accumulation is exact in any
order and the kernels must return the float64 result bit for bit.
Rounding family: real f32 operands with exact bf16 ties and a mask factor of 3; reference in float64 on operands rounded where
the kernels round (f32 multiply by the mask factor, then round-to-nearest-even to bf16); tolerance `bound`."""
import zlib

import torch

TILE, KSTEP, SHORT_R = 32, 32, 1024                  # csrc/wgrad_body.h:10-12
WB_TM, WB_TN, WB_KC = 128, 256, 64                   # csrc/wgradbig.hip:35
EXACT_VALS = (2.0, -0.5, 0.0)                        # m_pos, m_neg, m_zero
ROUND_VALS = (3.0, -0.5, 0.0)
U = 2.0 ** -24                                       # unit roundoff of f32

WGRAD_MUTANTS = ("drop_last_row", "drop_kstep", "drop_slab", "bias_per_split", "swap_pos_neg", "negzero_negative",
                 "mask_after_round", "truncate", "db_unmasked", "db_f32", "db_of_x_sums_g", "gm_out_ragged", "ragged_col_zeroed")
BIG_MUTANTS = ("big_drop_last_chunk", "big_colsum_skip_first")
ROUNDING_MUTANTS = ("mask_after_round", "truncate", "db_f32")      # what integers cannot see


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ launch regimes, restated
def fill_problem(R, M, N, target_wgs, nwave):
    """(tiles, splits, k_per_wg) as fill_problem gives them (csrc/wgrad_body.h:222-232)."""
    tiles = cdiv(M, TILE) * cdiv(N, TILE)
    slab = nwave * KSTEP
    splits = max(1, min(target_wgs // tiles, cdiv(R, slab)))
    k_per_wg = cdiv(cdiv(R, splits), slab) * slab
    return tiles, cdiv(R, k_per_wg), k_per_wg


def regime(spec):
    """[(nwave, tiles, splits, k_per_wg)] per problem, from the launchers of csrc/wgrad.hip: the single-problem entries aim at 512
    (8 waves) or 256 (16 waves) workgroups (:207-209), the group and the tail at 256 / n (:94, :102-103), the heterogeneous group at
    max(1024 / n, 64) with 16 waves as soon as one problem is longer than SHORT_R (:135-137, :146-148)."""
    probs, entry = spec["probs"], spec["entry"]
    n = len(probs)
    out = []
    for p in probs:
        if entry in ("multi", "multi_hop"):
            nwave = 16 if any(q["R"] > SHORT_R for q in probs) else 8
            target = max(1024 // n, 64)
        else:
            nwave = 8 if p["R"] <= SHORT_R else 16
            target = 256 // n if entry in ("group", "tail") else (512 if nwave == 8 else 256)
        out.append((nwave,) + fill_problem(p["R"], p["M"], p["N"], target, nwave))
    return out


def big_tiles(M, N):
    return cdiv(M, WB_TM) * cdiv(N, WB_TN)                        # mobgt_layer_wgrad_big_tiles, csrc/wgradbig.hip:207-210


def big_splits(R, ntiles):
    nchunk = cdiv(R, WB_KC)                                       # mobgt_layer_wgrad_big_splits, csrc/wgradbig.hip:197-205
    return min(32, max(1, min((240 + ntiles // 2) // ntiles, nchunk // 2)))


def big_S(spec):
    R = spec["probs"][0]["R"]
    nchunk = cdiv(R, WB_KC)
    S = spec["S"]
    if S == "nchunk":
        return nchunk
    if S == "rec":
        return big_splits(R, sum(big_tiles(p["M"], p["N"]) for p in spec["probs"]))
    return S


# ------------------------------------------------------------------------------------------------ the matrix
def P(R, M, N, form="bf16", gmask=False, xmask=False, db=None, gm_out=False, view=False, out_bias=False):
    """One problem: form bf16 | f32 | mixed (g bf16, x f32); db: None | "g" | "x"; view: operands are column views of wider buffers."""
    return dict(R=R, M=M, N=N, form=form, gmask=gmask, xmask=xmask, db=db, gm_out=gm_out, view=view, out_bias=out_bias)


def _pid(p):
    s = f"{p['form']}-R{p['R']}-M{p['M']}-N{p['N']}"
    for k, t in (("gmask", "gm"), ("xmask", "xm"), ("gm_out", "gout"), ("view", "view"), ("out_bias", "bias")):
        if p[k]:
            s += "-" + t
    return s + ("-db" + p["db"] if p["db"] else "")


def spec_id(spec):
    probs = spec["probs"]
    s = spec["entry"] + ("-round" if spec["family"] == "round" else "")
    if len(probs) == 1 and spec["entry"] not in ("group", "tail", "multi", "multi_hop", "big", "ops_big"):
        s += "-" + _pid(probs[0])
    else:
        Rs = sorted({p["R"] for p in probs})
        forms = sorted({p["form"] for p in probs})
        s += f"-n{len(probs)}-{'+'.join(forms)}-R{'+'.join(map(str, Rs))}-M{probs[0]['M']}-N{probs[0]['N']}"
    if spec.get("tag"):
        s += "-" + spec["tag"]
    if spec["entry"] in ("big", "ops_big"):
        s += f"-S{spec['S']}-cs{'null' if spec['colsum'] is None else ''.join(map(str, spec['colsum']))}"
        s += "-gview" if spec["gview"] else ""
    if spec.get("db_null_array"):
        s += "-dbarrnull"
    if spec.get("hop"):
        s += "-hopD{D}E{E}rt{rt}".format(**spec["hop"])
    if spec.get("tail"):
        s += "-gemm{gM}x{gN}x{gK}".format(**spec["tail"])
    return s + ("-pre" if spec["preload"] else "")


def S(entry, probs, family="exact", preload=False, **kw):
    spec = dict(entry=entry, family=family, probs=probs, preload=preload, db_null_array=False, hop=None, tail=None, tag=None)
    spec.update(kw)
    spec["id"] = spec_id(spec)
    return spec


PLAIN_R = (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 1537, 2049)
PLAIN_MN = ((2, 2), (6, 10), (30, 34), (32, 32), (34, 66), (130, 66))
GROUP_MN = ((2, 2), (6, 10), (30, 34), (32, 32), (34, 66), (130, 66), (66, 34), (10, 6))
BIG_R = (1, 63, 64, 65, 128, 129, 200)
BIG_MN = tuple((m, n) for m in (8, 128, 136) for n in (8, 256, 264))
HOP_D, HOP_E = (1, 3, 20), (1, 5, 256)
TAIL_GEMM = tuple((gM, gN, gK) for gM in (1, 33, 100) for gN in (8, 40) for gK in (32, 96))


def _group_probs(n, R, form, db_mode, shift=0):
    """n problems over the same R rows with different M, N and pitches; db_mode "null": no db anywhere, "some": every third null."""
    out = []
    for q in range(n):
        M, N = GROUP_MN[(q + shift) % len(GROUP_MN)]
        out.append(P(R, M, N, form, db=None if db_mode == "null" or q % 3 == 1 else "g", view=q % 2 == 0))
    return out


def _multi_probs(kind, n=None):
    if kind == "long":          # 40, 1024, 1025 and 2049 rows together: the short problems run in 16-wave workgroups
        return [P(40, 6, 10, "bf16", db="g", view=True), P(1024, 34, 66, "f32", gmask=True, db="g"),
                P(1025, 30, 34, "f32", xmask=True, db="x", view=True), P(2049, 130, 66, "bf16"),
                P(33, 32, 32, "f32", gmask=True, xmask=True, db="x")]
    if kind == "short":         # every problem <= SHORT_R: 8-wave workgroups
        return [P(40, 6, 10, "f32", gmask=True, xmask=True, db="x", view=True), P(300, 34, 66, "bf16", db="g"),
                P(1024, 30, 34, "f32", db="g"), P(257, 2, 2, "f32", xmask=True, view=True)]
    if kind == "one":
        return [P(7, 6, 10, "f32", gmask=True, db="g")]
    rows = (9, 257, 1025, 33, 600) if kind == "many16" else (9, 257, 1024, 33, 600)
    out = []
    for q in range(n):
        M, N = GROUP_MN[q % len(GROUP_MN)]
        f32 = q % 2 == 1
        out.append(P(rows[q % 5], M, N, "f32" if f32 else "bf16", gmask=f32 and q % 4 == 1, xmask=f32 and q % 8 >= 3,
                     db=(None, "g", "x")[q % 3], view=q % 3 == 0))
    return out


def matrix_specs():
    specs = []
    # ---- mobgt_linear_wgrad
    for form in ("bf16", "f32"):
        for iR, R in enumerate(PLAIN_R):
            for iS, (M, N) in enumerate(PLAIN_MN):
                k = iR * len(PLAIN_MN) + iS
                specs.append(S("plain", [P(R, M, N, form, db="g" if k % 2 == 0 else None, view=k % 3 == 0)], preload=(k // 2) % 2 == 0))
    specs.append(S("plain", [P(300, 736, 736, "bf16", db="g")], preload=True))          # 529 tiles > 512: one split
    specs.append(S("plain", [P(1100, 544, 544, "f32", db="g", view=True)]))             # 289 tiles > 256: one split
    # ---- _masked
    k = 0
    for R in (33, 1024, 1025):
        for gm, xm in ((True, False), (False, True), (True, True)):
            for M, N in ((34, 10), (34, 66), (130, 66)):
                specs.append(S("masked", [P(R, M, N, "f32", gmask=gm, xmask=xm, db=("g", "x", None)[k % 3], gm_out=gm and k % 4 != 3,
                                            view=k % 2 == 0)], preload=k % 2 == 1 or k % 6 == 0))
                k += 1
    # ---- _bias (dw is documented as zero on entry)
    for form in ("bf16", "f32"):
        for R, M, N in ((300, 6, 10), (1025, 34, 66), (31, 30, 34), (2049, 2, 2)):
            specs.append(S("bias", [P(R, M, N, form, out_bias=True, view=R == 1025)]))
    specs.append(S("bias", [P(300, 736, 730, "bf16", out_bias=True)]))                  # 529 tiles > 512: one split of two slabs
    # ---- _mixed (dw and db_x documented as zero on entry)
    for R in (33, 1025):
        for M, N in ((6, 10), (34, 66)):
            for db in ("x", None):
                specs.append(S("mixed", [P(R, M, N, "mixed", db=db, view=(M == 6) == (db is None))]))
    # ---- _group
    k = 0
    for n in (1, 4, 32):
        for R in (300, 1025):
            for db_mode in ("null", "some"):
                for form in ("bf16", "f32"):
                    specs.append(S("group", _group_probs(n, R, form, db_mode, shift=k), preload=k % 2 == 0,
                                   db_null_array=db_mode == "null"))
                    k += 1
    # ---- _multi
    for k, kind in enumerate(("long", "short", "one", "many16", "many8")):
        for pre in (False, True):
            specs.append(S("multi", _multi_probs(kind, 32 if kind == "many16" else 7), preload=pre, tag=kind))
    # ---- _multi_hop
    k = 0
    for D in HOP_D:
        for E in HOP_E:
            for rt in (0, 1):
                kind = ("long", "short", "one")[k % 3] if k % 4 else ("many16", "many8")[(k // 4) % 2]
                specs.append(S("multi_hop", _multi_probs(kind, 5), preload=k % 2 == 0, hop=dict(D=D, E=E, rt=rt), tag=kind))
                k += 1
    # ---- mobgt_layer_backward_tail
    for k, (gM, gN, gK) in enumerate(TAIL_GEMM):
        n, R = (1, 4, 32)[k % 3], (300, 1024)[k % 2]
        specs.append(S("tail", _group_probs(n, R, ("bf16", "f32")[(k // 2) % 2], ("some", "null")[(k // 3) % 2], shift=k),
                       preload=k % 2 == 0, db_null_array=(k // 3) % 2 == 1, tail=dict(gM=gM, gN=gN, gK=gK)))
    # ---- rounding family
    for R in (9, 33, 257):
        for M, N in ((6, 10), (34, 66)):
            specs.append(S("plain", [P(R, M, N, "f32", db="g", view=M == 6)], family="round"))
            specs.append(S("masked", [P(R, M, N, "f32", gmask=True, xmask=True, db="g", gm_out=True, view=M == 34)], family="round"))
            specs.append(S("masked", [P(R, M, N, "f32", xmask=True, db="x")], family="round"))
            specs.append(S("mixed", [P(R, M, N, "mixed", db="x", view=M == 6)], family="round"))
    # ---- mobgt_layer_wgrad_big
    k = 0
    for R in BIG_R:
        nchunk = cdiv(R, WB_KC)
        for s in (1, 2, "nchunk", "rec"):
            if s == 2 and nchunk < 2:
                continue
            n = (1, 2, 4)[k % 3]
            probs = [P(R, *BIG_MN[(2 * k + q) % len(BIG_MN)]) for q in range(n)]
            colsum = (None, [0], [n // 2], list(range(n)))[k % 4]
            specs.append(S("big", probs, preload=k % 2 == 0, S=s, colsum=colsum, gview=k % 2 == 1))
            k += 1
    specs.append(S("ops_big", [P(129, 136, 264), P(129, 8, 256), P(129, 128, 8)], S="rec", colsum=[1], gview=False))
    return specs


# ------------------------------------------------------------------------------------------------ case builder
def _gen(spec, salt):
    return torch.Generator().manual_seed(zlib.crc32((spec["id"] + "/" + salt).encode()))


def _ints(gen, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=gen).float()


def _reals(gen, shape):
    """Real f32 values, a quarter of them exact bf16 ties (1 + 2^-8, 1 + 3 2^-8, negated, scaled by 2^-2 .. 2^2), some zeros."""
    v = torch.randn(shape, generator=gen)
    tie = (1.0 + (1 + 2 * torch.randint(0, 2, shape, generator=gen)).float() * 2.0 ** -8)
    tie = tie * (2 * torch.randint(0, 2, shape, generator=gen) - 1).float() * 2.0 ** torch.randint(-2, 3, shape, generator=gen).float()
    r = torch.rand(shape, generator=gen)
    v = torch.where(r < 0.25, tie, v)
    return torch.where(r > 0.95, torch.zeros(()), v)


def _mask(gen, shape):
    """An activation output: positive, negative, +0.0 and -0.0 entries (the first four entries are one of each)."""
    kinds = torch.tensor([1.5, -2.0, 0.0, -0.0])
    m = kinds[torch.multinomial(torch.tensor([0.4, 0.4, 0.1, 0.1]), shape[0] * shape[1], True, generator=gen)]
    k = min(4, m.numel())
    m[:k] = kinds[:k]
    return m.reshape(shape)


def rne(v):
    return v.bfloat16().float()


def build_case(spec):
    """CPU tensors of a spec: per problem g [R, M], x [R, N] (f32 holding the values; bf16 forms hold bf16-representable ones),
    gmask, xmask, mask_vals, out_bias, dw0, db0 (the destinations' contents on entry); hop: dtab, enc, w; tail: a, b, c0."""
    exact = spec["family"] == "exact"
    case = dict(spec=spec, probs=[])
    for q, p in enumerate(spec["probs"]):
        gen = _gen(spec, str(q))
        R, M, N = p["R"], p["M"], p["N"]
        g = _ints(gen, (R, M), 3) if exact else _reals(gen, (R, M))
        x = _ints(gen, (R, N), 3) if exact else _reals(gen, (R, N))
        if p["form"] in ("bf16", "mixed"):
            g = rne(g)
        if p["form"] == "bf16":
            x = rne(x)
        ndb = {None: 0, "g": M, "x": N}[p["db"]]
        pre = spec["preload"]
        case["probs"].append(dict(
            p, g=g, x=x, gmask=_mask(gen, (R, M)) if p["gmask"] else None, xmask=_mask(gen, (R, N)) if p["xmask"] else None,
            mask_vals=EXACT_VALS if exact else ROUND_VALS, bias=_ints(gen, (N,), 5) if p["out_bias"] else None,
            dw0=_ints(gen, (M, N), 5) if pre else torch.zeros(M, N),
            db0=(_ints(gen, (ndb,), 5) if pre else torch.zeros(ndb)) if ndb else None))
    if spec.get("hop"):
        gen = _gen(spec, "hop")
        D, E = spec["hop"]["D"], spec["hop"]["E"]
        case["hop"] = dict(dtab=_ints(gen, (D, E, 8), 2), enc=_ints(gen, (E, 8), 2), w=_ints(gen, (D, 8, 8), 2))
    if spec.get("tail"):
        gen = _gen(spec, "tail")
        t = spec["tail"]
        case["tail"] = dict(a=_ints(gen, (t["gM"], t["gK"]), 3), b=_ints(gen, (t["gK"], t["gN"]), 3), c0=_ints(gen, (t["gM"], t["gN"]), 5))
    return case


# ------------------------------------------------------------------------------------------------ operands as the kernels see them
def mask_factor(mask, vals, mut=None):
    pos, neg, zer = vals
    if mut == "swap_pos_neg":
        pos, neg = neg, pos
    f = torch.where(mask > 0, torch.tensor(pos), torch.where(mask < 0, torch.tensor(neg), torch.tensor(zer)))
    if mut == "negzero_negative":
        f = torch.where((mask == 0) & torch.signbit(mask), torch.tensor(neg), f)
    return f.float()


def _round(v, mut):
    if mut == "truncate":
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return rne(v)


def operands(p, mut=None):
    """(g^ [R, M], x^ [R, N], masked g in f32 or None, db's source) of a built problem: the bf16 values that reach the matrix
    cores.  An f32 operand is multiplied by its mask factor in f32, then rounded to nearest even (wgrad_body.h pack_pair_masked)."""
    def one(v, mask, f32):
        if not f32:
            return v, v
        m32 = v * mask_factor(mask, p["mask_vals"], mut) if mask is not None else v
        if mask is not None and mut == "mask_after_round":
            return m32, _round(_round(v, None) * mask_factor(mask, p["mask_vals"]), None)
        return m32, _round(m32, mut)
    g32, gh = one(p["g"], p["gmask"], p["form"] == "f32")
    x32, xh = one(p["x"], p["xmask"], p["form"] in ("f32", "mixed"))
    src = None
    if p["db"] is not None:
        of_x = p["db"] == "x"
        src = xh if of_x else gh
        if mut == "db_unmasked" and p["form"] != "bf16":
            src = _round(p["x"] if of_x else p["g"], None)
        elif mut == "db_f32":
            src = x32 if of_x else g32
        elif mut == "db_of_x_sums_g" and of_x:          # g's column sums land in the [N] destination
            k = min(p["M"], p["N"])
            src = torch.zeros_like(xh)
            src[:, :k] = gh[:, :k]
    return gh, xh, (g32 if p["gmask"] is not None else None), src


# ------------------------------------------------------------------------------------------------ float64 restatement
def reference(case):
    """Per problem dict(dw, db, gm) in float64 (db / gm None where the problem has none): include/mobgt_hip.h's contracts."""
    out = []
    for p in case["probs"]:
        gh, xh, gm, src = operands(p)
        dw = gh.double().t() @ xh.double() + p["dw0"].double()
        if p["bias"] is not None:
            dw = dw + p["bias"].double()[None, :]
        out.append(dict(dw=dw, db=src.double().sum(0) + p["db0"].double() if src is not None else None,
                        gm=gm.double() if gm is not None and p["gm_out"] else None))
    return out


def bound(case):
    """Per problem dict(dw, db): (R + 64) 2^-24 (|g^|^T |x^|) -- the forward-error bound of an f32 sum of R exact products in any
    order, 64 further additions for the cross-wave, cross-split and atomic ones (the destination's entry value and out_bias are
    summands) -- and its analogue for the column sums."""
    out = []
    for p in case["probs"]:
        gh, xh, _, src = operands(p)
        k = (p["R"] + 64) * U
        mag = gh.double().abs().t() @ xh.double().abs() + p["dw0"].double().abs()
        if p["bias"] is not None:
            mag = mag + p["bias"].double().abs()[None, :]
        out.append(dict(dw=k * mag, db=k * (src.double().abs().sum(0) + p["db0"].double().abs()) if src is not None else None))
    return out


def tail_reference(case):
    t = case["tail"]
    return t["c0"].double() + t["a"].double() @ t["b"].double()


def hop_reference(case):
    """(d_enc [E, 8], d_w [D, 8, 8]) in float64; fp16_roundtrip rounds operands and results to fp16 (csrc/hop_body.h)."""
    h = case["hop"]
    rt = case["spec"]["hop"]["rt"]
    r = (lambda v: v.half().double()) if rt else (lambda v: v.double())
    dtab, enc, w = r(h["dtab"]), r(h["enc"]), r(h["w"])
    d_w = torch.einsum("ek,deh->dkh", enc, dtab)
    d_enc = torch.einsum("deh,dkh->ek", dtab, w)
    d_enc[0] = 0
    return r(d_enc.float()), r(d_w.float())


def big_ranges(R, S_):
    nchunk = cdiv(R, WB_KC)                                       # csrc/wgradbig.hip:74
    return [(s * nchunk // S_, (s + 1) * nchunk // S_) for s in range(S_)]


def big_reference(case):
    """Per job dict(sum = G^T X, colsum = entry value + column sums of G or None) in float64."""
    cs = case["spec"]["colsum"]
    out = []
    for q, p in enumerate(case["probs"]):
        on = cs is not None and q in cs
        out.append(dict(sum=p["g"].double().t() @ p["x"].double(),
                        colsum=p["g"].double().sum(0) + big_colsum0(case, q).double() if on else None))
    return out


def big_colsum0(case, q):
    p = case["probs"][q]
    if not case["spec"]["preload"]:
        return torch.zeros(p["M"])
    return _ints(_gen(case["spec"], f"cs{q}"), (p["M"],), 5)


# ------------------------------------------------------------------------------------------------ emulation and mutants
def emulate(case, mut=None):
    """The kernels' results as f32 tensors, computed on the CPU with their rounding points and launch structure (splits, slabs,
    chunks); `mut` plants one defect.  wgrad entries: per problem dict(dw, db, gm) (gm: NaN where nothing was written);
    big: per job dict(parts [S, M, N], colsum)."""
    spec = case["spec"]
    if spec["entry"] in ("big", "ops_big"):
        return _emulate_big(case, mut)
    out = []
    for p, (nwave, _, splits, k_per_wg) in zip(case["probs"], regime(spec)):
        R, M, N = p["R"], p["M"], p["N"]
        gh, xh, gm, src = operands(p, mut)
        dw = p["dw0"].clone()
        db = p["db0"].clone() if src is not None else None
        slab = nwave * KSTEP
        for s in range(splits):
            k0, k1 = s * k_per_wg, min(R, (s + 1) * k_per_wg)
            rows = torch.arange(k0, k1)
            if mut == "drop_last_row":
                rows = rows[rows != R - 1]
            elif mut == "drop_kstep" and s == 0:
                lo = KSTEP if R > KSTEP else 0
                rows = rows[(rows < lo) | (rows >= lo + KSTEP)]
            elif mut == "drop_slab" and s == 0 and splits > 1:
                rows = rows[rows < k1 - slab]
            acc = gh[rows].t() @ xh[rows]
            if p["bias"] is not None and (s == 0 or mut == "bias_per_split"):
                acc = acc + p["bias"][None, :]
            if mut == "ragged_col_zeroed" and N % TILE:
                acc[:, N - N % TILE:] = 0
            dw += acc
            if src is not None:
                db += src[rows].sum(0)
        gout = None
        if gm is not None and p["gm_out"]:
            gout = gm.clone()
            if mut == "gm_out_ragged" and N % TILE:          # written from the LAST tile column, whose lanes beyond N load nothing
                col = torch.arange(M) % TILE
                gout[:, col - col % 2 >= N % TILE] = float("nan")
        out.append(dict(dw=dw, db=db, gm=gout))
    return out


def _emulate_big(case, mut):
    spec = case["spec"]
    S_ = big_S(spec)
    out = []
    for q, p in enumerate(case["probs"]):
        R = p["R"]
        on = spec["colsum"] is not None and q in spec["colsum"]
        parts = torch.zeros(S_, p["M"], p["N"])
        cs = big_colsum0(case, q).clone() if on else None
        for s, (c0, c1) in enumerate(big_ranges(R, S_)):
            hi = c1 - 1 if (mut == "big_drop_last_chunk" and s == 0) else c1
            rows = torch.arange(c0 * WB_KC, min(R, hi * WB_KC))
            parts[s] = p["g"][rows].t() @ p["x"][rows]
            if on:
                lo = c0 + 1 if (mut == "big_colsum_skip_first" and s == 0) else c0
                cs += p["g"][lo * WB_KC:min(R, c1 * WB_KC)].sum(0)
        out.append(dict(parts=parts, colsum=cs))
    return out


# ------------------------------------------------------------------------------------------------ verdicts
def _ratio(got, ref, bnd):
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.tensor(float("inf"), dtype=torch.float64), err)
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.tensor(float("inf"), dtype=torch.float64), err))
    return float(r.max()) if r.numel() else 0.0


def verdict(case, got):
    """(ok, worst error / bound) of wgrad results `got` (emulate's layout).  Exact family: ok means bit equality with the float64
    restatement (the ratio is 0 or inf).  Rounding family: ok means every element within `bound`; the masked g is exact in both."""
    if "_ref" not in case:
        case["_ref"] = reference(case)
        case["_bound"] = bound(case) if case["spec"]["family"] == "round" else None
    worst = 0.0
    for q, (o, r) in enumerate(zip(got, case["_ref"])):
        for k in ("dw", "db", "gm"):
            if r[k] is None:
                continue
            if case["_bound"] is None or k == "gm":
                worst = max(worst, 0.0 if torch.equal(o[k].double(), r[k]) else float("inf"))
            else:
                worst = max(worst, _ratio(o[k], r[k], case["_bound"][q][k]))
    return worst <= 1.0, worst


def big_verdict(case, got):
    """Exact family only: every slice equals the emulated range product bit for bit, their sum and the column sums the reference."""
    if "_ref" not in case:
        case["_ref"], case["_emu"] = big_reference(case), emulate(case)
    ok = True
    for o, r, e in zip(got, case["_ref"], case["_emu"]):
        ok &= not bool(torch.isnan(o["parts"]).any()) and torch.equal(o["parts"], e["parts"])
        ok &= torch.equal(o["parts"].double().sum(0), r["sum"])
        if r["colsum"] is not None:
            ok &= torch.equal(o["colsum"].double(), r["colsum"])
    return ok
