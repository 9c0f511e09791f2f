"""A float64 restatement of the attention-bias assembly (include/mobgt_hip.h: mobgt_build_bias, mobgt_build_bias_bwd,
mobgt_bias_pack; oracle/model_oracle.py: assemble_bias), the case builders of tests/test_gpu_bias_matrix.py, an emulation with
planted defects and the verdicts.  Nothing here is derived from csrc/bias.hip except `matrix_specs`, which restates the
CONDITIONS of its dispatch (launch_build, launch_build_bwd, DISPATCH_IDX) to name the form a case reaches.

Forward [G,H,T,T], T = N + 1 (token 0 = graph token):
    every element 2 attn_bias;  rows >= 1, column 0: + vdist[h];
    rows, columns >= 1: + rel_table[rel_pos] (+ poi_table[poi_pos]) + (sum_{d<D} mean_f hop_table[d, edge_input[..,d,f]]) / spd
    spd: 0 -> 1, k > 1 -> k - 1, clamped to [0, D] when D > 0.   Packed: [G,H,T,ld], columns [T,ld) = -inf, and the transpose.
Backward: entries with attn_bias = -inf and row 0 of dBias carry nothing; d_vdist[h] += sum_{i>=1} dB[g,h,i,0];
    d_rel[rel_pos] += dB skipping key 0 (d_poi likewise);  d_hop[d, e] += dB / (F spd) for every d < D and f INCLUDING e = 0;
    bf16 slices are summed first.  The four tables are ACCUMULATED into.

Two input families.  EXACT: tables, vdist multiples of 2^-6, dBias entries k/8 with |k| <= K, rel_pos among the values whose divisor
is a power of two, F in {1, 2, 4}: every product, fixed-point conversion, bf16 split and partial sum is exact, so the device must
return the reference's bits (`exact_condition` asserts sum |addend| / granule < 2^24 per table).  ROUNDING: Gaussian tables and
gradients, every rel_pos, F = 3; bounds from u = 2^-24 and the documented rounding points (`forward_bound`, `backward_bound`),
never looser than the gates of tests/test_gpu_kernels.py."""
import zlib

import numpy as np
import torch

U = 2.0 ** -24
F64 = torch.float64
SENT = -12345.0
IDX = {"i64": torch.int64, "i32": torch.int32, "i16": torch.int16, "u8": torch.uint8}
OUT = {"f32": torch.float32, "bf16": torch.bfloat16}
NEG_INF = float("-inf")
LDS_REL, LDS_POI, HOP_LDS_ROWS, TABL = 512, 1024, 16, 128          # the caps named in the header comments of csrc/bias.hip

DEFAULTS = dict(G=1, N=7, H=8, D_in=4, D=None, F=1, n_rel=40, n_poi=24, n_edge=24, ldq=32, idx="i16", edge="u8", ragged=False,
                hop="path", big_ids=False, max_div=16, out="f32", bias_t=True, db="f32", L=1, gap=0, special=None, wg=None,
                tag="")


def spec(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    if s["D"] is None:
        s["D"] = s["D_in"]
    if s["db"] == "f32":
        s["L"] = 1                                    # (one f32 buffer already summed over the layers: n_slices is ignored)
    s["T"] = s["N"] + 1
    s["ld"] = -(-s["T"] // s["ldq"]) * s["ldq"]
    return s


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def pairs(s):
    return s["G"] * s["T"] * s["T"]


def fwd_form(s):
    if s["H"] == 8:
        return "long" if pairs(s) >= 2 ** 20 else "short8"
    return "short4"


def fwd_edge_path(s):
    if s["D"] == 0:
        return "noedge"
    if s["edge"] == "u8" and s["H"] == 8 and s["F"] == 1 and s["D"] <= 20 and s["D_in"] % 4 == 0:
        return "dwords"
    return "loop"


def bwd_form(s):
    hopmm = s["D"] > 0 and s["F"] == 1 and s["H"] == 8 and s["D"] <= 20
    if hopmm:
        return "mfma8" if pairs(s) >= 2 ** 20 else "mfma4"
    return "plain8" if s["H"] == 8 else "plain4"


def bwd_id_path(s):
    if bwd_form(s).startswith("mfma"):
        return ("dwords" if s["D_in"] % 4 == 0 else "bytes") if s["edge"] == "u8" else "ids"
    return "noedge" if s["D"] == 0 else "loop"


def spec_id(s, cus=256):
    T = s["T"]
    if s["dir"] == "fwd":
        form, tail = fwd_form(s), "%s-%s%s" % (s["out"], fwd_edge_path(s), "" if s["bias_t"] else "-nobt")
    else:
        form = bwd_form(s)
        units = -(-T // 64) * -(-T // (8 if form == "mfma8" else 4)) * s["G"]
        walk = units > (min(cus, 256) if form == "mfma8" else 768)
        tail = "%s-L%d%s-%s%s" % (s["db"], s["L"], "g" if s["gap"] else "", bwd_id_path(s), "-walk" if walk else "")
        if s["special"]:
            tail += "-" + s["special"]
        if s["wg"] is not None:
            tail += "-wg%d" % s["wg"]
    return "%s-%s-H%d-%s%s-G%dN%dld%d-D%din%dF%d-r%dp%de%d%s%s%s" % (
        s["dir"], form, s["H"], s["idx"], s["edge"], s["G"], s["N"], s["ld"], s["D"], s["D_in"], s["F"], s["n_rel"], s["n_poi"],
        s["n_edge"], "-rag" if s["ragged"] else "", "-" + tail, ("-" + s["tag"]) if s["tag"] else "")


def for_family(s, family):
    """The spec as a family runs it: the EXACT family needs a power-of-two F, so a case with F = 3 runs there with F = 4."""
    return dict(s, F=4) if family == "exact" and s["F"] == 3 else s


def form_of(s):
    return "%s/%s" % (s["dir"], fwd_form(s) if s["dir"] == "fwd" else bwd_form(s))


def matrix_specs(cus=256):
    """Every case of the GPU matrix, each a `spec` with dir = 'fwd' / 'bwd'."""
    out = []

    def fwd(**kw):
        out.append(dict(spec(**kw), dir="fwd"))

    def bwd(**kw):
        out.append(dict(spec(**kw), dir="bwd"))

    # ---- short forward, H in {4, 8}: every N around the 32-wide tile, G in {1, 3}, ld rounded to 32 and 64
    for H in (4, 8):
        for i, N in enumerate((1, 7, 31, 32, 63, 64, 65)):
            fwd(H=H, N=N, G=(1, 3)[i % 2], ldq=(32, 64)[(i // 2) % 2], out=("f32", "bf16")[i % 2], bias_t=i % 3 != 2,
                n_poi=(24, 0)[(i // 2) % 2], ragged=i % 2 == 1, D_in=4 if H == 8 else 3, F=1 if H == 8 else 2, edge="u8")
        fwd(H=H, N=33, G=3, ldq=64, out="bf16", bias_t=False, n_poi=0, ragged=True)
        fwd(H=H, N=65, G=1, ldq=64, out="f32", ragged=True)
    # ---- edge paths, forward (short H = 8)
    for D, D_in in ((20, 20), (3, 4), (5, 8), (4, 20)):
        fwd(N=33, G=3, D=D, D_in=D_in, ragged=True)                              # uint8 ids as dwords, all ids < 16
        fwd(N=33, G=3, D=D, D_in=D_in, big_ids=True, n_edge=40, out="bf16")      # ... a few ids in [16, 40)
    fwd(N=33, G=3, D=20, D_in=21, n_edge=40, big_ids=True)                       # the plain loop: D_in % 4 != 0
    fwd(N=33, G=3, D=21, D_in=21, n_edge=40, big_ids=True, max_div=16)           # D > 20
    for F in (2, 3):
        fwd(N=33, G=3, D=3, D_in=4, F=F, hop="random", n_edge=40)
    fwd(N=33, G=3, D=3, D_in=4, idx="i32", edge="i32", n_edge=300, hop="random")
    fwd(N=33, G=3, D=3, D_in=4, idx="i64", edge="i64", n_edge=300, hop="random")
    fwd(N=33, G=3, D=0, D_in=4, ragged=True)                                     # D = 0: edge_input dropped
    # ---- dtype pairs, short, both directions
    for idx, edge in (("i64", "i64"), ("i64", "u8"), ("i32", "i32"), ("i16", "u8"), ("i32", "u8")):
        for H in (4, 8):
            fwd(H=H, N=37, G=3, idx=idx, edge=edge, ragged=True, out="bf16" if H == 4 else "f32", tag="pair")
            bwd(H=H, N=37, G=3, idx=idx, edge=edge, ragged=True, db="bf16" if H == 8 else "f32", L=2, tag="pair")
    # ---- long forward (H = 8, G T^2 >= 2^20) and its boundary
    fwd(G=16, N=254, D_in=4, out="bf16", n_rel=600, n_poi=1500, ragged=True, max_div=4, tag="boundary")      # stays short
    fwd(G=16, N=255, D_in=4, out="bf16", n_rel=600, n_poi=1500, ragged=True, max_div=4)
    fwd(G=16, N=255, D_in=4, out="f32", n_rel=600, n_poi=1500, ragged=True, max_div=4)
    fwd(G=16, N=255, D_in=4, out="bf16", bias_t=False, n_rel=40, n_poi=0, max_div=4)
    fwd(G=17, N=250, D_in=4, D=3, out="bf16", n_rel=600, n_poi=1500, ragged=True, big_ids=True, n_edge=40, max_div=4)
    fwd(G=17, N=250, D_in=4, D=3, out="f32", n_rel=40, n_poi=24, ragged=True, max_div=4)
    fwd(G=15, N=269, D_in=4, out="bf16", n_rel=600, n_poi=1500, ragged=True, max_div=4)                      # ld = 288: odd nt
    fwd(G=15, N=269, D_in=4, out="f32", bias_t=False, n_rel=600, n_poi=0, max_div=4)
    fwd(G=16, N=255, D_in=20, out="bf16", n_rel=600, n_poi=1500, ragged=True, big_ids=True, n_edge=40, max_div=4)
    fwd(G=16, N=255, D_in=4, idx="i64", edge="i64", out="bf16", n_rel=600, n_poi=1500, n_edge=300, max_div=4, tag="pair")
    fwd(G=16, N=255, D_in=4, F=2, hop="random", out="f32", n_rel=40, max_div=4)
    # ---- backward, long MFMA form (8 waves, fixed point)
    for D, D_in in ((3, 4), (20, 20)):
        bwd(G=16, N=255, D=D, D_in=D_in, db="f32", n_rel=600, n_poi=1500, n_edge=40, big_ids=True, ragged=True, max_div=4)
        bwd(G=16, N=255, D=D, D_in=D_in, db="bf16", L=1, n_rel=600, n_poi=1500, n_edge=40, big_ids=True, ragged=True, max_div=4)
    bwd(G=16, N=255, D=3, D_in=4, db="bf16", L=2, gap=4096, n_rel=600, n_poi=1500, n_edge=40, big_ids=True, ragged=True, max_div=4)
    bwd(G=17, N=250, D=3, D_in=4, db="bf16", L=2, n_rel=40, n_poi=0, ragged=True, max_div=4)
    bwd(G=15, N=269, D=3, D_in=4, db="f32", n_rel=600, n_poi=1500, ragged=True, max_div=4)
    bwd(G=16, N=255, D=4, D_in=4, db="bf16", L=2, idx="i64", edge="i64", n_rel=600, n_poi=1500, n_edge=300, max_div=4, tag="pair")
    for special in ("lonely", "outlier", "nan"):
        bwd(G=16, N=255, D=3, D_in=4, db="bf16", L=2, n_rel=600, n_poi=1500, n_edge=40, big_ids=True, max_div=4, special=special)
    bwd(G=16, N=255, D=3, D_in=4, db="f32", n_rel=600, n_poi=1500, n_edge=40, big_ids=True, ragged=True, max_div=4, wg=3)
    # ---- backward, short MFMA form (4 waves)
    for i, N in enumerate((1, 7, 31, 63, 64, 65)):
        bwd(N=N, G=(1, 3)[i % 2], ldq=(32, 64)[(i // 2) % 2], db=("f32", "bf16")[i % 2], L=(1, 3)[i % 2], n_poi=(24, 0)[(i // 2) % 2],
            ragged=i % 2 == 1, big_ids=True, n_edge=40)
    bwd(N=33, G=3, D=5, D_in=5, big_ids=True, n_edge=40, ragged=True)                           # uint8 ids byte by byte
    bwd(N=33, G=3, D=20, D_in=20, big_ids=True, n_edge=40, db="bf16", L=13)                     # 13 slices: the 12-in-flight loop
    bwd(N=33, G=3, D=3, D_in=4, idx="i32", edge="i32", n_edge=300, big_ids=True)                # hop_id[]
    bwd(N=33, G=3, D=3, D_in=4, n_rel=600, n_poi=1500, db="bf16", L=2, gap=4096)                # keys past the LDS caps
    bwd(G=16, N=254, D=3, D_in=4, n_rel=600, n_poi=1500, db="bf16", L=2, ragged=True, max_div=4, tag="boundary")   # > 768 units
    bwd(N=33, G=3, D=3, D_in=4, big_ids=True, n_edge=40, special="nan")                          # a NaN beside the one-hot product
    # ---- backward, H = 8 without MFMA
    for F in (2, 3):
        bwd(N=33, G=3, D=3, D_in=4, F=F, hop="random", n_edge=40, db=("f32", "bf16")[F - 2], L=F)
    bwd(N=33, G=3, D=21, D_in=21, n_edge=40, big_ids=True, ragged=True, tag="clean")            # clean hop lists: the shortcut
    bwd(N=33, G=3, D=21, D_in=21, n_edge=40, big_ids=True, hop="midzero", db="bf16", L=2)       # a zero before a non-zero id
    bwd(N=33, G=3, D=0, D_in=4, ragged=True)
    bwd(N=33, G=3, D=0, D_in=4, n_rel=600, n_poi=1500, db="bf16", L=2)
    bwd(G=16, N=255, D=1, D_in=1, F=2, hop="random", db="bf16", L=2, n_rel=600, n_poi=1500, ragged=True, max_div=4)   # long, 4 waves
    # ---- backward, H = 4
    for i, N in enumerate((1, 7, 33, 64, 65)):
        bwd(H=4, N=N, G=(1, 3)[i % 2], F=(1, 2)[i % 2], hop=("path", "random")[i % 2], db=("f32", "bf16")[(i // 2) % 2], L=2,
            ldq=(32, 64)[i % 2], n_poi=(24, 0)[(i // 2) % 2], ragged=True, n_edge=40, big_ids=True)
    bwd(H=4, N=33, G=3, F=1, D=3, D_in=4, n_rel=600, n_poi=1500, db="bf16", L=2)
    seen = set()
    for s in out:
        s["id"] = spec_id(s, cus)
        assert s["id"] not in seen, s["id"]
        seen.add(s["id"])
    return out


# ------------------------------------------------------------------------------------------------ the operation, float64 (torch)
def divisor(rel_pos, D, defect=None):
    s = rel_pos.long()
    s = torch.where(s == 0, torch.ones_like(s), s)
    if defect != "divisor k instead of k-1":
        s = torch.where(s > 1, s - 1, s)
    if D > 0 and defect != "clamp to D missing":
        s = s.clamp(0, D)
    return s


def forward(inp, D, defect=None):
    """-> (bias [G,H,T,T] float64, magnitude of its addends [G,H,T,T]: the sum of |.| the forward bound is stated in)."""
    ab = inp["attn_bias"].to(F64)
    G, T = ab.shape[:2]
    H, F = inp["vdist"].shape[0], inp["edge_input"].shape[4]
    base = ab if defect == "attn_bias counted once" else 2 * ab
    out = base[:, None].repeat(1, H, 1, 1)
    mag = out.abs()
    vd = inp["vdist"].to(F64)
    out[:, :, 1:, 0] += vd[None, :, None]
    mag[:, :, 1:, 0] += vd.abs()[None, :, None]
    if defect == "vdist added on row 0":
        out[:, :, 0, 0] += vd[None]
    pair = inp["rel_table"].to(F64)[inp["rel_pos"].long()]                         # [G,N,N,H]
    pmag = pair.abs()
    if inp["poi_pos"] is not None:
        row = inp["poi_table"].to(F64)[inp["poi_pos"].long()]
        pair, pmag = pair + row, pmag + row.abs()
    if D > 0:
        Dk = inp["edge_input"].shape[3] if defect == "D_in used as D" else D
        Dr = Dk + 1 if defect == "hop d = D read" else Dk
        hop = inp["hop_table"].to(F64)                                             # [D_in, n_edge, H]
        e, emag = torch.zeros_like(pair), torch.zeros_like(pair)
        for d in range(Dr):
            for f in range(F):
                row = hop[d][inp["edge_input"][:, :, :, d, f].long()]
                e, emag = e + row, emag + row.abs()
        div = divisor(inp["rel_pos"], Dk, defect).to(F64)[..., None] * (1.0 if defect == "mean over F is a sum" else float(F))
        pair, pmag = pair + e / div, pmag + emag / div
    out[:, :, 1:, 1:] += pair.permute(0, 3, 1, 2)
    mag[:, :, 1:, 1:] += pmag.permute(0, 3, 1, 2)
    return out, mag


def pack(dense, ld, defect=None):
    """[G,H,T,T] -> (bias, bias_t) [G,H,T,ld], padding columns -inf."""
    G, H, T = dense.shape[:3]
    fill = 0.0 if defect == "padding columns finite" else NEG_INF
    b = torch.full((G, H, T, ld), fill, dtype=dense.dtype, device=dense.device)
    bt = b.clone()
    b[..., :T] = dense
    bt[..., :T] = dense if defect == "transposed copy not transposed" else dense.transpose(2, 3)
    return b, bt


def to_dtype(x, name):
    """float64 values -> what a device output of type `name` holds (round to nearest even), back in float64."""
    x = x.to(torch.float32)
    return (x.to(torch.bfloat16) if name == "bf16" else x).to(F64)


def _round_split(x):
    """The matrix-core operand of a hop addend: its f32 value as a bf16 high part plus a bf16 low part."""
    x32 = x.to(torch.float32)
    hi = x32.to(torch.bfloat16).to(torch.float32)
    lo = (x32 - hi).to(torch.bfloat16).to(torch.float32)
    return (hi.to(F64) + lo.to(F64))


def slice_sum(slices, T, defect=None):
    """[L,G,H,T,ld] (any float type) -> [G,H,T,T] float64: the layers' slices summed."""
    x = slices.to(F64)[..., :T]
    if defect == "only the first and last slices summed":
        return x[0] + x[-1] if x.shape[0] > 1 else x[0]
    if defect == "the 13th slice dropped":
        keep = [l for l in range(x.shape[0]) if l != 12]
        return x[keep].sum(0)
    return x.sum(0)


def scatter_add(rows, keys, src):
    """zeros([rows, ...]).index_add_(0, keys, src) in float64.  Most pairs of a batch share a handful of keys (padding, 'no hop',
    'unreachable'), and a million atomic adds on one address serialise; long key lists are therefore spread over 256 copies of the
    table (copy = position mod 256) that are summed afterwards -- float64, so the order of the additions is immaterial here."""
    P = keys.shape[0]
    C = 256 if P >= (1 << 16) else 1
    if C > 1:
        keys = keys + rows * (torch.arange(P, device=keys.device) % C)
    out = torch.zeros((C * rows,) + tuple(src.shape[1:]), dtype=F64, device=src.device).index_add_(0, keys, src)
    return out.view((C, rows) + tuple(src.shape[1:])).sum(0)


def backward(inp, slices, D, init, defect=None, weight=None, emulate=False, stats=False):
    """-> dict d_rel, d_poi (None without poi_pos), d_hop [D,n_edge,H] (None when D = 0), d_vdist: init + the scatter, float64.
    weight [G,N,N]: a factor per pair (the lost / doubled pair).  emulate: the documented rounding points applied to the addends.
    stats: additionally (sum |addend|, number of addends) per entry under the keys 'abs' and 'cnt'."""
    ab = inp["attn_bias"]
    G, T = ab.shape[:2]
    N, H, F = T - 1, inp["vdist"].shape[0], inp["edge_input"].shape[4]
    dev = ab.device
    dB = slice_sum(slices, T, defect)
    live = torch.ones_like(ab, dtype=torch.bool) if defect == "a -inf pair not skipped" else ab != NEG_INF
    dB = torch.where(live[:, None], dB, torch.zeros_like(dB))
    r0 = 0 if defect == "row 0 of dBias counted" else 1
    gp = dB[:, :, 1:, 1:].permute(0, 2, 3, 1).reshape(-1, H)
    lv = live[:, 1:, 1:].reshape(-1).to(F64)
    if weight is not None:
        gp = gp * weight.reshape(-1, 1).to(F64)
    if emulate:
        fin = slices.to(F64)[..., :T]
        m = float(torch.where(torch.isfinite(fin), fin.abs(), torch.zeros_like(fin)).max()) * slices.shape[0]
        gran = 2.0 ** (int(np.floor(np.log2(m))) - 34) if m > 0 else 0.0
    res, ab_, cnt = {}, {}, {}

    scatter = scatter_add

    res["d_vdist"] = dB[:, :, r0:, 0].sum((0, 2))
    if stats:
        ab_["d_vdist"], cnt["d_vdist"] = dB[:, :, 1:, 0].abs().sum((0, 2)), live[:, 1:, 0].sum().to(F64).expand(H)
    for name, key, cap in (("d_rel", "rel_pos", LDS_REL), ("d_poi", "poi_pos", LDS_POI)):
        if inp[key] is None:
            res[name] = None
            continue
        keys = inp[key].reshape(-1).long()
        rows = inp[name[2:] + "_table"].shape[0]
        src = gp
        if emulate and gran > 0:
            src = torch.where(torch.isfinite(gp), torch.round(gp / gran) * gran, gp)
        t = scatter(rows, keys, src)
        if defect != "key 0 not skipped":
            t[0] = 0
        if defect == "a key >= the LDS cap dropped":
            t[cap:] = 0
        res[name] = t
        if stats:
            a, c = scatter(rows, keys, gp.abs()), scatter(rows, keys, lv)
            a[0], c[0] = 0, 0
            ab_[name], cnt[name] = a, c[:, None].expand(-1, H)
    res["d_hop"] = None
    if D > 0:
        Dk = inp["edge_input"].shape[3] if defect == "D_in used as D" else D
        div = divisor(inp["rel_pos"], Dk, defect).reshape(-1, 1).to(F64) * (1.0 if defect == "mean over F is a sum" else float(F))
        ge = gp / div
        if emulate:
            ge = torch.where(torch.isfinite(ge), _round_split(ge), ge)
        n_edge = inp["hop_table"].shape[1]
        t = torch.zeros(D, n_edge, H, dtype=F64, device=dev)
        a, c = torch.zeros_like(t), torch.zeros(D, n_edge, dtype=F64, device=dev)
        for d in range(D):
            for f in range(F):
                keys = inp["edge_input"][:, :, :, d, f].reshape(-1).long()
                t[d] += scatter(n_edge, keys, ge)
                if stats:
                    a[d] += scatter(n_edge, keys, ge.abs())
                    c[d] += scatter(n_edge, keys, lv)
        c = c[:, :, None].expand(-1, -1, H)
        if defect == "zero tail (hop row 0) dropped":
            t[:, 0] = 0
        if defect == "an id >= 16 dropped":
            t[:, HOP_LDS_ROWS:] = 0
        res["d_hop"] = t
        ab_["d_hop"], cnt["d_hop"] = a, c
    for k in res:
        if res[k] is not None and defect != "an accumulator overwritten":
            res[k] = res[k] + init[k].to(F64)
    if stats:
        res["abs"], res["cnt"] = ab_, cnt
    return res


# ------------------------------------------------------------------------------------------------ the operation, numpy
def forward_np(inp, D):
    """The same forward as plain numpy loops over (d, f) -- the statement `forward` is checked against on the host."""
    g = {k: (v.cpu().numpy() if v is not None else None) for k, v in inp.items() if torch.is_tensor(v) or v is None}
    ab = g["attn_bias"].astype(np.float64)
    G, T = ab.shape[:2]
    H, F = g["vdist"].shape[0], g["edge_input"].shape[4]
    out = np.repeat(2 * ab[:, None], H, axis=1)
    out[:, :, 1:, 0] += g["vdist"].astype(np.float64)[None, :, None]
    rp = g["rel_pos"].astype(np.int64)
    pair = g["rel_table"].astype(np.float64)[rp]
    if g["poi_pos"] is not None:
        pair = pair + g["poi_table"].astype(np.float64)[g["poi_pos"].astype(np.int64)]
    if D > 0:
        spd = np.where(rp == 0, 1, rp)
        spd = np.clip(np.where(spd > 1, spd - 1, spd), 0, D)
        e = np.zeros_like(pair)
        for d in range(D):
            m = np.zeros_like(pair)
            for f in range(F):
                m += g["hop_table"].astype(np.float64)[d][g["edge_input"][:, :, :, d, f].astype(np.int64)]
            e += m / F
        pair = pair + e / spd[..., None]
    out[:, :, 1:, 1:] += pair.transpose(0, 3, 1, 2)
    return out


def backward_np(inp, slices, D, init):
    g = {k: (v.cpu().numpy() if v is not None else None) for k, v in inp.items() if torch.is_tensor(v) or v is None}
    ab = g["attn_bias"]
    G, T = ab.shape[:2]
    H, F = g["vdist"].shape[0], g["edge_input"].shape[4]
    dB = slices.to(F64).cpu().numpy()[..., :T].sum(0)
    dB = np.where((ab != -np.inf)[:, None], dB, 0.0)
    res = dict(d_vdist=init["d_vdist"].double().cpu().numpy() + dB[:, :, 1:, 0].sum((0, 2)), d_poi=None, d_hop=None)
    gp = dB[:, :, 1:, 1:].transpose(0, 2, 3, 1).reshape(-1, H)
    rp = g["rel_pos"].astype(np.int64).reshape(-1)
    for name, key in (("d_rel", "rel_pos"), ("d_poi", "poi_pos")):
        if g[key] is None:
            continue
        t = np.zeros(init[name].shape, np.float64)
        keys = g[key].astype(np.int64).reshape(-1)
        np.add.at(t, keys[keys != 0], gp[keys != 0])
        res[name] = t + init[name].double().cpu().numpy()
    if D > 0:
        spd = np.where(rp == 0, 1, rp)
        spd = np.clip(np.where(spd > 1, spd - 1, spd), 0, D)
        ge = gp / (F * spd[:, None])
        t = np.zeros(init["d_hop"].shape, np.float64)
        for d in range(D):
            for f in range(F):
                np.add.at(t[d], g["edge_input"][:, :, :, d, f].astype(np.int64).reshape(-1), ge)
        res["d_hop"] = t + init["d_hop"].double().cpu().numpy()
    return res


# ------------------------------------------------------------------------------------------------ case builders
def _gen(dev, *key):
    return torch.Generator(device=dev).manual_seed(zlib.crc32(repr(key).encode()) % (2 ** 31))


def _choice(vals, probs, shape, gen, dev):
    cum = torch.tensor(np.cumsum(probs)[:-1], dtype=torch.float32, device=dev)
    pick = torch.bucketize(torch.rand(shape, generator=gen, device=dev), cum)
    return torch.tensor(vals, dtype=torch.int64, device=dev)[pick]


def exact_rel_values(s):
    """rel_pos values of the EXACT family: those whose divisor is a power of two (and at most max_div)."""
    cand = [0, 1, 2, 3, 5, 9, 17, 510, 513, s["n_rel"] - 1]
    ok = []
    for v in sorted(set(cand)):
        if not 0 <= v < s["n_rel"]:
            continue
        d = int(divisor(torch.tensor([v]), s["D"])[0])
        if s["D"] == 0 or (d >= 1 and d & (d - 1) == 0 and d <= s["max_div"]):
            ok.append(v)
    assert len(ok) >= 3, (s, ok)
    return ok


_INPUT_KEYS = ("G", "N", "H", "D_in", "D", "F", "n_rel", "n_poi", "n_edge", "idx", "edge", "ragged", "hop", "big_ids", "max_div")


def input_key(s, family):
    return tuple(s[k] for k in _INPUT_KEYS) + (family,)


def build_inputs(s, family, dev="cpu"):
    """The index tensors and tables of one shape in one family, on `dev` (seeded per shape; the streams differ between devices)."""
    G, N, H, T, D_in, F = s["G"], s["N"], s["H"], s["T"], s["D_in"], s["F"]
    gen = _gen(dev, *[str(x) for x in input_key(s, family)])
    exact = family == "exact"
    assert not exact or F in (1, 2, 4)
    n_nodes = [max(1, N - (5 * g + 3) % (N // 2 + 1)) if s["ragged"] else N for g in range(G)]
    nn = torch.tensor(n_nodes, device=dev)
    real = torch.arange(N, device=dev)[None, :] < nn[:, None]                     # [G,N]
    real2 = real[:, :, None] & real[:, None, :]
    ab = torch.zeros(G, T, T, device=dev)
    ab[(torch.arange(T, device=dev)[None, :] > nn[:, None])[:, None, :].expand(G, T, T)] = NEG_INF
    holes = torch.rand((G, N, N), generator=gen, device=dev) < 0.01               # (-inf where spd >= rel_pos_max, collator.py)
    ab[:, 1:, 1:][holes] = NEG_INF
    some = torch.rand((G, T, T), generator=gen, device=dev) < 0.05                # a few finite non-zero entries: counted twice
    fine = (torch.randint(-64, 65, (G, T, T), generator=gen, device=dev).float() / 64 if exact
            else torch.randn((G, T, T), generator=gen, device=dev))
    ab = torch.where(some & (ab == 0), fine, ab)
    if exact:
        vals = exact_rel_values(s)
        probs = [0.6 / (len(vals) - 1)] * (len(vals) - 1) + [0.4]
        rel = _choice(vals, probs, (G, N, N), gen, dev)                            # (the last value is the heavy key)
    else:
        heavy = 510 if s["n_rel"] > 510 else s["n_rel"] - 1
        rel = torch.randint(1, s["n_rel"], (G, N, N), generator=gen, device=dev)
        u = torch.rand((G, N, N), generator=gen, device=dev)
        rel[u < 0.35] = heavy
        rel[u > 0.92] = 0
    rel = rel * real2
    poi = None
    if s["n_poi"]:
        poi = torch.randint(1, s["n_poi"], (G, N, N), generator=gen, device=dev)
        u = torch.rand((G, N, N), generator=gen, device=dev)
        poi[u < 0.3] = min(3, s["n_poi"] - 1)
        poi[u > 0.95] = 0
        poi = poi * real2
    if s["hop"] == "random":
        edge = torch.randint(0, s["n_edge"], (G, N, N, D_in, F), generator=gen, device=dev)
        edge[torch.rand(edge.shape, generator=gen, device=dev) < 0.3] = 0
    else:
        hops = torch.randint(0, D_in + 1, (G, N, N), generator=gen, device=dev)
        edge = torch.randint(1, min(6, s["n_edge"]), (G, N, N, D_in, F), generator=gen, device=dev)
        if s["big_ids"]:
            big = torch.randint(HOP_LDS_ROWS, s["n_edge"], edge.shape, generator=gen, device=dev)
            edge = torch.where(torch.rand(edge.shape, generator=gen, device=dev) < 0.03, big, edge)
        edge = edge * (torch.arange(D_in, device=dev)[None, None, None, :] < hops[..., None])[..., None]
    edge = edge * real2[..., None, None]
    if s["hop"] == "midzero":
        assert D_in >= 3 and n_nodes[0] >= 2
        edge[0, 0, 1, 0], edge[0, 0, 1, 1], edge[0, 0, 1, 2] = 0, 5, 2             # a zero before a non-zero id
        ab[0, 1, 2] = 0.0
    if exact:
        tab = lambda *shape: torch.randint(-64, 65, shape, generator=gen, device=dev).float() / 64            # noqa: E731
    else:
        tab = lambda *shape: torch.randn(shape, generator=gen, device=dev) * 0.5                              # noqa: E731
    inp = dict(attn_bias=ab, rel_pos=rel.to(IDX[s["idx"]]), poi_pos=poi.to(IDX[s["idx"]]) if poi is not None else None,
               edge_input=edge.to(IDX[s["edge"]]).contiguous(), rel_table=tab(s["n_rel"], H),
               poi_table=tab(s["n_poi"], H) if poi is not None else None, hop_table=tab(D_in, s["n_edge"], H), vdist=tab(H),
               n_nodes=n_nodes)
    assert int(inp["edge_input"].max()) < s["n_edge"] and int(inp["rel_pos"].max()) < s["n_rel"]
    if exact:
        # forward sums: at most 3 + D F addends of magnitude <= 1, granule 2^-6 / (F max divisor)
        dmax = int(divisor(inp["rel_pos"], s["D"]).max()) if s["D"] > 0 else 1
        assert dmax & (dmax - 1) == 0
        assert (3 + s["D"] * F) * 64 * F * dmax < 2 ** 24
        inp["dmax"] = dmax
    return inp


def init_tables(s, dev="cpu"):
    """The accumulators' starting values: odd multiples of 1/8 (non-zero, exact in both families)."""
    gen = _gen(dev, "init", s["n_rel"], s["n_poi"], s["n_edge"], s["D"], s["H"])
    odd = lambda *shape: (2 * torch.randint(-4, 4, shape, generator=gen, device=dev) + 1).float() / 8     # noqa: E731
    return dict(d_rel=odd(s["n_rel"], s["H"]), d_poi=odd(s["n_poi"], s["H"]) if s["n_poi"] else None,
                d_hop=odd(s["D"], s["n_edge"], s["H"]) if s["D"] > 0 else None, d_vdist=odd(s["H"]))


def exact_condition(s, inp, K, extra=0.0):
    """sum |addend| / granule per table entry, from an upper bound that holds for ANY gradient with |dBias| <= L K / 8 per pair
    (+ `extra`: one larger element) and the accumulators' |initial| <= 7/8: the largest such ratio per table.  < 2^24: every
    partial sum in any order is an integer number of granules that float32 holds exactly."""
    G, N, H, F, L, D = s["G"], s["N"], s["H"], s["F"], s["L"], s["D"]
    dev = inp["attn_bias"].device
    ones = torch.ones(G * N * N, dtype=F64, device=dev)
    worst = {"d_vdist": (G * N * L * K + 8 * extra + 7)}                          # granule 1/8
    for name, key in (("d_rel", "rel_pos"), ("d_poi", "poi_pos")):
        if inp[key] is not None:
            c = scatter_add(s["n_" + name[2:]], inp[key].reshape(-1).long(), ones)
            c[0] = 0
            worst[name] = float(c.max()) * L * K + 8 * extra + 7
    if D > 0:
        div = divisor(inp["rel_pos"], D).reshape(-1).to(F64) * F
        gran = 1.0 / (8 * float(div.max()))
        w = torch.zeros(D, s["n_edge"], dtype=F64, device=dev)
        for d in range(D):
            for f in range(F):
                w[d] += scatter_add(s["n_edge"], inp["edge_input"][:, :, :, d, f].reshape(-1).long(), 1.0 / div)
        worst["d_hop"] = (float(w.max()) * L * K / 8 + extra + 7.0 / 8) / gran
    return worst


def pick_K(s, inp, extra_per_K=0.0):
    for K in (7, 3, 1):
        worst = exact_condition(s, inp, K, extra_per_K * K)
        if all(v < 2 ** 24 for v in worst.values()):
            return K, worst
    raise AssertionError(("no K satisfies the exact condition: a builder bug", s["id"] if "id" in s else s, worst))


def sample_positions(total):
    """The flat positions of [G,H,T,ld] the long backward form looks at to scale its fixed point (csrc/bias.hip: 4 x 8 elements
    per thread of 512; the arithmetic of test_build_bias_bwd_fixed_point_fallbacks)."""
    at = (np.arange(2048, dtype=np.int64) * total // 2048) & ~7
    at = np.where(at + 8 > total, (total - 8) & ~7, at)
    return np.unique((at[:, None] + np.arange(8)[None, :]).reshape(-1))


def build_grad(s, inp, family, dev="cpu", poison=True):
    """dBias as L slices [L,G,H,T,ld] float32 (bf16-exact values when s['db'] == 'bf16') -> (slices, K, special position or None).
    poison: padding columns [T,ld) and row 0 hold NaN (nobody has to have written them; they must have no effect)."""
    G, H, T, ld, L = s["G"], s["H"], s["T"], s["ld"], s["L"]
    assert s["db"] == "bf16" or L == 1
    gen = _gen(dev, "grad", family, G, H, T, ld, L, s["db"], s["special"])
    K, spot = None, None
    if family == "exact":
        K, _ = pick_K(s, inp, extra_per_K=2.0 ** 13 * L / 8 if s["special"] == "outlier" else 0.0)
        x = torch.randint(-K, K + 1, (L, G, H, T, ld), generator=gen, device=dev).float() / 8
    else:
        x = torch.randn((L, G, H, T, ld), generator=gen, device=dev) * 0.1
        if s["db"] == "bf16":
            x = x.to(torch.bfloat16).float()
    if s["special"]:
        assert family == "exact"
        total = G * H * T * ld
        pos = sample_positions(total)
        if s["special"] == "lonely":
            x.reshape(L, -1)[:, torch.from_numpy(pos).to(dev)] = 0.0
        else:
            taken = set(pos.tolist())
            g, h, ab = 1 % G, 2 % H, inp["attn_bias"]
            N, at = T - 1, min(30, T - 1) * (T - 1)                    # walk the pairs of graph g from row 30 on, wrapping
            for step in range(N * N):
                i, j = 1 + (at + step) % (N * N) // N, 1 + (at + step) % N
                if (((g * H + h) * T + i) * ld + j not in taken and float(ab[g, i, j]) != NEG_INF
                        and int(inp["rel_pos"][g, i - 1, j - 1]) != 0):
                    break
            else:
                raise AssertionError("no unsampled live pair: a builder bug")
            spot = (g, h, i, j)
            x[0, g, h, i, j] = 2.0 ** 13 * L * K / 8 if s["special"] == "outlier" else float("nan")
    if poison:
        x[..., T:] = float("nan")
        x[:, :, :, 0, :] = float("nan")
    return x, K, spot


# ------------------------------------------------------------------------------------------------ bounds and verdicts
def forward_bound(s, ref, mag):
    """(D F + 8) u (sum of the addends' magnitudes) + 2^-9 |ref| for a bf16 output; never looser than the gates of
    tests/test_gpu_kernels.py (f32: rtol 1e-5, atol 1e-4; bf16: rtol 8e-3, atol 2e-3)."""
    fin = torch.isfinite(ref)
    r = torch.where(fin, ref.abs(), torch.zeros_like(ref))
    b = (s["D"] * s["F"] + 8) * U * torch.where(fin, mag, torch.zeros_like(mag))
    if s["out"] == "bf16":
        # round to nearest even on the bf16 grid (8 significant bits): half the grid's spacing at the value, 2^(e - 8) for
        # |v| in [2^e, 2^(e+1)) -- between 2^-9 |v| and 2^-8 |v|.  (2^-9 |ref| alone is below what a CORRECTLY rounded result needs
        # in the lower half of every binade: the float64 emulation itself reaches 1.97 times it.)
        top = r + b
        half = torch.where(top > 0, torch.exp2(torch.floor(torch.log2(torch.clamp(top, min=1e-300))) - 8), torch.zeros_like(top))
        return torch.minimum(b + half, 8e-3 * r + 2e-3)
    return torch.minimum(b, 1e-5 * r + 1e-4)


def backward_bound(s, name, ref, abs_sum, cnt, init, max_db):
    """Per entry with K addends over L slices: (K + L + 8) u sum|a| (the accumulator's start counts as one addend); hop entries
    + 2^-16 sum|a| (the bf16 hi/lo split, 'exact to ~2^-17'); rel / poi entries + K 2^-35 L max|dBias| (an addend rounded to 2^-34
    of the sample maximum); never looser than rtol 3e-3, atol 2e-3 max(scale, 1)."""
    L = s["L"]
    tot = abs_sum + init.to(F64).abs()
    b = (cnt + 1 + L + 8) * U * tot
    if name == "d_hop":
        b = b + 2.0 ** -16 * abs_sum
    if name in ("d_rel", "d_poi"):
        b = b + cnt * 2.0 ** -35 * L * max_db
    scale = max(float(ref.abs().max()), 1.0)
    return torch.minimum(b, 3e-3 * ref.abs() + 2e-3 * scale)


def same_bits(got, ref):
    """Equal as float64 values, NaN in the same places (the reference's values are exactly representable in the output type)."""
    got, ref = got.to(F64), ref.to(F64)
    if got.shape != ref.shape:
        return False
    gn, rn = torch.isnan(got), torch.isnan(ref)
    return bool(torch.equal(gn, rn)) and bool(torch.equal(torch.where(gn, torch.zeros_like(got), got), torch.where(rn, torch.zeros_like(ref), ref)))


def within(got, ref, bound):
    """(ok, worst err / bound) over the finite entries of ref; non-finite entries must match exactly."""
    got, ref = got.to(F64), ref.to(F64)
    if got.shape != ref.shape:
        return False, float("inf")
    fin = torch.isfinite(ref)
    if not bool(torch.equal(torch.where(fin, torch.zeros_like(got), got), torch.where(fin, torch.zeros_like(ref), ref))):
        return False, float("inf")                      # (a nan in got where ref is -inf compares unequal as well)
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    if bool(torch.isnan(err).any()):
        return False, float("inf")
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    return worst <= 1.0, worst


def forward_verdict(s, family, got_b, got_bt, ref, mag):
    """got_b, got_bt: [G,H,T,ld] as the device (or the emulation) left them (got_bt None: no transposed copy asked for).
    -> (ok, worst err / bound, reason)."""
    T, ld = s["T"], s["ld"]
    ref_b, ref_bt = pack(ref, ld)
    for got, want, label in ((got_b, ref_b, "bias"), (got_bt, ref_bt, "bias_t")):
        if got is None:
            continue
        got = got.to(F64)
        if ld > T and not bool((got[..., T:] == NEG_INF).all()):
            return False, float("inf"), label + ": padding columns are not -inf"
    if got_bt is not None and not same_bits(got_bt[..., :T], got_b[..., :T].transpose(2, 3)):
        return False, float("inf"), "bias_t is not the transpose of bias"
    if family == "exact":
        ok = same_bits(got_b, to_dtype(ref_b, s["out"]))
        return ok, 0.0 if ok else float("inf"), "" if ok else "bias: not the reference's bits"
    ok, worst = within(got_b[..., :T], ref, forward_bound(s, ref, mag))
    return ok, worst, "" if ok else "bias: beyond the bound"


def backward_verdict(s, family, got, ref, init=None, max_db=0.0):
    """got: dict of the four tables as left by the device (or the emulation); ref: `backward(..., stats=family == 'round')`.
    -> (ok, worst err / bound, reason)."""
    worst = 0.0
    for name in ("d_rel", "d_poi", "d_hop", "d_vdist"):
        if ref[name] is None:
            continue
        if family == "exact":
            if not same_bits(got[name], ref[name].to(torch.float32)):
                return False, float("inf"), name + ": not the reference's bits"
            continue
        b = backward_bound(s, name, ref[name], ref["abs"][name], ref["cnt"][name], init[name], max_db)
        ok, w = within(got[name], ref[name], b)
        worst = max(worst, w)
        if not ok:
            return False, worst, name + ": beyond the bound"
    return True, worst, ""


def pack_reference(src, ld, out):
    """mobgt_bias_pack: src [G,H,T,T] (values of its own type) -> (bias, bias_t) [G,H,T,ld] in type `out`, padding -inf."""
    b, bt = pack(src.to(F64), ld)
    return to_dtype(b, out), to_dtype(bt, out)


# ------------------------------------------------------------------------------------------------ emulation with planted defects
# name -> (direction, the family whose verdict is meant to reject it, what the planted defect is)
MUTANTS = {
    "one pair's contribution lost": ("bwd", "exact", "one live pair adds nothing to any table"),
    "one pair counted twice": ("bwd", "exact", "one live pair adds its gradient twice"),
    "key 0 not skipped": ("bwd", "both", "row 0 of d_rel / d_poi receives the padding pairs"),
    "a -inf pair not skipped": ("bwd", "both", "pairs masked by attn_bias = -inf scatter their gradient"),
    "row 0 of dBias counted": ("bwd", "both", "d_vdist includes dB[g,h,0,0]"),
    "vdist added on row 0": ("fwd", "both", "bias[g,h,0,0] += vdist[h]"),
    "divisor k instead of k-1": ("both", "both", "spd = rel_pos where it should be rel_pos - 1"),
    "clamp to D missing": ("both", "both", "spd not clamped to D"),
    "hop d = D read": ("fwd", "both", "one hop slot too many is summed"),
    "D_in used as D": ("fwd", "both", "all D_in slots summed and the clamp taken at D_in"),
    "mean over F is a sum": ("both", "both", "the 1/F of the mean is missing"),
    "attn_bias counted once": ("fwd", "both", "attn_bias added once (needs a finite non-zero attn_bias entry)"),
    "transposed copy not transposed": ("fwd", "both", "bias_t = bias"),
    "padding columns finite": ("fwd", "both", "columns [T, ld) hold 0"),
    "zero tail (hop row 0) dropped": ("bwd", "exact", "d_hop[:, 0] receives nothing"),
    "an id >= 16 dropped": ("bwd", "both", "d_hop[:, 16:] receives nothing"),
    "a key >= the LDS cap dropped": ("bwd", "exact", "d_rel[512:] / d_poi[1024:] receive nothing"),
    "only the first and last slices summed": ("bwd", "both", "slices 1 .. L-2 ignored (L >= 3)"),
    "the 13th slice dropped": ("bwd", "both", "slice 12 ignored (L = 13)"),
    "an accumulator overwritten": ("bwd", "both", "tables = sum instead of initial + sum"),
}


def _victim(inp, slices, T):
    """A live pair with non-zero keys and a non-zero gradient: the pair the lost / doubled mutants act on."""
    ab, rel = inp["attn_bias"], inp["rel_pos"]
    dB = slice_sum(slices, T)
    ok = (ab[:, 1:, 1:] != NEG_INF) & (rel != 0) & (dB[:, :, 1:, 1:].abs().amin(1) > 0)
    if inp["poi_pos"] is not None:
        ok &= inp["poi_pos"] != 0
    at = torch.nonzero(ok)
    assert len(at), "no pair to plant the defect on"
    return tuple(int(v) for v in at[len(at) // 2])


def emulate_forward(s, inp, defect=None):
    """What a device that rounds where the kernel says it rounds would leave: (bias, bias_t) in the output type's values."""
    ref, _ = forward(inp, s["D"], defect)
    b, bt = pack(ref, s["ld"], defect)
    return to_dtype(b, s["out"]), to_dtype(bt, s["out"])


def emulate_backward(s, inp, slices, init, defect=None):
    weight = None
    if defect in ("one pair's contribution lost", "one pair counted twice"):
        g, i, j = _victim(inp, slices, s["T"])
        weight = torch.ones(inp["rel_pos"].shape, dtype=F64, device=slices.device)
        weight[g, i, j] = 0.0 if "lost" in defect else 2.0
    res = backward(inp, slices, s["D"], init, defect, weight=weight, emulate=True)
    return {k: (v.to(torch.float32) if v is not None else None) for k, v in res.items()}


def mutant(name, s, inp, slices=None, init=None):
    """The emulation with the planted defect `name` -> forward: (bias, bias_t); backward: dict of tables."""
    direction = MUTANTS[name][0]
    if slices is None:
        assert direction in ("fwd", "both")
        return emulate_forward(s, inp, name)
    assert direction in ("bwd", "both")
    return emulate_backward(s, inp, slices, init, name)
