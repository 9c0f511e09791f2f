"""What the encoder chain kernels (csrc/chain.hip) are judged against, independent of the library.

The chain of include/mobgt_hip.h (the comment above mobgt_layer_chain_fwd / _bwd / _bwd_preln), everything row-local of a layer:

    y = a Wo^T + bo;  x1 = x + dropout1(y);  z = norm1(x1);  u = z W1^T + b1;  h = gelu(u);  f = h W2^T + b2;
    x2 = x1 + dropout2(f);  out = normx(x2);  qkv_next = out Wq^T + bq
    post-LN: `out` leaves the layer, the layer above hands back dout (its dx1) and dqkv:  d(out) = dout + dqkv Wq
    pre-LN:  x2 leaves the layer (normx is the successor's attention norm):                d(x2)  = dout + normx'(dqkv Wq)

  * `reference`   that, in float64 on the CPU through torch autograd, on the inputs as given (bf16 values widened);
  * `emulation`   the same mathematics in float64 with a HAND-WRITTEN backward that rounds to bf16 / f32 where chain.hip's design
                  does (its header: y, u, h, f, qkv "rounded to bf16 exactly where a bf16 tensor used to be written"; z, out_a the
                  bf16 MFMA operands; x1, x2, out, the statistics f32; backward: df, du, dy, da bf16, dz = bf16(du W1) -- in the
                  cluster / 64-row forms bf16 of the f32 sum of 4 / 2 / 3 f32 partial sums --, dx1 f32, the column sums taken from
                  the UNROUNDED f32 df / dy, db1 from the ROUNDED du).  The backward takes the SAVED tensors (x1, x2, u, statistics)
                  as arguments, so a backward can be judged on the emulation's forward.  It is the yardstick for tolerances:
                  tolerance = 2 x (emulation against reference) per case and tensor.  With `rounding=False` it is the reference
                  again (tests/test_host_chain_reference.py holds it to autograd);
  * `make_case`   seeded inputs of the families the GPU matrix runs;
  * `compare`     the one metric: per ROW relative error, next to the relative L2 and the largest element error of a tensor;
  * `mutant`      deliberately wrong float64 computations (a lost inv_keep, a swapped mask, a short column sum ...) `compare` must
                  reject at those tolerances -- tests/test_host_chain_reference.py shows it without a GPU.

Nothing in here imports mobgt_amd.  Dropout keep masks come from the caller (`keep_fn(seed, salt, R, C, p)`): the host tests draw
Bernoulli masks, the GPU tests replay the kernels' rule (ops.dropout_site_mask).
"""
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from attn_reference import FLOOR_SHARE_CAP, ROW_FLOOR, bf16r          # noqa: F401  (one set of conventions for both kernel families)

F64 = torch.float64
LN_EPS = 1e-5
SALT1, SALT2 = 9, 10

# Below this an error is f32 arithmetic, not a rounding point.  The kernels accumulate every product in f32: a chain of K <= 1024
# terms carries at most K 2^-24 = 2^-14 of the sum of the terms' magnitudes; the Abramowitz-Stegun erf is off by <= 1.5e-7 (2^-22),
# the hardware reciprocal, exponential and inverse square root by <= 2^-22 relative.  All of that lies under 2^-13, a bf16 rounding
# point is 2^-9, so 2^-12 separates the two: tolerances never go below it -- a tensor the emulation reproduces EXACTLY (an f32 column
# sum of f32 inputs, x1 where the mask drops) still admits f32 noise, and nothing a lost bf16 rounding could show.
TOL_FLOOR = 2.0 ** -12
# The ceilings the existing chain tests allow (tests/test_gpu_layer.py): 2e-2 of the tensor maximum at the model level, 2^-6 of it
# for the backward's row tensors at the C ABI.  No tolerance outside the common-mode and flat-row families exceeds them.  (The [C]
# sums get the 2e-2: a sum over R = 15..33 rows of bf16-rounded dz carries 5e-3 of its maximum in the emulation alone.)
CAP_ELEM, CAP_BWD_ROWS, CAP_SUMS = 2e-2, 2.0 ** -6, 2e-2
UNCAPPED = ("common", "flat")

FAMILIES = ("plain", "common", "flat", "dom_x", "dom_y", "gelu", "sparse")
FWD_NAMES = ("y", "x1", "z", "u", "h", "f", "x2", "out", "out_a", "qkv", "mean1", "rstd1", "mean2", "rstd2")
BWD_ROWS = ("df", "du", "dz", "dy", "da", "dx1")
SUMS = ("dnxw", "dnxb", "db2", "dn1w", "dn1b", "dbo")
PASSENGER_SHAPES = ("qkv", "o", "w1", "w2")                # dW [3C,C], [C,C], [F,C], [C,F]: the layer's own four weights


def f32r(t):
    return t.to(torch.float32).to(F64)


def sum_floor(R):
    """Floor of an f32 sum over R rows (the six [C] sums, db1, the passengers' dW / db): R additions of <= 2^-24 each."""
    return max(TOL_FLOOR, R * 2.0 ** -24)


def inv_keep_of(p_drop):
    """The kernels' f32 value: 1 / (1 - thr / 65536), thr = the 16-bit threshold of p."""
    if not p_drop:
        return 1.0
    thr = np.float32(int(np.float32(p_drop) * np.float32(65536.0) + np.float32(0.5)))
    return float(np.float32(1.0) / (np.float32(1.0) - thr / np.float32(65536.0)))


def host_keep(seed, salt, R, C, p_drop):
    thr = int(p_drop * 65536 + 0.5)
    rs = np.random.RandomState((seed * 31 + salt) & 0x7FFFFFFF)
    return rs.randint(0, 65536, size=(R, C)) >= thr


# ------------------------------------------------------------------------------------------------ cases
def flat_rows(R):
    """Family "flat": max(1, R // 12) rows (<= 8.4 % of them), spread over R, the LAST row among them."""
    n = max(1, R // 12)
    return sorted({R - 1 - (i * R) // n for i in range(n)})


def sparse_rows(R):
    """Family "sparse": the rows whose dout / dqkv are nonzero -- every 7th and the last; every other one of them in 8 columns only."""
    return sorted(set(range(0, R, 7)) | {R - 1})


def make_case(C, R, family="plain", F=1024, p_drop=0.0, preln=False, successor=True, tail=False, last=False, n_wg=0, with_db=True,
              seed=77, keep_fn=host_keep):
    """Seeded inputs, float64 tensors holding bf16 (a, weights, biases, dqkv, passenger operands) or f32 (x, norm weights, dout) values.
      plain    the scales of the existing chain tests: a, x, dout ~ N(0, 1), W ~ N(0, 1 / fan_in), biases 0.1 N, norm weights 1 + 0.1 N
      common   x = m + N(0, 1), one m per row, |m| uniform in 20..100 with either sign (no row of x1 / x2 under the row floor): mean and
               variance of both norms must survive the cancellation
      flat     `flat_rows` rows of x1 constant (a = 0 there, bo = 0: y = 0, x1 = x = c), every second of them up to ONE f32 ulp in one
               column: variance ~ 0, eps decides rstd = 316.  dout / dqkv of those rows are scaled by 2^-8 so that their dx1 / dy / da rows
               (316 x the others') do not push the other rows under the row floor
      dom_x    x ~ 64 N:  |x| >> |y|, |f|  (the branch outputs are round-off of the residual stream)
      dom_y    x ~ N / 64:  the opposite
      gelu     a third of the F columns of u pushed to |u| ~ 6..10 (b1 = +-8, both signs), a third clustered at 0 (W1 rows x 0.02,
               b1 ~ 0.02 N), a third plain: erf_as and gelu' in their tails and around the origin
      sparse   dout / dqkv nonzero in `sparse_rows` only (half of them in 8 columns only): every other row of df / du / dy / da / dx1 is
               EXACTLY zero (rows are independent), and a column leaking into another shows in the [C] sums
    preln: the pre-LN definition (successor: nxw / wq belong to the next layer; False: x2 is the only output of the second half).
    last: no next projection.  tail: the layer above hands back dqkv.  n_wg passengers with the shapes of PASSENGER_SHAPES."""
    assert family in FAMILIES, family
    has_norm = successor or not preln
    assert not (tail and not has_norm) and not (preln and not successor and not last)
    key = (C, R, family, F, float(p_drop), bool(preln), bool(successor), bool(tail), bool(last), int(n_wg), bool(with_db),
           int(seed) if p_drop else 0, getattr(keep_fn, "__name__", "keep") if p_drop else "")
    rng = np.random.RandomState(zlib.crc32(repr((C, R, family, F)).encode()) & 0x7FFFFFFF)

    rng_w = np.random.RandomState(zlib.crc32(repr(("weights", C, F)).encode()) & 0x7FFFFFFF)      # (the weights depend on the width alone)

    def normal(*shape, k=1.0, g=None):
        return torch.from_numpy((g or rng).standard_normal(shape)) * k

    def wnormal(*shape, k=1.0):
        return normal(*shape, k=k, g=rng_w)
    b, f = bf16r, f32r
    c = SimpleNamespace(C=C, R=R, F=F, family=family, p_drop=float(p_drop), preln=bool(preln), successor=bool(successor), has_norm=has_norm,
                        tail=bool(tail), last=bool(last), n_wg=int(n_wg), with_db=bool(with_db), seed=int(seed), key=key,
                        inv_keep=inv_keep_of(p_drop), keep1=None, keep2=None, flat=[], nonzero=None)
    c.wo, c.w1, c.w2, c.wq = b(wnormal(C, C, k=C ** -0.5)), wnormal(F, C, k=C ** -0.5), b(wnormal(C, F, k=F ** -0.5)), b(wnormal(3 * C, C, k=C ** -0.5))
    c.bo, c.b1, c.b2, c.bq = b(wnormal(C, k=0.1)), wnormal(F, k=0.1), b(wnormal(C, k=0.1)), b(wnormal(3 * C, k=0.1))
    c.n1w, c.n1b, c.nxw, c.nxb = f(1 + wnormal(C, k=0.1)), f(wnormal(C, k=0.1)), f(1 + wnormal(C, k=0.1)), f(wnormal(C, k=0.1))
    c.a, x = b(normal(R, C)), normal(R, C)
    dout, dqkv = normal(R, C), normal(R, 3 * C, k=0.3)
    if family == "common":
        x = x + torch.from_numpy(rng.uniform(20.0, 100.0, size=(R, 1)) * rng.choice([-1.0, 1.0], size=(R, 1)))
    elif family == "dom_x":
        x = x * 64.0
    elif family == "dom_y":
        x = x / 64.0
    elif family == "gelu":
        third = F // 3
        sign = torch.where(torch.arange(third) % 2 == 0, 1.0, -1.0).to(F64)
        c.b1[:third] = 8.0 * sign
        c.w1[third:2 * third] *= 0.02
        c.b1[third:2 * third] *= 0.2
    elif family == "flat":
        c.flat = flat_rows(R)
        c.bo = torch.zeros_like(c.bo)
        for i, r in enumerate(c.flat):
            c.a[r] = 0.0
            v = np.float32(x[r, 0])
            x[r] = float(v)
            if i % 2:
                x[r, (7 * i + 3) % C] = float(np.nextafter(v, np.float32(np.inf)))
            dout[r] *= 2.0 ** -8
            dqkv[r] *= 2.0 ** -8
    elif family == "sparse":
        c.nonzero = sparse_rows(R)
        m = torch.zeros(R, 1, dtype=F64)
        m[c.nonzero] = 1.0
        cols = torch.ones(R, C, dtype=F64)
        for r in c.nonzero[1::2]:
            cols[r] = 0.0
            cols[r, (5 * r) % (C - 8):(5 * r) % (C - 8) + 8] = 1.0
        dout = dout * m * cols
        dqkv = dqkv * m
    c.w1, c.b1 = b(c.w1), b(c.b1)
    c.x, c.dout, c.dqkv = f(x), f(dout), b(dqkv)
    if p_drop:
        c.keep1 = torch.from_numpy(np.ascontiguousarray(keep_fn(seed, SALT1, R, C, p_drop))).to(F64)
        c.keep2 = torch.from_numpy(np.ascontiguousarray(keep_fn(seed, SALT2, R, C, p_drop))).to(F64)
    # the passengers: the weight gradients of the layer above, dW = g^T x over the same R rows (bf16 operands)
    shapes = {"qkv": (3 * C, C), "o": (C, C), "w1": (F, C), "w2": (C, F)}
    c.wg = []
    for name in PASSENGER_SHAPES[:n_wg]:
        M, N = shapes[name]
        c.wg.append(SimpleNamespace(name=name, M=M, N=N, g=b(normal(R, M, k=0.5)), x=b(normal(R, N))))
    return c


# ------------------------------------------------------------------------------------------------ reference
def _ln(x, w, b):
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rs = (var + LN_EPS).rsqrt()
    return (x - mu) * rs * w + b, mu.squeeze(1), rs.squeeze(1)


def _gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u * 0.7071067811865476))


def _gelu_grad(u):
    return 0.5 * (1.0 + torch.erf(u * 0.7071067811865476)) + u * torch.exp(-0.5 * u * u) * 0.3989422804014327


def _drop(v, keep, inv_keep):
    return v if keep is None else v * keep * inv_keep


def reference(c):
    """Forward and autograd backward in float64.  dict of FWD_NAMES (what the definition has: no out / qkv / statistics of a norm
    that is not there), BWD_ROWS, SUMS, db1 and the passengers' pw{i} / pb{i} (dW, db)."""
    leaves = {n: getattr(c, n).clone().requires_grad_(True) for n in ("a", "wo", "bo", "n1w", "n1b", "w1", "b1", "w2", "b2", "nxw", "nxb")}
    L = SimpleNamespace(**leaves)
    t = {}
    t["y"] = L.a @ L.wo.T + L.bo
    t["x1"] = c.x + _drop(t["y"], c.keep1, c.inv_keep)
    t["z"], t["mean1"], t["rstd1"] = _ln(t["x1"], L.n1w, L.n1b)
    t["u"] = t["z"] @ L.w1.T + L.b1
    t["h"] = _gelu(t["u"])
    t["f"] = t["h"] @ L.w2.T + L.b2
    t["x2"] = t["x1"] + _drop(t["f"], c.keep2, c.inv_keep)
    if c.has_norm:
        t["out"], t["mean2"], t["rstd2"] = _ln(t["x2"], L.nxw, L.nxb)
        t["out_a"] = t["out"]                          # (the bf16 copy the next projection multiplies)
        if not c.last:
            t["qkv"] = t["out"] @ c.wq.T + c.bq
    for n in ("y", "x1", "z", "u", "f"):
        t[n].retain_grad()
    loss = ((t["x2"] if c.preln else t["out"]) * c.dout).sum()
    if c.tail:
        loss = loss + ((t["out"] @ c.wq.T) * c.dqkv).sum()
    loss.backward()
    res = {n: v.detach() for n, v in t.items()}
    res.update(df=t["f"].grad, du=t["u"].grad, dz=t["z"].grad, dy=t["y"].grad, da=L.a.grad, dx1=t["x1"].grad,
               db2=L.b2.grad, dn1w=L.n1w.grad, dn1b=L.n1b.grad, dbo=L.bo.grad, db1=L.b1.grad)
    zc = torch.zeros(c.C, dtype=F64)
    res["dnxw"] = L.nxw.grad if L.nxw.grad is not None else zc
    res["dnxb"] = L.nxb.grad if L.nxb.grad is not None else zc.clone()
    for i, p in enumerate(c.wg):
        res["pw%d" % i] = p.g.T @ p.x
        res["pb%d" % i] = p.g.sum(0)
    return res


# ------------------------------------------------------------------------------------------------ emulation
MUTANTS = ("no_inv_keep_site2", "site2_mask_of_site1", "ln_bwd_without_xhat_term", "ln_stats_from_bf16", "w2_kstep_missing",
           "colsum_full_blocks_only", "tail_behind_the_norm", "gelu_grad_of_h", "dw_last_split_skipped")


def _ln_stats(x, rounding, from_bf16=False):
    xs = bf16r(x) if from_bf16 else x
    mu = xs.mean(1, keepdim=True)
    var = ((xs - mu) ** 2).mean(1, keepdim=True)
    rs = (var + LN_EPS).rsqrt()
    return (f32r(mu), f32r(rs)) if rounding else (mu, rs)


def emulation_forward(c, rounding=True, mut=None):
    """chain.hip's forward: r = bf16 where a bf16 tensor is written (y, z, u, h, f, out_a, qkv), f32 for the residual stream and the
    statistics.  h = gelu of the ROUNDED u; the statistics are two-pass, from the f32 rows."""
    r = bf16r if rounding else (lambda v: v)
    s = f32r if rounding else (lambda v: v)
    keep2 = c.keep1 if mut == "site2_mask_of_site1" else c.keep2
    t = {}
    t["y"] = r(c.a @ c.wo.T + c.bo)
    t["x1"] = s(c.x + s(_drop(t["y"], c.keep1, c.inv_keep)))
    mu, rs = _ln_stats(t["x1"], rounding, from_bf16=mut == "ln_stats_from_bf16")
    t["mean1"], t["rstd1"] = mu.squeeze(1), rs.squeeze(1)
    t["z"] = r((t["x1"] - mu) * rs * c.n1w + c.n1b)
    t["u"] = r(t["z"] @ c.w1.T + c.b1)
    t["h"] = r(_gelu(t["u"]))
    h = t["h"]
    if mut == "w2_kstep_missing":
        h = h.clone()
        h[:, c.F - 32:] = 0.0
    t["f"] = r(h @ c.w2.T + c.b2)
    t["x2"] = s(t["x1"] + s(_drop(t["f"], keep2, c.inv_keep)))
    if c.has_norm:
        mu2, rs2 = _ln_stats(t["x2"], rounding)
        t["mean2"], t["rstd2"] = mu2.squeeze(1), rs2.squeeze(1)
        t["out"] = s((t["x2"] - mu2) * rs2 * c.nxw + c.nxb)
        t["out_a"] = r(t["out"])
        if not c.last:
            t["qkv"] = r(t["out_a"] @ c.wq.T + c.bq)
    return t


def _colsum(v, c, mut):
    if mut == "colsum_full_blocks_only":
        return v[: (c.R // 16) * 16].sum(0)
    return v.sum(0)


def _ln_bwd(d, xpre, mu, rs, w, no_xhat_term=False):
    xh = (xpre - mu.unsqueeze(1)) * rs.unsqueeze(1)
    gg = d * w
    s1 = gg.mean(1, keepdim=True)
    s2 = (gg * xh).mean(1, keepdim=True)
    t = rs.unsqueeze(1) * (gg - s1 - (0.0 if no_xhat_term else xh * s2))
    return t, xh


def emulation_backward(c, saved, rounding=True, n_split=1, mut=None):
    """chain.hip's backward from the SAVED x1, x2, u and statistics (`saved`: a dict with those names, values of their storage types).
    n_split: the f32 partial sums dz = du W1 is formed from (1: the one-workgroup form, 4 / 2: the cluster forms' K ranges of
    F / n_split, 3: the 64-row form's chunks of 384, 384 and F - 768 columns)."""
    r = bf16r if rounding else (lambda v: v)
    s = f32r if rounding else (lambda v: v)
    keep2 = c.keep1 if mut == "site2_mask_of_site1" else c.keep2
    inv2 = 1.0 if mut == "no_inv_keep_site2" else c.inv_keep
    res = {}
    zc = torch.zeros(c.C, dtype=F64)
    tailp = s(c.dqkv @ c.wq) if c.tail else None
    if not c.has_norm:
        dx2, res["dnxw"], res["dnxb"] = c.dout, zc, zc.clone()
    else:
        if c.preln:
            d = tailp if c.tail else torch.zeros_like(c.dout)
        elif mut == "tail_behind_the_norm":
            d = c.dout
        else:
            d = s(c.dout + tailp) if c.tail else c.dout
        t, xh2 = _ln_bwd(d, saved["x2"], saved["mean2"], saved["rstd2"], c.nxw)
        if c.preln:
            t = t + c.dout
        elif mut == "tail_behind_the_norm" and c.tail:
            t = t + tailp
        dx2 = s(t)
        res["dnxw"], res["dnxb"] = _colsum(d * xh2, c, mut), _colsum(d, c, mut)
    dfv = s(_drop(dx2, keep2, inv2))
    res["db2"] = _colsum(dfv, c, mut)
    res["df"] = r(dfv)
    u = saved["u"]
    gp = _gelu_grad(r(_gelu(u))) if mut == "gelu_grad_of_h" else _gelu_grad(u)
    res["du"] = r((res["df"] @ c.w2) * gp)
    res["db1"] = _colsum(res["du"], c, mut)
    bounds = {1: [0, c.F], 2: [0, c.F // 2, c.F], 4: [0, c.F // 4, c.F // 2, 3 * c.F // 4, c.F], 3: [0, 384, 768, c.F]}[n_split]
    acc = None
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        part = s(res["du"][:, lo:hi] @ c.w1[lo:hi])
        acc = part if acc is None else s(acc + part)
    res["dz"] = r(acc)
    t, xh1 = _ln_bwd(res["dz"], saved["x1"], saved["mean1"], saved["rstd1"], c.n1w, no_xhat_term=mut == "ln_bwd_without_xhat_term")
    res["dn1w"], res["dn1b"] = _colsum(res["dz"] * xh1, c, mut), _colsum(res["dz"], c, mut)
    res["dx1"] = s(dx2 + t)
    dyv = s(_drop(res["dx1"], c.keep1, c.inv_keep))
    res["dbo"] = _colsum(dyv, c, mut)
    res["dy"] = r(dyv)
    res["da"] = r(res["dy"] @ c.wo)
    for i, p in enumerate(c.wg):
        g = p.g
        if mut == "dw_last_split_skipped":
            g = g.clone()
            g[passenger_last_split(c.R, p.M, p.N):] = 0.0
        res["pw%d" % i] = g.T @ p.x                       # (bf16 operands, f32 sums: nothing of it rounds to bf16)
        res["pb%d" % i] = g.sum(0)
    return res


def passenger_last_split(R, M, N):
    """First row of the last split of R a passenger's workgroups walk (csrc/wgrad_body.h fill_problem: 32 x 32 tiles, 64 workgroups
    aimed at, slabs of 12 waves x 32 rows); R itself when there is only one split."""
    tiles = ((M + 31) // 32) * ((N + 31) // 32)
    slab = 12 * 32
    splits = max(1, min(64 // tiles, (R + slab - 1) // slab))
    k_per = (((R + splits - 1) // splits + slab - 1) // slab) * slab
    n = (R + k_per - 1) // k_per
    return (n - 1) * k_per if n > 1 else R


def saved_of(fwd):
    """What the forward leaves for the backward, in the storage types: x1, x2, statistics f32, u bf16."""
    return {n: fwd[n] for n in ("x1", "x2", "u", "mean1", "rstd1", "mean2", "rstd2") if n in fwd}


def emulation(c, rounding=True, n_split=1, mut=None):
    fwd = emulation_forward(c, rounding, mut)
    res = dict(fwd)
    res.update(emulation_backward(c, saved_of(fwd), rounding, n_split, mut))
    return res


def mutant(c, which):
    """A deliberately wrong float64 computation of the case (no rounding anywhere), or None where the defect does not exist for it:
      no_inv_keep_site2         df = dx2 * keep, the 1 / (1 - p) lost at the second site's backward
      site2_mask_of_site1       site 2 (forward and backward) uses the mask of site 1 (salt1 for salt2)
      ln_bwd_without_xhat_term  the first norm's backward without its mean-of-(dz * xhat) term
      ln_stats_from_bf16        mean / rstd of the first norm taken from the bf16-rounded rows
      w2_kstep_missing          the last 32-wide k-step missing from h W2^T
      colsum_full_blocks_only   every column sum stops at the last full 16-row block of a ragged R
      tail_behind_the_norm      post-LN: the tail product added behind the second norm instead of in front
      gelu_grad_of_h            gelu' evaluated on h instead of u
      dw_last_split_skipped     a passenger dW / db that skips its last split of R"""
    assert which in MUTANTS, which
    if which in ("no_inv_keep_site2", "site2_mask_of_site1") and not c.p_drop:
        return None
    if which == "colsum_full_blocks_only" and c.R % 16 == 0:
        return None
    if which == "tail_behind_the_norm" and (c.preln or not c.tail):
        return None
    if which == "dw_last_split_skipped" and (not c.wg or all(passenger_last_split(c.R, p.M, p.N) >= c.R for p in c.wg)):
        return None
    return emulation(c, rounding=False, mut=which)


# ------------------------------------------------------------------------------------------------ caches
_CACHE = {}


def _cached(kind, c, make):
    k = (kind,) + c.key
    if k not in _CACHE:
        if len(_CACHE) > 48:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[k] = make()
    return _CACHE[k]


def case_reference(c):
    return _cached("ref", c, lambda: reference(c))


def case_emulation(c, n_split=1):
    """Forward + backward-on-its-own-forward; the forward is shared by every n_split."""
    fwd = _cached("emu_fwd", c, lambda: emulation_forward(c))

    def make():
        res = dict(fwd)
        res.update(emulation_backward(c, saved_of(fwd), True, n_split))
        return res
    return _cached(("emu", n_split), c, make)


# ------------------------------------------------------------------------------------------------ the metric
def kind_of(name):
    if name in BWD_ROWS:
        return "bwd_rows"
    if name in SUMS or name == "db1" or name.startswith("pw") or name.startswith("pb"):
        return "sums"
    return "fwd"


def measure(got, want):
    """One tensor: dict(row, l2, elem, floor_share, n_judged, n_zero).
      row    max over judged rows of ||got - want|| / max(||want row||, ROW_FLOOR * the tensor's largest row norm).  A row: a row of a
             2-D tensor; a 1-D tensor ([C] sums, db1, the statistics) is ONE row;
      l2     ||got - want|| / ||want|| over the whole tensor;   elem  max |got - want| / max |want|;
      floor_share  share of the judged rows whose reference norm lies below the floor.
    Rows whose reference is identically zero (the sparse family) are not judged here: the tests assert them exactly zero."""
    g64, w64 = got.detach().to(F64).cpu(), want.detach().to(F64).cpu()
    assert g64.shape == w64.shape, (g64.shape, w64.shape)
    assert bool(torch.isfinite(g64).all()), "non-finite values"
    if g64.dim() == 1:
        g64, w64 = g64.unsqueeze(0), w64.unsqueeze(0)
    nrm = w64.pow(2).sum(1).sqrt()
    judged = nrm > 0
    diff = (g64 - w64) * judged.unsqueeze(1)
    err = diff.pow(2).sum(1).sqrt()
    if bool(judged.any()):
        floor = ROW_FLOOR * float(nrm.max())
        row = float((err[judged] / nrm[judged].clamp_min(floor)).max())
        share = float((nrm[judged] < floor).double().mean())
    else:
        row, share = 0.0, 0.0
    wn, wm = float(w64.norm()), float(w64.abs().max())
    return dict(row=row, l2=float(diff.norm()) / wn if wn > 0 else 0.0, elem=float(diff.abs().max()) / wm if wm > 0 else 0.0,
                floor_share=share, n_judged=int(judged.sum()), n_zero=int((~judged).sum()))


def tolerances(c, names, n_split=1):
    """Per tensor of `names`: 2 x what `measure` gives the emulation against the float64 reference on this very case, never below the
    f32 floor (TOL_FLOOR; sum_floor(R) for what is summed over the R rows) and -- outside the common-mode and flat-row families --
    never above the ceilings of the existing chain tests."""
    ref, emu = case_reference(c), case_emulation(c, n_split)
    tol = {}
    for name in names:
        m = measure(emu[name], ref[name])
        kind = kind_of(name)
        floor = sum_floor(c.R) if kind == "sums" else TOL_FLOOR
        t = {k: max(2.0 * m[k], floor) for k in ("row", "l2", "elem")}
        if c.family not in UNCAPPED:
            cap = {"fwd": CAP_ELEM, "bwd_rows": CAP_BWD_ROWS, "sums": CAP_SUMS}[kind]
            t["l2"], t["elem"] = min(t["l2"], CAP_ELEM), min(t["elem"], cap)
        t["emu"] = m
        tol[name] = t
    return tol


def compare(got, want, tol):
    """Every tensor of `tol` in `got` against `want`: {name: measure(...)} and, in "fail", the (name, metric, value, tolerance) beyond `tol`."""
    rep, fail = {}, []
    for name, t in tol.items():
        m = measure(got[name], want[name])
        rep[name] = m
        for k in ("row", "l2", "elem"):
            if not m[k] <= t[k]:
                fail.append((name, k, m[k], t[k]))
    rep["fail"] = fail
    return rep


def worst_ratio(rep, tol):
    return max(rep[n][k] / tol[n][k] for n in tol for k in ("row", "l2", "elem"))


def format_report(rep, tol, label, emu_rep=None):
    lines = []
    for n in tol:
        m, t = rep[n], tol[n]
        extra = "" if emu_rep is None else "  vs emu row %.2e l2 %.2e" % (emu_rep[n]["row"], emu_rep[n]["l2"])
        lines.append("%s %-6s row %.2e/%.2e  l2 %.2e/%.2e  elem %.2e/%.2e  emu row %.2e l2 %.2e  floor share %.3f%s"
                     % (label, n, m["row"], t["row"], m["l2"], t["l2"], m["elem"], t["elem"], t["emu"]["row"], t["emu"]["l2"],
                        m["floor_share"], extra))
    return "\n".join(lines)


def check(got, want, tol, label="", emu=None):
    rep = compare(got, want, tol)
    emu_rep = None if emu is None else {n: measure(got[n], emu[n]) for n in tol}
    print(format_report(rep, tol, label, emu_rep))
    assert not rep["fail"], "%s: beyond tolerance (tensor, metric, value, tolerance): %s" % (label, rep["fail"])
    return rep


def floor_shares(c):
    ref = case_reference(c)
    return {n: measure(v, v)["floor_share"] for n, v in ref.items()}


def fwd_names(c):
    return [n for n in FWD_NAMES if (c.has_norm or n not in ("out", "out_a", "mean2", "rstd2", "qkv")) and (n != "qkv" or not c.last)]


def bwd_names(c, big=False):
    """What a backward entry point writes (dz stays inside the kernels); db1 on the 64-row entry point."""
    names = [n for n in BWD_ROWS if n != "dz"] + list(SUMS) + (["db1"] if big else [])
    for i in range(len(c.wg)):
        names += ["pw%d" % i] + (["pb%d" % i] if c.with_db else [])
    return names


# ------------------------------------------------------------------------------------------------ the matrix
WIDTHS = (128, 192, 256)
BIG_ROWS = 4096                        # csrc/chain.hip CHAIN_BIG_ROWS: past it the 64-row forms
R16 = (1, 15, 16, 17, 33)
R64 = (63, 64, 65)
DROP_MODES = ((0.0, "host"), (0.1, "host"), (0.1, "split"))
FORMS = ("one", "cl4", "cl2", "big64", "bwd_big")


def expected_form(R, ws, cus):
    """What the entry points dispatch to (chain.hip pick_ncl): "big64" past BIG_ROWS; with a workspace "cl4" while 4 workgroups per
    16-row block fit the compute units (at most 256 of them count), "cl2" while 2 do; else "one"."""
    if R > BIG_ROWS:
        return "big64"
    if not ws:
        return "one"
    nblk, cus = (R + 15) // 16, min(cus, 256)
    return "cl4" if nblk * 4 <= cus else ("cl2" if nblk * 2 <= cus else "one")


def spec_id(s, cus=256):
    want = "bwd_big" if s["form"] == "bwd_big" else expected_form(s["R"], s["form"] in ("cl4", "cl2", "ws_one"), cus)
    kind = ("preln" + ("" if s["successor"] else "_alone")) if s["preln"] else "post"
    return "%s-%s-C%d-R%d-%s-%s%s%s-p%s%s-wg%d%s" % (s["dir"], want, s["C"], s["R"], s["family"], kind, "-last" if s["last"] else "",
                                                     "-tail" if s["tail"] else "", ("%g" % s["p"]).replace(".", ""),
                                                     ("-" + s["seed_mode"]) if s["p"] else "", s["n_wg"],
                                                     "" if s["with_db"] or not s["n_wg"] else "-nodb")


def matrix_specs(cus=256):
    """Every case of the chain matrix as a dict(dir, form, C, R, family, p, seed_mode, preln, successor, last, tail, n_wg, with_db).
    dir: "fwd" (against the reference), "bwd" (the backward ON THE EMULATION'S saved tensors), "both" (forward, then backward on the
    device's own saved tensors).  form: which launch form the case is built to reach -- "one" (no workspace), "ws_one" (a workspace past
    the cluster thresholds), "cl4" / "cl2" (the thresholds follow the device's compute units), "big64" (R > 4096 through the common entry
    points), "bwd_big" (mobgt_layer_chain_bwd_big at any R).  The cross is thinned PAIRWISE: every (width, form), (R edge, form up to
    its threshold), (family, form), (dropout mode, form), (layer kind, tail), (passenger count, cluster or not) pair occurs
    (tests/test_host_chain_reference.py asserts it); an axis is never dropped."""
    specs = []
    r4, r2 = 16 * (min(cus, 256) // 4), 16 * (min(cus, 256) // 2)       # the largest R of the 4- and the 2-member form

    def add(dir, form, C, R, family="plain", mode=0, preln=False, successor=True, last=False, tail=False, n_wg=0, with_db=True):
        p, seed_mode = DROP_MODES[mode % 3]
        if preln and not successor:
            last, tail = True, False
        specs.append(dict(dir=dir, form=form, C=C, R=R, family=family, p=p, seed_mode=seed_mode, preln=preln, successor=successor,
                          last=last, tail=tail, n_wg=n_wg if dir != "fwd" and form not in ("big64", "bwd_big") else 0, with_db=with_db))
    # R around the 16- and 64-row edges: every R in the one-workgroup and the 4-member form both ways, and through the 64-row entry point
    for i, R in enumerate(R16 + R64):
        C = WIDTHS[i % 3]
        for k, form in enumerate(("one", "cl4")):
            add("fwd", form, C, R, mode=i + k, last=i % 4 == 3)
            add("bwd", form, C, R, mode=i + k, tail=(i + k) % 2 == 0, n_wg=(0, 1, 4)[(i + k) % 3], with_db=i % 2 == 0)
        add("bwd", "bwd_big", C, R, mode=i + 2, tail=i % 2 == 1)
    # the 2-member form and the thresholds
    for i, (R, form) in enumerate(((r4 + 1, "cl2"), (r4 + 16, "cl2"), (r2, "cl2"), (r2 + 1, "ws_one"), (r4, "cl4"))):
        C = WIDTHS[(i + 1) % 3]
        add("fwd", form, C, R, mode=i, last=i == 1)
        add("bwd", form, C, R, mode=i, tail=i % 2 == 0, n_wg=(4, 0, 1, 0, 0)[i], with_db=i != 0)
    for i, R in enumerate((BIG_ROWS, BIG_ROWS + 1, BIG_ROWS + 54, BIG_ROWS + 64)):
        C = WIDTHS[i % 3]
        form = "one" if R <= BIG_ROWS else "big64"
        add("fwd", form, C, R, mode=i + 1, last=i == 2)
        add("bwd", form, C, R, mode=i + 1)                                  # (no guests past 4 096 rows through this entry point)
    add("bwd", "bwd_big", 256, BIG_ROWS + 54, mode=2, tail=True)
    add("bwd", "bwd_big", 128, BIG_ROWS, mode=1)
    # every family in every form
    for i, fam in enumerate(FAMILIES):
        if fam == "plain":
            continue
        C, R = WIDTHS[i % 3], (33, 65, 17)[i % 3]
        for k, form in enumerate(("one", "cl4")):
            add("fwd", form, C, R, fam, mode=i + k)
            add("bwd", form, C, R, fam, mode=i + k, tail=True)
        add("bwd", "bwd_big", C, R, fam, mode=i, tail=True)
        add("fwd", "cl2", 128, r4 + 1, fam, mode=i)
        add("bwd", "cl2", 128, r4 + 1, fam, mode=i, tail=i % 2 == 0)
        add("fwd", "big64", 128, BIG_ROWS + 1, fam, mode=i + 1)
        add("bwd", "big64", 128, BIG_ROWS + 1, fam, mode=i + 1)
    add("bwd", "bwd_big", 192, BIG_ROWS + 1, "plain", mode=0, tail=True)
    # pre-LN (C = 128): forward with and without successor, backward with and without tail, in the 16-row forms
    for i, (R, form) in enumerate(((33, "one"), (17, "cl4"), (r4 + 1, "cl2"), (65, "cl4"))):
        add("fwd", form, 128, R, mode=i, preln=True, successor=True, last=i == 3)
        add("fwd", form, 128, R, mode=i + 1, preln=True, successor=False)
        add("bwd", form, 128, R, mode=i, preln=True, tail=True, n_wg=(1, 0, 4, 0)[i])
        add("bwd", form, 128, R, mode=i + 1, preln=True, tail=False, n_wg=(0, 4, 0, 1)[i], with_db=False)
        add("bwd", form, 128, R, mode=i + 2, preln=True, successor=False)
    # forward, then backward on the device's own saved tensors: once per form
    for i, (form, R) in enumerate((("one", 33), ("cl4", 65), ("cl2", r4 + 16), ("big64", BIG_ROWS + 54), ("bwd_big", 333))):
        add("both", form, WIDTHS[i % 3], R, mode=1 + i % 2, tail=form != "big64", n_wg=1 if form in ("one", "cl4", "cl2") else 0)
    add("both", "cl4", 128, 33, mode=1, preln=True, tail=True)
    seen, out = set(), []
    for s in specs:
        k = spec_id(s, cus)
        if k not in seen:
            seen.add(k)
            out.append(s)
    return out


def spec_case(s, keep_fn=host_keep, seed=77):
    return make_case(s["C"], s["R"], s["family"], p_drop=s["p"], preln=s["preln"], successor=s["successor"], tail=s["tail"], last=s["last"],
                     n_wg=s["n_wg"], with_db=s["with_db"], seed=seed, keep_fn=keep_fn)


def spec_split(s):
    """The partial sums dz is formed from in the form the spec reaches."""
    return {"one": 1, "ws_one": 1, "cl4": 4, "cl2": 2, "big64": 3, "bwd_big": 3}[s["form"]]
