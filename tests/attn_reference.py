"""What the attention kernels (csrc/attn.hip, csrc/attn_f32_body.h) are judged against, independent of the library.

  * `reference`   graphormer/model.py:436-455 in float64 on the CPU through torch autograd, on the inputs as given;
  * `emulation`   the same mathematics in float64 with a hand-written backward and bf16 rounding at exactly the points the kernels'
                  documented design rounds (header comment of attn.hip, "consistent softmax", and the comments of the three backward
                  forms).  It is the yardstick for tolerances: tolerance = 2 x (emulation against reference) per case and tensor;
  * `make_case`   seeded inputs of the families the GPU matrix runs;
  * `compare`     the one metric: per HEAD ROW relative error, next to the relative L2 and the largest element error of a tensor;
  * `mutant`      deliberately wrong float64 references (a lost key, a skipped chunk, a transposed mask ...) that `compare` must reject
                  at those tolerances -- tests/test_host_attn_reference.py shows it without a GPU.

Nothing in here imports mobgt_amd.  Dropout keep masks come from the caller (`keep_fn`): the host tests draw Bernoulli masks, the GPU
tests replay the kernels' rule (ops.dropout_keep_mask).
"""
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch

LOG2E = 1.4426950408889634

# Below this, an error is f32 arithmetic, not a rounding point: the kernels accumulate in f32, and the output row the backward's
# delta is formed from is carried as bf16 + a bf16 residual (16 significand bits: 2^-17 relative per element; with |V|, |K| ~ sqrt(d)
# <= 5.7 and scale = d^-1/2 that is at most 5.7 * 2^-17 = 4.3e-5 of |dO| in a dQ row whose true value is zero).  Tolerances never
# go below it, so a case whose emulation is EXACT (one valid key: P = 1) still admits f32 noise -- and nothing a bf16 output (2^-9)
# could show.
TOL_FLOOR = 2.0 ** -12
# tests/test_gpu_c5.py: relative L2 <= 1e-2, element error <= 1.5e-2 * max|ref|.  No tolerance outside the common-mode family exceeds them.
C5_L2, C5_ELEM = 1e-2, 1.5e-2
ROW_FLOOR = 0.05              # a head row's error is divided by max(its norm, ROW_FLOOR * the tensor's largest row norm)
FLOOR_SHARE_CAP = 0.10        # at most this share of the judged rows of a tensor may lie below that floor


def bf16r(t):
    """Round to bf16, keep the dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _heads(x, H):
    G, T, C = x.shape
    return x.view(G, T, H, C // H).transpose(1, 2)


def _merge(x):
    G, H, T, d = x.shape
    return x.transpose(1, 2).reshape(G, T, H * d)


# ------------------------------------------------------------------------------------------------ reference
def reference(q, k, v, gy, bias, H, scale, keep=None, inv_keep=1.0):
    """model.py:436-455 and its autograd in float64: q = q * scale; x = q k^T + bias; softmax; dropout; x v.
    Returns dict(out, dq, dk, dv, dbias); dbias of -inf entries is 0."""
    q, k, v, b = (t.detach().to(torch.float64).clone().requires_grad_(True) for t in (q, k, v, bias))
    x = _heads(q * scale, H) @ _heads(k, H).transpose(2, 3) + b
    p = torch.softmax(x, dim=3)
    if keep is not None:
        p = p * keep.to(torch.float64) * inv_keep
    out = _merge(p @ _heads(v, H))
    out.backward(gy.to(torch.float64))
    db = b.grad.clone()
    db[torch.isinf(bias)] = 0.0
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dbias=db)


# ------------------------------------------------------------------------------------------------ emulation
def emulation(q, k, v, gy, bias, H, scale, keep=None, inv_keep=1.0, form="two", dbias_f32=False, delta_from_rounded_out=False):
    """The kernels' arithmetic in float64 with their bf16 rounding points (r = round to bf16; inputs are bf16 values already).

    forward (attn_fwd_kernel):  qs = r(q scale);  x = (qs . k + bias) log2 e;  integer M = ceil(max_j x);  P_b = r(2^(x - M));
        l = sum_j P_b (the ROUNDED probabilities, before dropout);  O = sum_j keep P_b v / l / (1 - p) unrounded;  out = r(O).
        (The backward's M' = rint(lse log2 e) is another integer: bf16 rounding commutes with the power of two between them.)
    backward, form "two" (attn_bwd_dq_kernel + attn_bwd_dkv_kernel; the T <= 64 attn_bwd_both_kernel runs the same two bodies):
        dQ pass:   dO~ = r(dO / l);  delta = dO~ . O (O unrounded: bf16 O + its bf16 residual);  dP = dO~ . v;
                   dS = P_b (keep dP / (1 - p) - delta): the f32 dBias as it is, r(dS) is the bf16 dBias slice and what dQ sums;
                   dq = r(scale sum_j r(dS) k).
        dK/dV pass: the scale rides on K: x' = (q . r(k scale) + bias) log2 e, P_b' = r(2^(x' - M));  delta' = dO . O;
                   v' = r(v / (1 - p));  dP' = dO . v';  X = keep P_b';  dv = r(sum_i r(X / l) dO / (1 - p));
                   dk = r(scale sum_i r((X dP' - P_b' delta') / l) q).
    backward, form "one" (attn_bwd_one_kernel + attn_dq_finish_kernel): the scale rides on the staged Q rows, so x and P_b are the
        forward's; dO~ and delta as in the dQ pass, v' as in the dK/dV pass;  dP = dO~ . v';  X = keep P_b;  dS = r(X dP - P_b delta)
        is the dBias slice;  dv = r(sum_i X dO~ / (1 - p));  dk = r(sum_i dS qs);  dq = r(scale sum_j dS k).
    `delta_from_rounded_out`: delta from out = r(O) alone -- the inconsistency the consistent-softmax rework removed."""
    f8 = torch.float64
    qh, kh, vh, dO = (_heads(t.to(f8), H) for t in (q, k, v, gy))
    bias = bias.to(f8)
    kp = None if keep is None else keep.to(f8)
    r = bf16r
    x = (r(qh * scale) @ kh.transpose(2, 3) + bias) * LOG2E
    M = torch.ceil(x.max(dim=3, keepdim=True).values)
    Pb = r(torch.exp2(x - M))
    l = Pb.sum(dim=3, keepdim=True)
    O = ((Pb if kp is None else Pb * kp) @ vh) / l * inv_keep
    out = r(O)
    Od = out if delta_from_rounded_out else O
    res = dict(out=_merge(out))
    if form == "two":
        dOt = r(dO / l)
        delta = (dOt * Od).sum(dim=3, keepdim=True)
        dP = dOt @ vh.transpose(2, 3)
        dd = dP - delta if kp is None else torch.where(kp > 0, dP * inv_keep - delta, -delta)
        dS = Pb * dd
        dSb = r(dS)
        res["dq"] = _merge(r(scale * (dSb @ kh)))
        res["dbias"] = dS if dbias_f32 else dSb
        x2 = (qh @ r(kh * scale).transpose(2, 3) + bias) * LOG2E
        Pb2 = r(torch.exp2(x2 - M))
        delta2 = (dO * Od).sum(dim=3, keepdim=True)
        v2 = vh if kp is None else r(vh * inv_keep)
        dP2 = dO @ v2.transpose(2, 3)
        X = Pb2 if kp is None else Pb2 * kp
        res["dv"] = _merge(r(inv_keep * (r(X / l).transpose(2, 3) @ dO)))
        res["dk"] = _merge(r(scale * (r((X * dP2 - Pb2 * delta2) / l).transpose(2, 3) @ qh)))
    elif form == "one":
        assert not dbias_f32, "the one-pass backward writes a bf16 dBias slice"
        qs = r(qh * scale)                           # the staged Q rows carry the scale: S and P_b are the forward's
        dOt = r(dO / l)
        delta = (dOt * Od).sum(dim=3, keepdim=True)
        v2 = vh if kp is None else r(vh * inv_keep)
        dP = dOt @ v2.transpose(2, 3)
        X = Pb if kp is None else Pb * kp
        dS = r(X * dP - Pb * delta)
        res["dv"] = _merge(r(inv_keep * (X.transpose(2, 3) @ dOt)))
        res["dk"] = _merge(r(dS.transpose(2, 3) @ qs))
        res["dq"] = _merge(r(scale * (dS @ kh)))
        res["dbias"] = dS
    else:
        raise ValueError(form)
    return res


# ------------------------------------------------------------------------------------------------ cases
STEEP_EVERY = 16             # family "steep": every 16th query row has the steep bias
FAMILIES = ("plain", "one_key", "common", "steep", "many", "two_use")


def default_n_real(T, G):
    """[T, max(1, T - 1 - 3g), ...]; from T = 129 on the LAST graph has its whole trailing 64-key chunk masked (and a tail inside the
    chunk before it)."""
    n = [T] + [max(1, T - 1 - 3 * g) for g in range(1, G)]
    if T >= 129:
        n[-1] = 64 * ((T + 63) // 64 - 1) - 5
    return n


def host_keep(seed, G, H, T, p_drop):
    """Bernoulli keep mask for the host tests (the GPU tests replay the kernels' own rule instead)."""
    thr = int(p_drop * 65536 + 0.5)
    rs = np.random.RandomState(seed & 0x7FFFFFFF)
    return rs.randint(0, 65536, size=(G, H, T, T)) >= thr


def make_case(T, d, H, G=3, family="plain", p_drop=0.0, bias_dtype="bf16", io="bf16", a=4.0, seed=0x5DEECE66D1234567,
              keep_fn=host_keep, n_real=None, variant=0):
    """Seeded inputs.  q, k, v, gy ~ N(0, 1) [G, T, H d], rounded to bf16 (io "bf16") or f32; bias as make_bias of
    test_gpu_kernels.py: N(0, 0.7) [G, H, T, T], -inf for keys >= n_real[g], rounded to `bias_dtype`.  Families:
      plain     n_real = default_n_real
      one_key   G = 3, n_real = [1, 4, 8]: one valid key (P = 1: out = v[g, 0] exactly, dq = dk = dbias = 0) beside graphs of four and
                eight keys.  (A graph of T keys beside them puts most rows of the short graphs below the row floor: measured share 0.5-0.98;
                graphs of two and three keys have a fifth of their rows near one-hot: 0.21.  With [1, 4, 8] the share is <= 0.083.)
      common    k += a ck[g] and v += a cv[g], one vector per graph shared by all its keys (MobGT's fused user embedding passes through
                both projections).  With k alone an inconsistent delta does not stand out on N(0, 1) data (0.5-1.5 x the tolerance
                for a = 4, 8, 16): the common part of v is what makes |O|, hence the error of delta, large next to dP - delta.
      steep     bias scale 6.0 on every STEEP_EVERY-th query row (near one-hot rows, a running maximum that climbs from chunk to chunk);
                the other rows keep 0.7 and get one N(0, 6) offset per row, so row maxima spread over about +-20 everywhere.  (Scale
                6.0 on EVERY row leaves 23-41 % of the dq / dbias rows below the row floor: near-one-hot rows have no gradient.)
      (`variant` only re-seeds: T = 2 has 8 judged dq rows, where ONE row below the floor already breaks the 10 % cap.)
      many      as plain with whatever (large) G, H the caller gives
      two_use   a second set q2, k2, v2, gy2 for a second attention call on the same bias
    With p_drop: keep = keep_fn(seed, G, H, T, p_drop) (bool [G, H, T, T]), inv_keep from the kernels' 16-bit threshold."""
    assert family in FAMILIES, family
    if family == "one_key":
        G, n_real = 3, [1, 4, 8]
    if n_real is None:
        n_real = default_n_real(T, G)
    n_real = [min(int(n), T) for n in n_real]
    assert len(n_real) == G and min(n_real) >= 1
    C = H * d
    key = (T, d, H, G, family, float(p_drop), bias_dtype, io, float(a) if family == "common" else 0.0, seed if p_drop else 0,
           tuple(n_real), getattr(keep_fn, "__name__", "keep") if p_drop else "", variant)
    rng = np.random.RandomState(zlib.crc32(repr(key[:5] + key[8:9] + (variant,)).encode()) & 0x7FFFFFFF)
    rnd = (lambda t: bf16r(t)) if io == "bf16" else (lambda t: t.to(torch.float32).to(torch.float64))

    def normal(*shape):
        return torch.from_numpy(rng.standard_normal(shape))
    q, k, v, gy = (normal(G, T, C) for _ in range(4))
    if family == "common":
        k = k + a * normal(G, 1, C)
        v = v + a * normal(G, 1, C)
    b = normal(G, H, T, T) * 0.7
    if family == "steep":
        b[:, :, ::STEEP_EVERY] *= 6.0 / 0.7
        b[:, :, :] += torch.where(torch.arange(T).view(1, 1, T, 1) % STEEP_EVERY == 0, 0.0, 1.0) * 6.0 * normal(G, H, T, 1)
    for g in range(G):
        b[g, :, :, n_real[g]:] = -math.inf
    b = bf16r(b) if bias_dtype == "bf16" else b.to(torch.float32).to(torch.float64)
    case = SimpleNamespace(T=T, d=d, H=H, G=G, C=C, family=family, p_drop=float(p_drop), bias_dtype=bias_dtype, io=io, seed=seed,
                           n_real=n_real, scale=d ** -0.5, key=key, q=rnd(q), k=rnd(k), v=rnd(v), gy=rnd(gy), bias=b,
                           keep=None, inv_keep=1.0)
    if family == "two_use":
        case.q2, case.k2, case.v2, case.gy2 = (rnd(normal(G, T, C)) for _ in range(4))
    if p_drop:
        case.keep = torch.from_numpy(np.ascontiguousarray(keep_fn(seed, G, H, T, p_drop))).to(torch.float64)
        case.inv_keep = 1.0 / (1.0 - int(p_drop * 65536 + 0.5) / 65536.0)
    return case


def _uses(case):
    yield "", (case.q, case.k, case.v, case.gy)
    if case.family == "two_use":
        yield "2", (case.q2, case.k2, case.v2, case.gy2)


def _run(fn, case, overwrite_second=False, **kw):
    """`fn` (reference / emulation / a mutant's) on every use of the case's bias: out, dq, dk, dv (+ out2 ... for the second use),
    dbias = the SUM over uses."""
    res = {}
    for tag, (q, k, v, gy) in _uses(case):
        r = fn(q, k, v, gy, case.bias, case.H, case.scale, case.keep, case.inv_keep, **kw)
        for name in ("out", "dq", "dk", "dv"):
            res[name + tag] = r[name]
        res["dbias"] = r["dbias"] if "dbias" not in res or overwrite_second else res["dbias"] + r["dbias"]
    return res


_CACHE = {}


def _cached(kind, case, make):
    k = (kind,) + case.key
    if k not in _CACHE:
        if len(_CACHE) > 64:                       # (references of T = 513 are tens of MB each)
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[k] = make()
    return _CACHE[k]


def case_reference(case):
    return _cached("ref", case, lambda: _run(reference, case))


def case_emulation(case, form="two", dbias_f32=False, delta_from_rounded_out=False):
    return _cached(("emu", form, dbias_f32, delta_from_rounded_out), case,
                   lambda: _run(emulation, case, form=form, dbias_f32=dbias_f32, delta_from_rounded_out=delta_from_rounded_out))


# ------------------------------------------------------------------------------------------------ the metric
def _kind(name):
    return name.rstrip("2")


def measure(got, want, case, name):
    """One tensor: dict(row, l2, elem, floor_share, zero, n_judged).
      row    max over judged head rows of ||got - want|| / max(||want row||, ROW_FLOOR * max row norm of the tensor).  A head row: the d
             elements of (g, t, h) for out / dq / dk / dv, the VALID keys of (g, h, i) for dbias;
      zero   rows of a graph whose reference is identically zero (one valid key: dq, dk, dbias) are counted apart, absolutely:
             max ||got row|| / max row norm of the output gradient gy (the scale of every gradient here: dS = P (dP - delta), dP = dO . v);
      l2     ||got - want|| / ||want|| over the whole tensor;   elem  max |got - want| / max |want|;
      floor_share  share of the judged rows whose reference norm lies below the floor.
    Rows (dk, dv) and columns (dbias) of padded keys are not judged here: `assert_padding_zero`."""
    kind = _kind(name)
    g64, w64 = got.detach().to(torch.float64).cpu(), want.detach().to(torch.float64).cpu()
    assert g64.shape == w64.shape, (name, g64.shape, w64.shape)
    assert bool(torch.isfinite(g64).all()), f"{name}: non-finite values"
    G = case.G
    if kind == "dbias":
        valid = torch.zeros(G, 1, 1, case.T, dtype=torch.bool)
        for g in range(G):
            valid[g, ..., : case.n_real[g]] = True
        err = ((g64 - w64) * valid).pow(2).sum(3).sqrt()           # [G, H, T]
        nrm = (w64 * valid).pow(2).sum(3).sqrt()
        judged = torch.ones_like(nrm, dtype=torch.bool)
        diff_all, want_all = (g64 - w64) * valid, w64 * valid
    else:
        e4 = (g64 - w64).view(G, case.T, case.H, case.d)
        err = e4.pow(2).sum(3).sqrt()                              # [G, T, H]
        nrm = w64.view(G, case.T, case.H, case.d).pow(2).sum(3).sqrt()
        judged = torch.ones_like(nrm, dtype=torch.bool)
        if kind in ("dk", "dv"):
            for g in range(G):
                judged[g, case.n_real[g]:] = False
        diff_all, want_all = e4 * judged.unsqueeze(3), w64.view(G, case.T, case.H, case.d) * judged.unsqueeze(3)
    zero_graph = torch.tensor([bool((w64[g] == 0).all()) for g in range(G)]).view(G, 1, 1)
    gy_scale = float(_heads(case.gy.to(torch.float64), case.H).pow(2).sum(3).sqrt().max())
    zsel = judged & zero_graph
    jsel = judged & ~zero_graph
    zero = float((err[zsel] / gy_scale).max()) if bool(zsel.any()) else 0.0
    if bool(jsel.any()):
        floor = ROW_FLOOR * float(nrm[jsel].max())
        row = float((err[jsel] / nrm[jsel].clamp_min(floor)).max())
        share = float((nrm[jsel] < floor).double().mean())
    else:
        row, share = 0.0, 0.0
    wn, wm = float(want_all.norm()), float(want_all.abs().max())
    l2 = float(diff_all.norm()) / wn if wn > 0 else 0.0
    elem = float(diff_all.abs().max()) / wm if wm > 0 else 0.0
    return dict(row=row, zero=zero, l2=l2, elem=elem, floor_share=share, n_judged=int(jsel.sum()))


def tolerances(case, form="two", dbias_f32=False, with_dbias=True):
    """Per tensor: 2 x what `measure` gives the emulation against the float64 reference on this very case, never below TOL_FLOOR
    and -- outside the common-mode family -- never above the c5 ceilings (relative L2, element error)."""
    ref, emu = case_reference(case), case_emulation(case, form, dbias_f32)
    tol = {}
    for name in emu:
        if name == "dbias" and not with_dbias:
            continue
        m = measure(emu[name], ref[name], case, name)
        t = {k: max(2.0 * m[k], TOL_FLOOR) for k in ("row", "zero", "l2", "elem")}
        if case.family != "common":
            t["l2"], t["elem"] = min(t["l2"], C5_L2), min(t["elem"], C5_ELEM)
        t["emu"] = m
        tol[name] = t
    return tol


def compare(got, want, tol, case, label=""):
    """Every tensor of `tol` in `got` against `want`: returns {name: measure(...)} and, in "fail", the list of (name, metric, value,
    tolerance) that exceed `tol`.  `check` asserts that list empty."""
    rep, fail = {}, []
    for name, t in tol.items():
        m = measure(got[name], want[name], case, name)
        rep[name] = m
        for k in ("row", "zero", "l2", "elem"):
            if not m[k] <= t[k]:
                fail.append((name, k, m[k], t[k]))
    rep["fail"] = fail
    return rep


def worst_ratio(rep, tol):
    """max over tensors and metrics of measured / tolerance."""
    return max(rep[n][k] / tol[n][k] for n in tol for k in ("row", "zero", "l2", "elem"))


def format_report(rep, tol, label):
    lines = []
    for n in tol:
        m, t = rep[n], tol[n]
        lines.append("%s %-6s row %.2e/%.2e  l2 %.2e/%.2e  elem %.2e/%.2e  zero %.1e/%.1e  emu row %.2e l2 %.2e  floor share %.3f"
                     % (label, n, m["row"], t["row"], m["l2"], t["l2"], m["elem"], t["elem"], m["zero"], t["zero"],
                        t["emu"]["row"], t["emu"]["l2"], m["floor_share"]))
    return "\n".join(lines)


def check(got, want, tol, case, label=""):
    rep = compare(got, want, tol, case, label)
    print(format_report(rep, tol, label))
    assert not rep["fail"], "%s: beyond tolerance (tensor, metric, value, tolerance): %s" % (label, rep["fail"])
    return rep


def assert_padding_zero(got, case):
    """Padded keys receive EXACTLY zero gradient: their dk / dv rows and their dbias columns (as tests/test_gpu_c5.py asserts)."""
    for name, t in got.items():
        kind = _kind(name)
        for g, n in enumerate(case.n_real):
            if n >= case.T:
                continue
            if kind in ("dk", "dv"):
                assert float(t[g, n:].abs().max()) == 0.0, (name, g, n)
            elif kind == "dbias":
                assert float(t[g, :, :, n:].abs().max()) == 0.0, (name, g, n)


def floor_shares(case, ref=None):
    """{tensor: share of judged rows below the row floor} of the case's reference."""
    ref = ref or case_reference(case)
    return {n: measure(ref[n], ref[n], case, n)["floor_share"] for n in ref}


# ------------------------------------------------------------------------------------------------ mutants
MUTANTS = ("keep_transposed", "key_dropped", "last_key_dropped", "chunk_skipped", "bias_transposed", "second_use_overwrites")


def mutant(case, which):
    """A deliberately wrong float64 reference of `case` (what a subtly broken kernel would compute), or None where the defect does
    not exist for the case (no dropout: no keep mask; one use: nothing to overwrite; no room for the lost piece).
      keep_transposed        keep[i, j] read as keep[j, i]
      key_dropped            one valid key (the middle one) lost for ONE (graph, head)
      last_key_dropped       key n_real - 1 lost for one (graph, head): a tail mask one short
      chunk_skipped          one 64-key chunk (T <= 64: one 32-key tile) lost for the 32 query rows of one wave tile of one (graph, head)
      bias_transposed        bias[g, h] read transposed for one head among the valid keys (-inf columns stay in place)
      second_use_overwrites  the second use's dbias replaces the first's instead of adding to it"""
    G, H, T = case.G, case.H, case.T
    g = max(range(G), key=lambda i: (case.n_real[i] < T, case.n_real[i]))      # the largest graph that has padded keys, else graph 0
    n, h = case.n_real[g], H - 1
    if which == "second_use_overwrites":
        return _run(reference, case, overwrite_second=True) if case.family == "two_use" else None
    c2 = SimpleNamespace(**vars(case))
    if which == "keep_transposed":
        if case.keep is None:
            return None
        c2.keep = case.keep.transpose(2, 3).contiguous()
        return _run(reference, c2)
    b = case.bias.clone()
    if which == "key_dropped":
        if n < 2:
            return None
        b[g, h, :, n // 2] = -math.inf
    elif which == "last_key_dropped":
        if n < 2:
            return None
        b[g, h, :, n - 1] = -math.inf
    elif which == "chunk_skipped":
        w = 64 if T > 64 else 32
        g = max(range(G), key=lambda i: case.n_real[i])
        n = case.n_real[g]
        if n <= w:
            return None
        c0 = ((n - w) // w) * w                    # the last whole chunk below n
        i0 = max(0, ((T - 32) // 32) * 32)         # the last whole 32-row tile
        b[g, h, i0:i0 + 32, c0:c0 + w] = -math.inf
    elif which == "bias_transposed":
        if n < 2:
            return None
        b[g, h, :n, :n] = case.bias[g, h, :n, :n].transpose(0, 1)
    else:
        raise ValueError(which)
    c2.bias = b
    return _run(reference, c2)


# ------------------------------------------------------------------------------------------------ the matrix
T_ALL = (1, 2, 17, 31, 32, 33, 48, 63, 64, 65, 96, 97, 127, 128, 129, 160, 191, 192, 193, 257, 300, 513)
T_DROP = (17, 33, 64, 65, 130, 300)
D_ALL = (16, 24, 32)
T2_VARIANT = {16: 0, 24: 4, 32: 0}      # (make_case: `variant`)

# backward forms: name -> (bias dtype, wants dBias, two-pass forced, emulation form for T <= 64 / T > 64, f32 dBias)
#   slice     bf16 bias + bf16 dBias slice: attn_bwd_both_kernel (T <= 64), attn_bwd_one_kernel + attn_dq_finish_kernel (T > 64)
#   slice2p   the same through attn_bwd_dq_kernel + attn_bwd_dkv_kernel (T > 64 only)
#   f32acc    f32 bias + f32 dBias accumulator: both-kernel / the two passes
#   nodb      bf16 bias, no bias gradient: both-kernel / the two passes
FORMS = {"slice": ("bf16", True, False), "slice2p": ("bf16", True, True), "f32acc": ("f32", True, False), "nodb": ("bf16", False, False)}


def forms_for(T):
    return ("slice", "f32acc", "nodb") if T <= 64 else ("slice", "slice2p", "f32acc", "nodb")


def emu_form(T, form):
    return "one" if (T > 64 and form == "slice") else "two"


def heads_for(T):
    return 4 if T % 2 else 8


def spec_id(s):
    return "%s-T%d-d%d-H%d-%s-p%s%s" % (s["family"], s["T"], s["d"], s["H"], s["form"], ("%g" % s["p_drop"]).replace(".", ""),
                                         ("-" + s["seed_mode"]) if s["p_drop"] else "")


def matrix_specs():
    """Every case of the bf16 matrix as a dict(family, T, d, H, G, form, p_drop, seed_mode).  The dropout x T x d x form cross is
    thinned pairwise (the full cross made the GPU file slower than tests/test_gpu_kernels.py): every (T, form) runs p = 0.1 and
    p = 0.5 at two different d, one with the seed wholly on the host and one split into host + device word; every pair (T, d),
    (d, form), (d, p), (form, p), (form, seed mode) occurs (tests/test_host_attn_reference.py asserts it)."""
    specs = []

    def add(family, T, d, form, p=0.0, mode="host", H=None, G=3):
        specs.append(dict(family=family, T=T, d=d, H=H or heads_for(T), G=G, form=form, p_drop=p, seed_mode=mode))
    for T in T_ALL:
        for d in D_ALL:
            for form in forms_for(T):
                add("plain", T, d, form)
    for it, T in enumerate(T_DROP):                                # two cases per (T, form): p = 0.1 and p = 0.5, the d's rotating
        for i, form in enumerate(forms_for(T)):
            flip = (it + i) % 2
            add("plain", T, D_ALL[(it + i) % 3], form, 0.1, "split" if flip else "host")
            add("plain", T, D_ALL[(it + i + 1 + it // 3) % 3], form, 0.5, "host" if flip else "split")
    for T, d in ((130, 24), (300, 32)):                            # many (graph, head) pairs: choose_nq, uneven tile dealing
        add("many", T, d, "slice", H=8, G=16)
    add("many", 130, 16, "slice2p", H=8, G=16)
    for T in (33, 130):
        for d in D_ALL:
            for form in ("slice", "f32acc") + (("slice2p",) if T > 64 else ()):
                add("two_use", T, d, form)
            add("one_key", T, d, "slice")
            add("one_key", T, d, "slice2p" if T > 64 else "f32acc", 0.1, "split")
    for T in (33, 130, 300):
        for d in D_ALL:
            for form in ("slice", "f32acc") + (("slice2p",) if T > 64 else ()):
                add("common", T, d, form)
    for T in (33, 64, 130):
        for d in D_ALL:
            for form in ("slice", "f32acc"):
                add("steep", T, d, form)
    add("two_use", 130, 32, "slice", 0.1, "split")
    add("plain", 17, 16, "f32acc", 0.5, "split")                   # (NW = 1 with dropout and an f32 bias at d = 16: the rotation above misses it)
    return specs


_A_CACHE = {}


def choose_a(T, d, H, form):
    """Family "common": the smallest a of 4, 8, 16 for which the emulation with delta taken from the ROUNDED output exceeds the
    case's tolerance three times (chosen on the CPU, from the emulation alone)."""
    k = (T, d, H, form)
    if k not in _A_CACHE:
        _A_CACHE[k] = None
        for a in (4.0, 8.0, 16.0):
            case = make_case(T, d, H, family="common", a=a, bias_dtype=FORMS[form][0])
            ef, f32 = emu_form(T, form), form == "f32acc"
            tol = tolerances(case, ef, f32)
            rep = compare(case_emulation(case, ef, f32, True), case_reference(case), tol, case)
            if worst_ratio(rep, tol) >= 3.0:
                _A_CACHE[k] = a
                break
    return _A_CACHE[k]


def spec_case(s, keep_fn=host_keep):
    a = choose_a(s["T"], s["d"], s["H"], s["form"]) if s["family"] == "common" else 0.0
    assert a is not None, "no a of 4, 8, 16 separates the inconsistent delta: %r" % (s,)
    return make_case(s["T"], s["d"], s["H"], G=s["G"], family=s["family"], p_drop=s["p_drop"], bias_dtype=FORMS[s["form"]][0], a=a or 4.0,
                     keep_fn=keep_fn, variant=T2_VARIANT[s["d"]] if s["T"] == 2 else 0)


def spec_tolerances(s, case):
    return tolerances(case, emu_form(s["T"], s["form"]), s["form"] == "f32acc", with_dbias=FORMS[s["form"]][1])
