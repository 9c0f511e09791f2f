"""What the encoder-input kernels are judged against (csrc/layer.hip assemble_tokens_kernel, csrc/chain.hip assemble_qkv_kernel and
token_fwd_chain_kernel, csrc/tokbwd.hip, csrc/embed.hip gather_multi_kernel), written from the MODEL's expressions, stage by stage,
in float64 on the CPU:

    gathers      model_fqandtoyo.py:1259-1264, 1288-1298, 348-351: rows of tables at index lists, -1 = no row (zeros); `[poi | time]`
                 side by side -> pt, the category row -> the trailing columns of x4, the SUM of the additive rows -> add; a folded
                 table (accum = 2) is one more summand of the job in front of it, read at that job's index
    fuse         :444-456, :1268-1269   f2 = leaky(pt W2^T + b2);  x4 = [f2 | cat];  nf = leaky(x4 W4^T + b4)
    assembly     :1287-1298, 348-358, 1338-1347   out[g, 0] = drop_in(drop_pos(token + pe[0])),
                 out[g, 1 + n] = drop_in(drop_pos(nf[g, n] * real[g, n] + add[g, n]));  the keep masks are drawn per SITE with three
                 salts and three row numberings: salt_nf rows g N + n, salt_tok rows g, salt_in rows g T + t
    qkv          the first layer's projection of the bf16 rows: rows16 Wq^T + bq
    backward     d = dout * masks;  d_add = d;  d_nf = d * real;  dx4 = (d_nf * leaky'(nf)) W4;  d_pt = (dx4[:, :W2] * leaky'(f2)) W2;
                 d_token += sum over graphs of the token rows' d;  leaky' is taken from the OUTPUT and is the slope at 0;  the
                 scatter adds a gradient buffer's rows into the tables, skipping `skip` rows (nn.Embedding's padding_idx),
                 negative indices and tables without a gradient;  extra_row0 (the graph token's share of pe[0]) goes to row 0

  * `forward` / `backward`   the stages composed (tests/test_host_token_reference.py holds them to torch autograd);
  * `emulate_*`              what a correct device run returns: the exact stages (gathers, assembly, d_add / d_nf) in f32 in the
                             documented order, the products in float64 rounded once -- and, with `mut`, a deliberately wrong one;
  * `judge_*`                the verdicts of tests/test_gpu_token_matrix.py, stage by stage on the GIVEN upstream tensors: bit equality
                             where exactness is the contract, else the forward bound of an f32 dot product of K terms in any order,
                             |got - ref| <= (K + 2) 2^-24 (sum_k |a_k| |w_k| + |b|), computed in float64 from the operands (K terms, the
                             bias add, the activation's multiply; nothing fitted to a device);
  * `make_case`, `fwd_specs` ...   the seeded cases of the GPU matrix.

Keep masks come from `keep_fn(seed, salt, R, C, p)`; the default replays the kernels' counter hash on the host
(mobgt_amd.ops.dropout_site_mask -- a host function of the library, no GPU needed)."""
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from chain_reference import inv_keep_of

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
C_FUSED, W2_FUSED = 192, 160
SALTS = (0x1001, 0x1002, 0x1003)                                 # nf, tok, in
GUARD, SENT = 3, 123.0
TOKEN_INIT, TABLE_INIT = 3.25, 1.5                               # what the accumulated buffers hold before a call
LAYOUTS = {"one160": ((160, 0),), "128+32": ((128, 0), (32, 128)), "64+32at128": ((64, 0), (32, 128))}
ADD_NAMES = {1: ("pos",), 2: ("fre", "pos"), 4: ("fre", "indeg", "outdeg", "pos")}
TABLE_ROWS = dict(poi=64, time=48, cat=17, fre=3, indeg=9, outdeg=9, pos=40)
SKIP = dict(time=0, fre=0, indeg=0, outdeg=0)                    # padding_idx of the model's tables (poi, cat, pos: none)


def site_keep(seed, salt, R, C, p):
    from mobgt_amd import ops
    return ops.dropout_site_mask(seed, salt, R, C, p) if R > 0 else np.ones((0, C), dtype=bool)


def f32r(t):
    return t.to(F32).to(F64)


def leaky(x, slope):
    return torch.where(x > 0, x, slope * x)


def leaky_grad(y, slope):
    """From the activation's OUTPUT (slope > 0: same sign as the input); at 0 the slope, as F.leaky_relu's backward."""
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))


# ------------------------------------------------------------------------------------------------ cases
def lengths_of(G, N, pad):
    """Real nodes per graph.  full: all N.  mixed: graphs cycle full length / a single real node / all padding (one graph: a single
    real node when N > 1).  allpad: no real node anywhere."""
    if pad == "full" or N == 0:
        return [N] * G
    if pad == "allpad":
        return [0] * G
    if G == 1:
        return [1]
    return [(N, 1, 0)[g % 3] for g in range(G)]


def make_case(G, N, pad="full", p_pos=0.0, p_in=0.0, layout="128+32", n_fold=0, n_add=4, C=C_FUSED, seed=77, keep_fn=site_keep,
              case_seed=None):
    """A seeded case: every value f32-representable (bf16 for the QKV weight), float64 CPU tensors.  C != 192: the assembly entries'
    operands only (nf_in, add_in, real, token, pe0, dout)."""
    key = "%d %d %s %g %g %s %d %d %d" % (G, N, pad, p_pos, p_in, layout, n_fold, n_add, C)
    rs = np.random.RandomState(zlib.crc32(key.encode()) if case_seed is None else case_seed)
    rn = lambda *s: torch.from_numpy(rs.standard_normal(s)).to(F32).to(F64)                    # noqa: E731
    R, T = G * N, N + 1
    c = SimpleNamespace(G=G, N=N, T=T, R=R, C=C, W2=W2_FUSED, pad=pad, p_pos=p_pos, p_in=p_in, layout=layout, n_fold=n_fold, n_add=n_add,
                        seed=seed, salts=SALTS, slope2=float(np.float32(0.2)), slope4=float(np.float32(0.1)), keep_fn=keep_fn)
    lens = lengths_of(G, N, pad)
    c.lengths = lens
    real = torch.zeros(G, N, dtype=F64)
    for g, n in enumerate(lens):
        real[g, :n] = 1.0
    c.real = real.reshape(R)
    c.claims = set()
    if float(c.real.sum()) < R:
        c.claims.add("padded")
    fused = C == C_FUSED
    if fused:
        names = [("poi", 0)] + [("part%d" % f, 0) for f in range(n_fold)] + [("time", 0)] * (len(LAYOUTS[layout]) - 1) + [("cat", 1)]
        names += [(n, 2) for n in ADD_NAMES[n_add]]
        widths = dict(cat=C - c.W2)
        widths["poi"], coffs = LAYOUTS[layout][0][0], dict(poi=LAYOUTS[layout][0][1], cat=c.W2)
        if len(LAYOUTS[layout]) > 1:
            widths["time"], coffs["time"] = LAYOUTS[layout][1]
        sprinkle = R >= 4 and pad != "allpad"
        if sprinkle:
            c.claims.add("negatives")
        jobs, first2 = [], True
        for name, slot in names:
            fold = name.startswith("part")
            W = widths["poi"] if fold else widths.get(name, C)
            rows = TABLE_ROWS["poi" if fold else name]
            j = SimpleNamespace(name=name, slot=slot, width=W, coff=0 if fold else coffs.get(name, 0), skip=SKIP.get(name, -1),
                                accum=2 if fold else (0 if slot < 2 or first2 else 1), table=rn(rows, W), fold=fold)
            if slot == 2:
                first2 = False
            if fold:
                j.idx = jobs[0].idx
            else:
                idx = torch.from_numpy(rs.randint(0, rows, size=R)).to(torch.int64)
                if name == "pos":                                                      # (:348-351: rows 1..n of the real nodes)
                    idx = (torch.arange(N).repeat(G) + 1).to(torch.int64)
                if sprinkle:
                    idx[torch.from_numpy(rs.rand(R) < 0.2)] = -1
                    real_rows = torch.nonzero(c.real > 0).reshape(-1)
                    if len(real_rows) >= 2:
                        idx[real_rows[rs.randint(len(real_rows))]] = -1                # a negative index on a REAL node
                        if j.skip >= 0:
                            others = real_rows[idx[real_rows] >= 0]
                            if len(others):
                                idx[others[rs.randint(len(others))]] = j.skip              # ... and the padding row on another
                idx[c.real == 0] = -1                                                  # padding: every index -1
                j.idx = idx
            jobs.append(j)
        c.jobs = jobs
        c.pos_job = [k for k, j in enumerate(jobs) if j.name == "pos"][0]
        c.w2, c.b2 = rn(c.W2, c.W2) / np.sqrt(c.W2), 0.5 * rn(c.W2)
        c.w4, c.b4 = rn(C, C) / np.sqrt(C), 0.5 * rn(C)
        if "padded" in c.claims:
            # output columns of nf that are EXACTLY 0 on a padded row (x4 = [leaky(b2) | 0] there): no weight on f2, no bias
            c.zero_cols = [3, 17, 100, 191]
            c.w4[c.zero_cols, :c.W2] = 0.0
            c.b4[c.zero_cols] = 0.0
        c.w2, c.b2, c.w4, c.b4 = f32r(c.w2), f32r(c.b2), f32r(c.w4), f32r(c.b4)
        c.pe0 = jobs[c.pos_job].table[0].clone()
    else:
        c.jobs, c.pe0 = [], rn(C)
    c.token = rn(C)
    c.nf_in, c.add_in = rn(R, C), rn(R, C)
    if C in (192, 256):
        c.wq = (rn(3 * C, C) / np.sqrt(C)).to(BF).to(F64)
        c.bq = (0.5 * rn(3 * C)).to(BF).to(F64)
    c.dout = rn(G, T, C)
    draw_masks(c)
    return c


def draw_masks(c, salts=None, in_rows_gn=False):
    """keep_nf [R, C] rows g N + n, keep_tok [G, C] rows g, keep_in [G T, C] rows g T + t; ik_*: the kernels' f32 1 / keep."""
    s = salts or c.salts
    k = lambda salt, rows, p: torch.from_numpy(np.asarray(c.keep_fn(c.seed, salt, rows, c.C, p))).to(F64)      # noqa: E731
    c.keep_nf, c.keep_tok = k(s[0], c.R, c.p_pos), k(s[1], c.G, c.p_pos)
    c.keep_in = k(s[2], c.G * c.T, c.p_in)
    if in_rows_gn:                                                 # (a mutant's numbering: node row (g, n) takes row g N + n)
        w = c.keep_in.reshape(c.G, c.T, c.C).clone()
        w[:, 1:] = c.keep_in[:c.R].reshape(c.G, c.N, c.C)
        c.keep_in = w.reshape(c.G * c.T, c.C)
    c.ik_pos, c.ik_in = inv_keep_of(c.p_pos), inv_keep_of(c.p_in)


# ------------------------------------------------------------------------------------------------ the stages, float64
def gather(jobs, R, widths, dtype=F64, drop_fold=False):
    """The job list -> {slot: [R, widths[slot]]}, {slot: bool [widths[slot]] covered columns}.  A copy writes its columns, accum = 1
    adds to them, accum = 2 is a summand of the last job in front of it that is not folded, at that job's index; a negative index
    reads zeros.  dtype float32: the additions in job order, as the kernels make them (bit-exact yardstick)."""
    bufs = {s: torch.zeros(R, w, dtype=dtype) for s, w in widths.items()}
    cover = {s: torch.zeros(w, dtype=torch.bool) for s, w in widths.items()}
    k = 0
    while k < len(jobs):
        j = jobs[k]
        rows = lambda t, idx: torch.where((idx >= 0)[:, None], t.to(dtype)[idx.clamp(min=0)], torch.zeros((), dtype=dtype))   # noqa: E731
        v = rows(j.table, j.idx)
        k += 1
        while k < len(jobs) and jobs[k].accum == 2:
            if not (drop_fold and (k + 1 == len(jobs) or jobs[k + 1].accum != 2)):
                v = v + rows(jobs[k].table, j.idx)
            k += 1
        dst = bufs[j.slot][:, j.coff:j.coff + j.width]
        dst.copy_(dst + v if j.accum == 1 else v)
        cover[j.slot][j.coff:j.coff + j.width] = True
    return bufs, cover


def chain_widths(c):
    return {0: c.W2, 1: c.C, 2: c.C}


def linear_bound(a, w, b, K):
    """(K + 2) 2^-24 (|a| |w|^T + |b|): a [R, K], w [M, K] (F.linear layout), b [M] or None."""
    s = a.abs() @ w.abs().t()
    return (K + 2) * U * (s + (b.abs() if b is not None else 0.0))


def fuse2(c, pt):
    return leaky(pt @ c.w2.t() + c.b2, c.slope2)


def fuse4(c, x4):
    return leaky(x4 @ c.w4.t() + c.b4, c.slope4)


def scale_of(c):
    """[G, T, C]: keep_pos / (1 - p_pos) * keep_in / (1 - p_in) with the site masks at their numberings."""
    pos = torch.cat((c.keep_tok.reshape(c.G, 1, c.C), c.keep_nf.reshape(c.G, c.N, c.C)), 1)
    return pos * c.ik_pos * c.keep_in.reshape(c.G, c.T, c.C) * c.ik_in


def assemble(c, nf, add):
    v = torch.cat(((c.token + c.pe0).expand(c.G, 1, c.C), nf.reshape(c.G, c.N, c.C) * c.real.reshape(c.G, c.N, 1) + add.reshape(c.G, c.N, c.C)), 1)
    return v * scale_of(c)


def qkv_of(c, rows16):
    return rows16.reshape(-1, c.C) @ c.wq.t() + c.bq


def forward(c):
    bufs, _ = gather(c.jobs, c.R, chain_widths(c))
    o = SimpleNamespace(pt=bufs[0], add=bufs[2])
    o.f2 = fuse2(c, o.pt)
    o.x4 = torch.cat((o.f2, bufs[1][:, c.W2:]), 1)
    o.nf = fuse4(c, o.x4)
    o.out = assemble(c, o.nf, o.add)
    return o


def scatter(jobs, bufs, init=0.0, extra_row0=None, extra_job=0, no_grad=(), dtype=F64, skip_padding=True, extra_row=0):
    """d_table_t[idx_t[r]] += bufs[slot_t][r, coff_t : coff_t + W_t] over the jobs that are not folded; -> (list of [rows, W] or None
    for `no_grad` jobs, list of addend counts per table element, list of sum |addends|)."""
    out, cnt, mag = [], [], []
    live = [j for j in jobs if j.accum != 2]
    for k, j in enumerate(live):
        if k in no_grad:
            out.append(None), cnt.append(None), mag.append(None)
            continue
        g = bufs[j.slot][:, j.coff:j.coff + j.width].to(F64)
        ok = (j.idx >= 0) & ((j.idx != j.skip) | (not skip_padding))
        d = torch.zeros(j.table.shape, dtype=F64)
        n = torch.zeros(j.table.shape[0], dtype=F64)
        m = torch.zeros(j.table.shape, dtype=F64)
        d.index_add_(0, j.idx[ok], g[ok])
        m.index_add_(0, j.idx[ok], g[ok].abs())
        n.index_add_(0, j.idx[ok], torch.ones(int(ok.sum()), dtype=F64))
        if extra_row0 is not None and k == extra_job:
            d[extra_row] += extra_row0
            m[extra_row] += extra_row0.abs()
            n[extra_row] += 1
        out.append(d + init), cnt.append(n[:, None].expand_as(d)), mag.append(m + abs(init))
    return out, cnt, mag


def backward(c, fwd, dout=None):
    """Every gradient of sum(out * dout): the stages of the module's docstring, plus the weight gradients (the kernels under test do
    not produce them; the autograd comparison covers them all the same)."""
    dout = c.dout if dout is None else dout
    d = dout * scale_of(c)
    b = SimpleNamespace(d_token=d[:, 0].sum(0), d_add=d[:, 1:].reshape(c.R, c.C))
    b.d_nf = b.d_add * c.real[:, None]
    g4 = b.d_nf * leaky_grad(fwd.nf, c.slope4)
    b.dx4 = g4 @ c.w4
    b.dw4, b.db4 = g4.t() @ fwd.x4, g4.sum(0)
    g2 = b.dx4[:, :c.W2] * leaky_grad(fwd.f2, c.slope2)
    b.d_pt = g2 @ c.w2
    b.dw2, b.db2 = g2.t() @ fwd.pt, g2.sum(0)
    b.d_tables, _, _ = scatter(c.jobs, {0: b.d_pt, 1: b.dx4, 2: b.d_add}, extra_row0=b.d_token, extra_job=live_index(c, c.pos_job))
    return b


def live_index(c, k):
    """Index of job k among the jobs that are not folded (a backward call's job list)."""
    return sum(1 for j in c.jobs[:k] if j.accum != 2)


# ------------------------------------------------------------------------------------------------ exact stages in f32
def assemble_f32(c, nf, add, no_keep=()):
    """The documented order in f32: v = nf * real + add (real in {0, 1}: the product is exact, so a fused multiply-add rounds the
    same way), scale = keep_pos, scale *= keep_in, out = v * scale.  nf / add: float32 tensors."""
    f = lambda t: t.to(F32)                                                                  # noqa: E731
    v = torch.cat(((f(c.token) + f(c.pe0)).expand(c.G, 1, c.C),
                   nf.reshape(c.G, c.N, c.C) * f(c.real).reshape(c.G, c.N, 1) + add.reshape(c.G, c.N, c.C)), 1)
    return v * scale_f32(c, no_keep)


def scale_f32(c, no_keep=()):
    one = torch.ones((), dtype=F32)
    ik_pos = one if "pos" in no_keep else torch.tensor(c.ik_pos, dtype=F32)
    ik_in = one if "in" in no_keep else torch.tensor(c.ik_in, dtype=F32)
    pos = torch.cat((c.keep_tok.reshape(c.G, 1, c.C), c.keep_nf.reshape(c.G, c.N, c.C)), 1).to(F32)
    scale = pos * ik_pos if c.p_pos else torch.ones_like(pos)
    if c.p_in:
        scale = scale * (c.keep_in.reshape(c.G, c.T, c.C).to(F32) * ik_in)
    return scale


def d_of_f32(c, dout=None):
    """d = dout * scale in f32 -> (token rows [G, C], node rows [R, C])."""
    d = (c.dout if dout is None else dout).to(F32) * scale_f32(c)
    return d[:, 0], d[:, 1:].reshape(c.R, c.C)


# ------------------------------------------------------------------------------------------------ buffers with guards
class Buffers:
    """Output buffers with GUARD sentinel rows past R (2-D; and sentinel columns up to `ld`) or GUARD sentinel elements past the end
    (1-D).  A "written" buffer is pre-filled with NaN, an "accumulated" one with a known value."""

    def __init__(self, device="cpu"):
        self.full, self.view, self.device = {}, {}, device

    def add(self, name, shape, dtype=F32, fill=float("nan"), ld=None):
        if len(shape) == 2:
            full = torch.full((shape[0] + GUARD, ld or shape[1]), SENT, dtype=dtype, device=self.device)
            view = full[:shape[0], :shape[1]]
        else:
            full = torch.full((shape[0] + GUARD,), SENT, dtype=dtype, device=self.device)
            view = full[:shape[0]]
        view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
        self.full[name], self.view[name] = full, view
        return view

    def guard_failures(self):
        bad = []
        for name, full in self.full.items():
            v = self.view[name]
            if not bool((full[v.shape[0]:] == SENT).all()):
                bad.append("%s: rows past R were written" % name)
            if full.dim() == 2 and full.shape[1] > v.shape[1] and not bool((full[:, v.shape[1]:] == SENT).all()):
                bad.append("%s: columns past the width were written" % name)
        return bad

    def args(self):
        """What a call is given: the view, or -- a view of no rows has no address -- the buffer behind it (N = 0: a dummy that must
        stay untouched, which the guard check then sees)."""
        return {n: v if v.numel() else self.full[n] for n, v in self.view.items()}

    def cpu(self):
        return {n: v.detach().cpu() for n, v in self.view.items()}


# ------------------------------------------------------------------------------------------------ verdicts
def _exact(fails, name, got, want, what=""):
    if got.shape != want.shape or not torch.equal(got, want):
        n = int((got != want).sum()) if got.shape == want.shape else -1
        fails.append("%s: %d elements differ from %s" % (name, n, what or "the f32 restatement"))


def _within(fails, name, got, ref, bound):
    err = (got.to(F64) - ref).abs()
    bad = ~(err <= bound)                                          # (a NaN fails)
    if bool(bad.any()):
        ratio = float((err / bound.clamp(min=1e-300))[bad].nan_to_num(nan=float("inf")).max())
        fails.append("%s: %d of %d elements past the bound, worst %.3g x" % (name, int(bad.sum()), bad.numel(), ratio))
    return float((err / bound.clamp(min=1e-300)).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0


def judge_gather(c, got, widths=None, jobs=None, uncovered_zero=True, prefix=""):
    """pt / x4's trailing columns / add (or `widths`' slots, named by slot) against the gathered rows, bit for bit; columns no table
    covers are zero (the fused launch) or still hold their NaN prefill (mobgt_embed_gather_multi on its own)."""
    fails = []
    jobs = c.jobs if jobs is None else jobs
    widths = widths or chain_widths(c)
    want, cover = gather(jobs, c.R, widths, dtype=F32)
    for slot, name in ((0, "pt"), (1, "x4"), (2, "add")):
        if slot not in widths:
            continue
        g, cv = got[prefix + name], cover[slot]
        if name == "x4" and uncovered_zero:
            g, w, cv = g[:, c.W2:], want[slot][:, c.W2:], cv[c.W2:]
        else:
            w = want[slot]
        _exact(fails, name, g[:, cv], w[:, cv], "the gathered rows")
        if bool((~cv).any()):
            rest = g[:, ~cv]
            if not bool(((rest == 0) if uncovered_zero else torch.isnan(rest)).all()):
                fails.append("%s: columns no table covers were %s" % (name, "not zero" if uncovered_zero else "written"))
    return fails


def judge_forward(c, got, report=None):
    """The fused forward's outputs (float32 / bfloat16 CPU tensors: pt, x4, add, nf, out, out16, qkv), each stage on got's upstream."""
    fails = judge_gather(c, got)
    rep = {} if report is None else report
    pt, x4, nf = got["pt"].to(F64), got["x4"].to(F64), got["nf"]
    rep["f2"] = _within(fails, "f2", got["x4"][:, :c.W2], fuse2(c, pt), linear_bound(pt, c.w2, c.b2, c.W2))
    rep["nf"] = _within(fails, "nf", nf, fuse4(c, x4), linear_bound(x4, c.w4, c.b4, c.C))
    fails += judge_assembly(c, got, nf, got["add"], rep)
    return fails


def judge_assembly(c, got, nf, add, report=None):
    """out / out16 / qkv (those present in got) from the f32 operands nf, add."""
    fails = []
    want = assemble_f32(c, nf, add).reshape(got["out"].shape)
    _exact(fails, "out", got["out"], want)
    dropped = (scale_f32(c) == 0).reshape(got["out"].shape)
    if not bool((got["out"][dropped] == 0).all()):
        fails.append("out: a dropped element is not exactly 0")
    if got.get("out16") is not None:
        _exact(fails, "out16", got["out16"], got["out"].to(BF), "round-to-nearest-even of out")
    if got.get("qkv") is not None:
        rows = got["out16"].to(F64).reshape(-1, c.C)
        ref = qkv_of(c, rows)
        r = _within(fails, "qkv", got["qkv"], ref, 2.0 ** -8 * ref.abs() + linear_bound(rows, c.wq, c.bq, c.C))
        if report is not None:
            report["qkv"] = r
    return fails


def judge_assembly_bwd(c, got, dout=None, token_init=TOKEN_INIT, report=None):
    """d_nf, d_add bit for bit; d_token = its initial value + the float64 sum of the token rows' f32 d, within (n + 2) 2^-24 sum |terms|."""
    fails = []
    d_tok, d_node = d_of_f32(c, dout)
    if c.R:
        _exact(fails, "d_add", got["d_add"], d_node)
        _exact(fails, "d_nf", got["d_nf"], d_node * c.real.to(F32)[:, None])
    terms = d_tok.to(F64)
    ref = token_init + terms.sum(0)
    n = (terms != 0).sum(0).to(F64) + 1
    r = _within(fails, "d_token", got["d_token"], ref, (n + 2) * U * (terms.abs().sum(0) + abs(token_init)))
    if report is not None:
        report["d_token"] = r
    return fails


def judge_backward(c, got, y4, y2, dout=None, report=None):
    """The fused backward's outputs (d_nf, d_add, dx4, d_pt, d_token) with the saved activations y4 [R, C], y2 [R, W2] (float64)."""
    rep = {} if report is None else report
    fails = judge_assembly_bwd(c, got, dout, report=rep)
    g4 = got["d_nf"].to(F64) * leaky_grad(y4, c.slope4)
    rep["dx4"] = _within(fails, "dx4", got["dx4"], g4 @ c.w4, linear_bound(g4, c.w4.t(), None, c.C))
    g2 = got["dx4"].to(F64)[:, :c.W2] * leaky_grad(y2, c.slope2)
    rep["d_pt"] = _within(fails, "d_pt", got["d_pt"], g2 @ c.w2, linear_bound(g2, c.w2.t(), None, c.W2))
    return fails


def judge_scatter(jobs, bufs, got_tables, extra_row0=None, extra_job=0, no_grad=(), init=TABLE_INIT):
    """got_tables[k]: the k-th live job's gradient table (float32) after the scatter into a table pre-filled with `init`; a `no_grad`
    job's table must still hold its sentinel fill (the caller's check)."""
    fails = []
    ref, cnt, mag = scatter(jobs, bufs, init=init, extra_row0=extra_row0, extra_job=extra_job, no_grad=no_grad)
    for k, r in enumerate(ref):
        if r is not None:
            _within(fails, "d_table[%d]" % k, got_tables[k], r, (cnt[k] + 2) * U * mag[k])
    return fails


# ------------------------------------------------------------------------------------------------ emulation and mutants
MUTANTS = ("no_keep_pos", "no_keep_in", "salts_swapped", "in_rows_gn", "real_not_applied", "leaky_wrong_side", "w2_transposed",
           "w4_transposed", "w4_transposed_bwd", "w2_transposed_bwd", "kstep_f2", "kstep_nf", "kstep_dx4", "kstep_dpt", "kstep_qkv",
           "d_token_overwritten", "fold_dropped", "extra_row0_row1", "padding_row_not_skipped", "row_past_R")


def _kstep(a, w, step=1):
    """a [R, K] w^T with one k-step of 16 left out."""
    keep = torch.ones(a.shape[1], dtype=torch.bool)
    keep[16 * step:16 * step + 16] = False
    return a[:, keep] @ w[:, keep].t()


def emulate_forward(c, mut=None):
    """-> Buffers holding what the fused forward launch leaves (mut: a deliberately wrong one)."""
    b = Buffers()
    R, C, W2 = c.R, c.C, c.W2
    bufs, _ = gather(c.jobs, R, chain_widths(c), dtype=F32, drop_fold=mut == "fold_dropped")
    pt = b.add("pt", (R, W2), fill=bufs[0])
    pre2 = (_kstep(pt.to(F64), c.w2) if mut == "kstep_f2" else pt.to(F64) @ (c.w2 if mut == "w2_transposed" else c.w2.t())) + c.b2
    x4 = b.add("x4", (R, C), fill=torch.cat((leaky(pre2, c.slope2).to(F32), bufs[1][:, W2:]), 1))
    add = b.add("add", (R, C), fill=bufs[2])
    pre4 = (_kstep(x4.to(F64), c.w4) if mut == "kstep_nf" else x4.to(F64) @ (c.w4 if mut == "w4_transposed" else c.w4.t())) + c.b4
    nf = b.add("nf", (R, C), fill=leaky(pre4, c.slope4).to(F32))
    m = c
    if mut in ("salts_swapped", "in_rows_gn"):
        m = SimpleNamespace(**vars(c))
        draw_masks(m, (c.salts[1], c.salts[0], c.salts[2]) if mut == "salts_swapped" else None, in_rows_gn=mut == "in_rows_gn")
    out = b.add("out", (c.G * c.T, C), fill=assemble_f32(m, nf, add, no_keep={"no_keep_pos": ("pos",), "no_keep_in": ("in",)}.get(mut, ())).reshape(-1, C))
    o16 = b.add("out16", (c.G * c.T, C), BF, fill=out.to(BF))
    rows = o16.to(F64)
    q = (_kstep(rows, c.wq, 5) if mut == "kstep_qkv" else rows @ c.wq.t()) + c.bq
    b.add("qkv", (c.G * c.T, 3 * C), BF, fill=q.to(BF))
    if mut == "row_past_R":
        b.full["nf"][R] = b.full["nf"][max(R - 1, 0)]
    return b


def emulate_backward(c, y4, y2, mut=None):
    b = Buffers()
    R, C, W2 = c.R, c.C, c.W2
    d_tok, d_node = d_of_f32(c)
    b.add("d_add", (R, C), fill=d_node)
    d_nf = b.add("d_nf", (R, C), fill=d_node if mut == "real_not_applied" else d_node * c.real.to(F32)[:, None])
    lg = (lambda y, s: torch.where(y > 0, torch.full_like(y, s), torch.ones_like(y))) if mut == "leaky_wrong_side" else leaky_grad
    g4 = d_nf.to(F64) * lg(y4, c.slope4)
    v = _kstep(g4, c.w4.t()) if mut == "kstep_dx4" else g4 @ (c.w4.t() if mut == "w4_transposed_bwd" else c.w4)
    dx4 = b.add("dx4", (R, C), fill=v.to(F32))
    g2 = dx4.to(F64)[:, :W2] * lg(y2, c.slope2)
    v = _kstep(g2, c.w2.t()) if mut == "kstep_dpt" else g2 @ (c.w2.t() if mut == "w2_transposed_bwd" else c.w2)
    b.add("d_pt", (R, W2), fill=v.to(F32))
    tok = d_tok.to(F64).sum(0) + (0.0 if mut == "d_token_overwritten" else TOKEN_INIT)
    b.add("d_token", (C,), fill=tok.to(F32))
    if mut == "row_past_R":
        b.full["dx4"][R] = b.full["dx4"][max(R - 1, 0)]
    return b


def emulate_scatter(c, bufs, extra_row0, mut=None, no_grad=()):
    """-> list of float32 tables (None for no_grad jobs)."""
    out, _, _ = scatter(c.jobs, bufs, init=TABLE_INIT, extra_row0=extra_row0, extra_job=live_index(c, c.pos_job), no_grad=no_grad,
                        skip_padding=mut != "padding_row_not_skipped", extra_row=1 if mut == "extra_row0_row1" else 0)
    return [t.to(F32) if t is not None else None for t in out]


def saved_for_backward(c):
    """y4 = nf, y2 = f2 of the float64 forward, rounded to f32, with exact zeros planted on REAL nodes (first real row: columns 0, 5,
    64, 159): leaky'(0) is the slope, and only a real node's d_nf is nonzero to show it."""
    f = forward(c)
    y4, y2 = f32r(f.nf), f32r(f.f2)
    real_rows = torch.nonzero(c.real > 0).reshape(-1)
    if len(real_rows):
        for col in (0, 5, 64, 159):
            y4[real_rows[0], col] = 0.0
            y2[real_rows[0], col] = 0.0
    return y4, y2


# ------------------------------------------------------------------------------------------------ the matrix
FWD_SHAPES = ((1, 1), (1, 15), (1, 16), (2, 7), (4, 3), (3, 5), (8, 1), (5, 37), (13, 9))
BWD_SHAPES = ((1, 1), (1, 15), (1, 16), (1, 17), (12, 3), (13, 5), (25, 2))
DROPOUTS = ((0.0, 0.0), (0.1, 0.0), (0.0, 0.1), (0.1, 0.3))
PADS = ("full", "mixed", "allpad")
GATHER_ROWS = (1, 3, 4, 5, 301)
ASSEMBLE_WIDTHS = (4, 190, 192, 1024)
QKV_WIDTHS = (192, 256)
BWD_STRIDES = ((160, 192), (192, 192), (160, 200), (192, 200))        # (ld_y2, ld_dx4)


def _spec(entry, G, N, k, **kw):
    """Row k of an entry's table: the other dimensions cycle with k at coprime periods, so each value of each of them comes up."""
    lay = list(LAYOUTS)
    s = dict(entry=entry, G=G, N=N, pad=PADS[k % 3], drop=DROPOUTS[(k + 3) % 4], seed_mode=("whole", "split")[k % 2],
             layout=lay[k % 3], n_fold=(0, 1, 3)[(k // 3 + k) % 3], n_add=(4, 1, 2)[(k + k // 3) % 3], idx=("i64", "i32")[(k // 2) % 2])
    s.update(kw)
    return s


def spec_id(s):
    tail = "-".join(str(s[k]) for k in ("ld_y2", "ld_dx4", "C", "bf16") if k in s)
    return "%s-G%d-N%d-%s-p%g_%g-%s-%s-f%d-a%d-%s%s" % (s["entry"], s["G"], s["N"], s["pad"], s["drop"][0], s["drop"][1], s["seed_mode"],
                                                         s["layout"], s["n_fold"], s["n_add"], s["idx"], "-" + tail if tail else "")


def fwd_specs():
    out = [_spec("fwd_chain", G, N, k) for k, (G, N) in enumerate(FWD_SHAPES)]
    # every dropout pair on a shape with several tiles and straddling graphs, both seed modes; every layout x fold count
    out += [_spec("fwd_chain", 3, 5, 20 + k, pad="mixed", drop=d, seed_mode=m) for k, (d, m) in
            enumerate((d, m) for d in DROPOUTS for m in ("whole", "split"))]
    out += [_spec("fwd_chain", 4, 3, 40 + k, pad="mixed", layout=lay, n_fold=f, n_add=a) for k, (lay, f, a) in
            enumerate((lay, f, a) for lay in LAYOUTS for f, a in ((0, 1), (1, 2), (3, 4)))]
    out += [_spec("fwd_chain", 5, 37, 60, pad="mixed", drop=(0.1, 0.3)), _spec("fwd_chain", 13, 9, 61, pad="mixed", drop=(0.1, 0.3))]
    out += [_spec("fwd_chain", G, 0, 70 + k, pad="full", drop=(0.1, 0.3)) for k, G in enumerate((1, 17))]
    seen, uniq = set(), []
    for s in out:
        if (s["G"], s["N"]) == (1, 1) and s["pad"] == "mixed":
            s["pad"] = "full"                                      # (one node: nothing to mix)
        if spec_id(s) not in seen:
            seen.add(spec_id(s))
            uniq.append(s)
    return uniq


def bwd_specs():
    out = [_spec("bwd_chain", G, N, k, ld_y2=BWD_STRIDES[k % 4][0], ld_dx4=BWD_STRIDES[k % 4][1]) for k, (G, N) in enumerate(BWD_SHAPES)]
    out += [_spec("bwd_chain", 13, 5, 20 + k, pad="mixed", drop=d, seed_mode=m, ld_y2=BWD_STRIDES[k % 4][0], ld_dx4=BWD_STRIDES[k % 4][1])
            for k, (d, m) in enumerate((d, m) for d in DROPOUTS for m in ("whole", "split"))]
    out += [_spec("bwd_chain", 25, 2, 40 + k, pad=p, drop=(0.1, 0.3), ld_y2=a, ld_dx4=b) for k, (p, (a, b)) in
            enumerate((p, st) for p in ("mixed", "allpad") for st in BWD_STRIDES)]
    for s in out:
        if (s["G"], s["N"]) == (1, 1) and s["pad"] == "mixed":
            s["pad"] = "full"
        s["layout"], s["n_fold"], s["n_add"], s["idx"] = "128+32", 0, 4, "i64"         # (no gathers in this launch)
    return out


def assemble_specs():
    out = []
    for k, C in enumerate(ASSEMBLE_WIDTHS):
        for q, (G, N) in enumerate(((4, 3), (3, 5), (8, 1), (5, 37), (1, 0), (17, 0))):
            out.append(_spec("assemble", G, N, k + 2 * q, C=C, bf16=("bf16", "f32only")[(k + q) % 2], pad="mixed" if N else "full",
                             drop=DROPOUTS[(k + q) % 4]))
    for k, C in enumerate(QKV_WIDTHS):
        for q, (G, N) in enumerate(FWD_SHAPES + ((1, 0), (17, 0))):
            out.append(_spec("qkv", G, N, k + q, C=C, pad=("mixed" if (G, N) != (1, 1) else "full") if N else "full", drop=DROPOUTS[(k + q) % 4]))
    for s in out:
        s["layout"], s["n_fold"], s["n_add"], s["idx"] = "128+32", 0, 4, "i64"
    return out


def gather_specs():
    out = []
    for k, R in enumerate(GATHER_ROWS):
        for q, (lay, f, a) in enumerate(((lay, f, a) for lay in LAYOUTS for f, a in ((0, 1), (1, 2), (3, 4)))):
            if (k + q) % 2 == 0 or R == 301:
                out.append(_spec("gather", R, 1, k + q, layout=lay, n_fold=f, n_add=a, pad="full", drop=(0.0, 0.0), idx=("i64", "i32")[(k + q // 2) % 2]))
    return out


def spec_case(s, keep_fn=site_keep, seed=77):
    return make_case(s["G"], s["N"], s["pad"], s["drop"][0], s["drop"][1], s["layout"], s["n_fold"], s["n_add"], C=s.get("C", C_FUSED),
                     seed=seed, keep_fn=keep_fn)


_CACHE = {}


def cached_case(s, keep_fn=site_keep, seed=77):
    """One case per spec and process; it is shared and must not be changed."""
    k = (spec_id(s), seed, keep_fn)
    if k not in _CACHE:
        if len(_CACHE) > 64:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[k] = spec_case(s, keep_fn, seed)
    return _CACHE[k]
