"""The split-K weight-gradient kernels (csrc/wgrad.hip, csrc/wgrad_body.h, csrc/wgradbig.hip, and the hop table's backward they
carry) through every entry point of their C ABI, against the float64 restatement of tests/wgrad_reference.py.

Exact family: integer operands, so every result must equal the reference BIT FOR BIT whatever the split count, wave count or
atomic order -- a dropped, doubled or misplaced row, column, split, mask or bias is a mismatch.  Rounding family: real operands
with bf16 ties, within the derived bound (R + 64) 2^-24 |g^|^T |x^| per element (wgrad_reference.bound); the worst error / bound
per case is printed.  Every output is a view into a larger sentinel-filled buffer whose guard rows and columns must stay untouched.
tests/test_host_wgrad_reference.py shows on the CPU that these verdicts reject the defects they are meant to reject."""
import pytest
import torch

import wgrad_abi as abi
import wgrad_reference as wr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -12345.0
SPECS = wr.matrix_specs()
BF, F32 = torch.bfloat16, torch.float32


class Guarded:
    """A [rows, cols] f32 destination inside a sentinel-filled buffer: `gr` guard rows above and below, `off` guard columns to the
    left and `pad` to the right (1-D: one row)."""

    def __init__(self, init, off=2, pad=2, gr=2, ld=None):
        self.one_d = init.dim() == 1
        init = init.reshape(1, -1) if self.one_d else init
        rows, cols = init.shape
        self.ld = ld or cols + off + pad
        self.box = (gr, gr + rows, off, off + cols)
        self.big = torch.full((rows + 2 * gr, self.ld), SENT, dtype=F32, device=DEV)
        self.view = self.big[gr:gr + rows, off:off + cols]
        self.view.copy_(init)

    def result(self):
        """The destination on the host; asserts that nothing outside it was written."""
        big = self.big.cpu()
        r0, r1, c0, c1 = self.box
        out = big[r0:r1, c0:c1].clone()
        big[r0:r1, c0:c1] = SENT
        assert bool((big == SENT).all()), "a guard row or column was written"
        return out.reshape(-1) if self.one_d else out


def place(t, dtype, view, fill=1000.0, off=2, pad=4):
    """(device tensor, leading dimension) of operand t [R, C]: contiguous, or (view) columns off .. off + C of a wider buffer whose
    other columns hold `fill` -- a kernel that reads them is wrong by thousands."""
    R, C = t.shape
    if not view:
        return t.to(DEV, dtype).contiguous(), C
    wide = torch.full((R, C + off + pad), fill, dtype=dtype, device=DEV)
    v = wide[:, off:off + C]
    v.copy_(t)
    return v, C + off + pad


def stage(p):
    """Device buffers of one built problem."""
    gdt, xdt = (F32 if p["form"] == "f32" else BF), (BF if p["form"] == "bf16" else F32)
    s = dict(R=p["R"], M=p["M"], N=p["N"], f32=int(p["form"] == "f32"), mask_vals=p["mask_vals"], db_of_x=p["db"] == "x")
    s["g"], s["ldg"] = place(p["g"], gdt, p["view"])
    s["x"], s["ldx"] = place(p["x"], xdt, p["view"])
    s["gmask"] = place(p["gmask"], F32, p["view"], fill=1.0)[0] if p["gmask"] is not None else None
    s["xmask"] = place(p["xmask"], F32, p["view"], fill=1.0)[0] if p["xmask"] is not None else None
    s["dw"] = Guarded(p["dw0"])
    s["db"] = Guarded(p["db0"], off=4, pad=4, gr=0) if p["db"] is not None else None
    s["gout"] = None
    if p["gm_out"]:                                   # g's layout: the same pitch and column offset as g
        off = 2 if p["view"] else 0
        s["gout"] = Guarded(torch.full((p["R"], p["M"]), SENT), off=off, pad=s["ldg"] - off - p["M"], ld=s["ldg"])
    s["bias"] = p["bias"].to(DEV) if p["bias"] is not None else None
    return s


def v(t):
    return t.view if t is not None else None


def collect(staged):
    return [dict(dw=s["dw"].result(), db=s["db"].result() if s["db"] else None, gm=s["gout"].result() if s["gout"] else None)
            for s in staged]


def cols(staged, key, f=lambda t: t):
    return [f(s[key]) for s in staged]


def launch_wgrad(spec, st, hop=None, tail=None):
    """The spec's entry point over the staged problems -> status."""
    e, s0 = spec["entry"], st[0]
    dt = abi.F32 if s0["f32"] else abi.BF16
    if e == "plain":
        return abi.wgrad(s0["g"], s0["ldg"], s0["x"], s0["ldx"], s0["dw"].view, s0["dw"].ld, v(s0["db"]), s0["R"], s0["M"], s0["N"], dt)
    if e == "masked":
        return abi.wgrad_masked(s0["g"], s0["ldg"], s0["x"], s0["ldx"], s0["gmask"], s0["xmask"], s0["mask_vals"], v(s0["gout"]),
                                s0["dw"].view, s0["dw"].ld, v(s0["db"]), s0["db_of_x"], s0["R"], s0["M"], s0["N"])
    if e == "bias":
        return abi.wgrad_bias(s0["g"], s0["ldg"], s0["x"], s0["ldx"], s0["bias"], s0["dw"].view, s0["dw"].ld, s0["R"], s0["M"], s0["N"], dt)
    if e == "mixed":
        return abi.wgrad_mixed(s0["g"], s0["ldg"], s0["x"], s0["ldx"], s0["dw"].view, s0["dw"].ld, v(s0["db"]), s0["R"], s0["M"], s0["N"])
    common = (cols(st, "g"), cols(st, "ldg"), cols(st, "x"), cols(st, "ldx"))
    dst = (cols(st, "dw", lambda t: t.view), cols(st, "dw", lambda t: t.ld))
    if e in ("group", "tail"):
        db = None if spec["db_null_array"] else cols(st, "db", v)
        args = common + dst + (db, s0["R"], cols(st, "M"), cols(st, "N"), dt)
        return abi.wgrad_group(*args) if e == "group" else abi.backward_tail(*args, *tail)
    args = common + (cols(st, "gmask"), cols(st, "xmask"), cols(st, "mask_vals")) + dst + \
        (cols(st, "db", v), cols(st, "db_of_x"), cols(st, "R"), cols(st, "M"), cols(st, "N"), cols(st, "f32"))
    return abi.wgrad_multi(*args) if e == "multi" else abi.wgrad_multi_hop(*args, hop)


def stage_hop(case):
    h, hs = case["hop"], case["spec"]["hop"]
    t = {k: h[k].to(DEV).contiguous() for k in ("dtab", "enc", "w")}
    t["d_enc"] = Guarded(torch.full((hs["E"] * 8,), SENT), off=4, pad=4, gr=0)
    t["d_w"] = Guarded(torch.full((hs["D"] * 64,), SENT), off=4, pad=4, gr=0)
    return t


def check_wgrad(case, got):
    ok, ratio = wr.verdict(case, got)
    spec = case["spec"]
    if spec["family"] == "round":
        print(f"wgrad-ratio {spec['entry']} {spec['id']} {ratio:.4f}")
    assert ok, (spec["id"], ratio)


@pytest.mark.parametrize("spec", [s for s in SPECS if s["entry"] not in ("big", "ops_big")], ids=lambda s: s["id"])
def test_wgrad_entry(spec):
    case = wr.build_case(spec)
    st = [stage(p) for p in case["probs"]]
    hop = tail = None
    if spec["hop"]:
        hs = spec["hop"]
        ht = stage_hop(case)
        hop = (ht["dtab"], ht["enc"], ht["w"], ht["d_enc"].view, ht["d_w"].view, hs["D"], hs["E"], hs["rt"])
    if spec["tail"]:
        t, ts = case["tail"], spec["tail"]
        a, lda = place(t["a"], BF, True, off=8, pad=8)
        b, ldb = place(t["b"], BF, True)
        c = Guarded(t["c0"], off=4, pad=4)
        tail = (a, lda, b, ldb, c.view, c.ld, ts["gM"], ts["gN"], ts["gK"])
    assert launch_wgrad(spec, st, hop, tail) == 0
    torch.cuda.synchronize()
    got = collect(st)
    check_wgrad(case, got)
    if tail:
        assert torch.equal(c.result().double(), wr.tail_reference(case))
    if hop:
        d_enc, d_w = ht["d_enc"].result(), ht["d_w"].result()
        ref_enc, ref_w = wr.hop_reference(case)
        assert torch.equal(d_enc.double(), ref_enc.reshape(-1)) and torch.equal(d_w.double(), ref_w.reshape(-1))
        # the same body launched alone: bit for bit (it uses no atomics)
        alone = stage_hop(case)
        assert abi.hop_table_bwd(alone["dtab"], alone["enc"], alone["w"], alone["d_enc"].view, alone["d_w"].view, hs["D"], hs["E"], 8,
                                 hs["rt"]) == 0
        assert torch.equal(alone["d_enc"].result(), d_enc) and torch.equal(alone["d_w"].result(), d_w)
        # ... and the weight gradients do not notice the passenger
        st2 = [stage(p) for p in case["probs"]]
        assert launch_wgrad(dict(spec, entry="multi"), st2) == 0
        for o, o2 in zip(got, collect(st2)):
            assert all(o[k] is None or torch.equal(o[k], o2[k]) for k in ("dw", "db"))


def stage_big(case):
    spec = case["spec"]
    S = wr.big_S(spec)
    jobs = []
    for q, p in enumerate(case["probs"]):
        R, M, N = p["R"], p["M"], p["N"]
        if spec["gview"]:                              # the middle third of an [R, 3M] block
            g, ldg = place(p["g"], BF, True, off=M, pad=M)
        else:
            g, ldg = place(p["g"], BF, True, off=0, pad=8)
        x, ldx = place(p["x"], BF, True, off=8, pad=8)
        on = spec["colsum"] is not None and q in spec["colsum"]
        jobs.append(dict(g=g, ldg=ldg, x=x, ldx=ldx, M=M, N=N, part=Guarded(torch.full((S * M * N,), float("nan")), off=64, pad=64, gr=0),
                         colsum=Guarded(wr.big_colsum0(case, q), off=4, pad=4, gr=0) if on else None))
    return S, jobs


@pytest.mark.parametrize("spec", [s for s in SPECS if s["entry"] == "big"], ids=lambda s: s["id"])
def test_wgrad_big(spec):
    case = wr.build_case(spec)
    R = spec["probs"][0]["R"]
    S, jobs = stage_big(case)
    tiles = sum(abi.big_tiles(j["M"], j["N"]) for j in jobs)
    assert tiles == sum(wr.big_tiles(j["M"], j["N"]) for j in jobs) and abi.big_splits(R, tiles) == wr.big_splits(R, tiles)
    colsum = None if spec["colsum"] is None else cols(jobs, "colsum", v)
    assert abi.wgrad_big(cols(jobs, "g"), cols(jobs, "ldg"), cols(jobs, "x"), cols(jobs, "ldx"), cols(jobs, "part", v), colsum,
                         cols(jobs, "M"), cols(jobs, "N"), R, S) == 0
    torch.cuda.synchronize()
    got = [dict(parts=j["part"].result().reshape(S, j["M"], j["N"]), colsum=j["colsum"].result() if j["colsum"] else None) for j in jobs]
    assert wr.big_verdict(case, got), spec["id"]


def test_ops_layer_wgrad_big():
    """ops.layer_wgrad_big (its own S, its own partial buffers and their sum) at R = 129 against the same reference."""
    from mobgt_amd import ops
    spec = next(s for s in SPECS if s["entry"] == "ops_big")
    case = wr.build_case(spec)
    ref = wr.big_reference(case)
    db = {q: Guarded(torch.zeros(p["M"]), off=4, pad=4, gr=0) for q, p in enumerate(case["probs"]) if q in spec["colsum"]}
    items = [(p["g"].to(DEV, BF), p["x"].to(DEV, BF), db[q].view if q in db else None, None) for q, p in enumerate(case["probs"])]
    assert ops.layer_wgrad_big_ok(items)
    outs = ops.layer_wgrad_big(items, 129)
    for q, (o, r) in enumerate(zip(outs, ref)):
        assert torch.equal(o.cpu().double(), r["sum"])
        if q in db:
            assert torch.equal(db[q].result().double(), r["colsum"])


# ------------------------------------------------------------------------------------------------ refusals: status codes only
class Refusal:
    """Small valid operands whose destinations hold the sentinel; every refused call must leave them untouched."""

    def __init__(self):
        self.R, self.M, self.N = 8, 6, 10
        z = lambda r, c, dt: torch.ones(r, c, dtype=dt, device=DEV)          # noqa: E731
        self.gb, self.xb, self.gf, self.xf = z(8, 8, BF), z(8, 12, BF), z(8, 8, F32), z(8, 12, F32)
        self.dw, self.db, self.dbx = (Guarded(torch.full(s, SENT)) for s in ((6, 10), (6,), (10,)))
        self.gout = Guarded(torch.full((8, 8), SENT))
        self.Gb, self.Xb = z(64, 16, BF), z(64, 16, BF)
        self.part, self.cs = Guarded(torch.full((2 * 16 * 16,), SENT), off=4, pad=4), Guarded(torch.full((16,), SENT), off=4, pad=4)
        self.hop = [torch.ones(n, device=DEV) for n in (257 * 8, 257 * 8, 64)] + [Guarded(torch.full((257 * 8,), SENT)),
                                                                                   Guarded(torch.full((64,), SENT))]
        self.c = Guarded(torch.full((8, 8), SENT), off=4, pad=4)
        self.outs = (self.dw, self.db, self.dbx, self.gout, self.part, self.cs, self.c, self.hop[3], self.hop[4])

    def plain(self, g=None, x=None, ldg=8, ldx=12, R=8, M=6, N=10, dt=None, f32=False):
        g = (self.gf if f32 else self.gb) if g is None else g
        x = (self.xf if f32 else self.xb) if x is None else x
        return abi.wgrad(g, ldg, x, ldx, self.dw.view, self.dw.ld, self.db.view, R, M, N, (abi.F32 if f32 else abi.BF16) if dt is None else dt)

    def masked(self, gmask=None, xmask=None, R=8):
        return abi.wgrad_masked(self.gf, 8, self.xf, 12, gmask, xmask, (1, 1, 1), self.gout.view, self.dw.view, self.dw.ld, self.db.view,
                                0, R, 6, 10)

    def bias(self, R=8, dt=None):
        return abi.wgrad_bias(self.gb, 8, self.xb, 12, self.xf, self.dw.view, self.dw.ld, R, 6, 10, abi.BF16 if dt is None else dt)

    def mixed(self, x=None, R=8):
        return abi.wgrad_mixed(self.gb, 8, self.xf if x is None else x, 12, self.dw.view, self.dw.ld, self.dbx.view, R, 6, 10)

    def group(self, n=None, R=8, dt=abi.BF16, tail=False):
        args = ([self.gb], [8], [self.xb], [12], [self.dw.view], [self.dw.ld], [self.db.view], R, [6], [10], dt)
        if tail:
            return abi.backward_tail(*args, self.Gb, 16, self.Xb, 16, self.c.view, self.c.ld, 8, 8, 32, n=n)
        return abi.wgrad_group(*args, n=n)

    def multi(self, n=None, f32=1, gmask=None, hop=None, R=8):
        g, x = (self.gf, self.xf) if f32 else (self.gb, self.xb)
        args = ([g], [8], [x], [12], [gmask], [None], [(1, 1, 1)], [self.dw.view], [self.dw.ld], [self.db.view], [0], [R], [6], [10], [f32])
        return abi.wgrad_multi(*args, n=n) if hop is None else abi.wgrad_multi_hop(*args, hop, n=n)

    def big(self, n=None, R=64, S=1, M=16, ldg=16, g=None):
        return abi.wgrad_big([self.Gb if g is None else g], [ldg], [self.Xb], [16], [self.part.view], [self.cs.view], [M], [16], R, S, n=n)


REFUSALS = {
    "odd-M": (lambda c: c.plain(M=5), abi.EBADDIM), "odd-N": (lambda c: c.plain(N=9), abi.EBADDIM),
    "odd-ldg": (lambda c: c.plain(ldg=9), abi.EBADDIM), "odd-ldx": (lambda c: c.plain(ldx=13, f32=True), abi.EBADDIM),
    "g-bf16-off-4-bytes": (lambda c: c.plain(g=c.gb.data_ptr() + 2), abi.EALIGN),
    "x-bf16-off-4-bytes": (lambda c: c.plain(x=c.xb.data_ptr() + 2), abi.EALIGN),
    "g-f32-off-8-bytes": (lambda c: c.plain(g=c.gf.data_ptr() + 4, f32=True), abi.EALIGN),
    "x-f32-off-8-bytes": (lambda c: c.plain(x=c.xf.data_ptr() + 4, f32=True), abi.EALIGN),
    "mixed-x-off-8-bytes": (lambda c: c.mixed(x=c.xf.data_ptr() + 4), abi.EALIGN),
    "g_mask-off-8-bytes": (lambda c: c.masked(gmask=c.gf.data_ptr() + 4), abi.EALIGN),
    "x_mask-off-8-bytes": (lambda c: c.masked(xmask=c.xf.data_ptr() + 4), abi.EALIGN),
    "group-n0": (lambda c: c.group(n=0), abi.EBADDIM), "group-n33": (lambda c: c.group(n=33), abi.EBADDIM),
    "multi-n0": (lambda c: c.multi(n=0), abi.EBADDIM), "multi-n33": (lambda c: c.multi(n=33), abi.EBADDIM),
    "tail-n0": (lambda c: c.group(n=0, tail=True), abi.EBADDIM), "tail-n33": (lambda c: c.group(n=33, tail=True), abi.EBADDIM),
    "big-n0": (lambda c: c.big(n=0), abi.EBADDIM), "big-n5": (lambda c: c.big(n=5), abi.EBADDIM),
    "plain-dtype": (lambda c: c.plain(dt=99), abi.EDTYPE), "bias-dtype": (lambda c: c.bias(dt=99), abi.EDTYPE),
    "group-dtype": (lambda c: c.group(dt=99), abi.EDTYPE), "tail-dtype": (lambda c: c.group(dt=99, tail=True), abi.EDTYPE),
    "multi-in_f32-2": (lambda c: c.multi(f32=2), abi.EDTYPE),
    "multi-mask-on-bf16": (lambda c: c.multi(f32=0, gmask=c.gf), abi.EDTYPE),
    "multi-hop-n_edge-257": (lambda c: c.multi(hop=(*c.hop[:3], c.hop[3].view, c.hop[4].view, 1, 257, 0)), abi.EBADDIM),
    "tail-R1025": (lambda c: c.group(R=1025, tail=True), abi.EBADDIM),
    "big-S-above-nchunk": (lambda c: c.big(R=64, S=2), abi.EBADDIM), "big-M-12": (lambda c: c.big(M=12), abi.EBADDIM),
    "big-ld-below-width": (lambda c: c.big(ldg=8), abi.EBADDIM), "big-g-off-16-bytes": (lambda c: c.big(g=c.Gb.data_ptr() + 8), abi.EALIGN),
    "R0-plain": (lambda c: c.plain(R=0), 0), "R0-masked": (lambda c: c.masked(R=0), 0), "R0-bias": (lambda c: c.bias(R=0), 0),
    "R0-mixed": (lambda c: c.mixed(R=0), 0), "R0-group": (lambda c: c.group(R=0), 0), "R0-tail": (lambda c: c.group(R=0, tail=True), 0),
}


@pytest.fixture(scope="module")
def refusal():
    return Refusal()


@pytest.mark.parametrize("name", list(REFUSALS), ids=list(REFUSALS))
def test_refusal(refusal, name):
    """Host-side checks: the status code comes back, no kernel runs, no destination changes."""
    fn, code = REFUSALS[name]
    assert fn(refusal) == code
    torch.cuda.synchronize()
    for o in refusal.outs:
        assert bool((o.result() == SENT).all())


# ------------------------------------------------------------------------------------------------ the Python callers' row pitch
@pytest.mark.parametrize("how", ["linear_wgrad", "linear_wgrad_bias", "linear_wgrad_masked"])
def test_ops_respect_the_destination_pitch(how):
    """A caller-supplied dw that is a column view of a wider buffer: the product lands in the view, the rest keeps its sentinel."""
    from mobgt_amd import ops
    spec = wr.S("plain" if how != "linear_wgrad_masked" else "masked",
                [wr.P(40, 6, 10, "bf16" if how == "linear_wgrad" else "f32", gmask=how == "linear_wgrad_masked",
                      out_bias=how == "linear_wgrad_bias")])
    case = wr.build_case(spec)
    p = case["probs"][0]
    dw = Guarded(p["dw0"], off=2, pad=4)
    dt = BF if p["form"] == "bf16" else F32
    g, x = p["g"].to(DEV, dt), p["x"].to(DEV, dt)
    if how == "linear_wgrad":
        ops.linear_wgrad(g, x, dw=dw.view)
    elif how == "linear_wgrad_bias":
        ops.linear_wgrad(g, x, out_bias=p["bias"].to(DEV), dw=dw.view)
    else:
        ops.linear_wgrad_masked(g, x, g_mask=p["gmask"].to(DEV), mask_vals=p["mask_vals"], dw=dw.view)
    torch.cuda.synchronize()
    assert torch.equal(dw.result().double(), wr.reference(case)[0]["dw"])
