"""The bitmask GCN kernels (csrc/maskgemm.hip), the small f32 GEMM's activation / masked / transposed forms (csrc/sgemm.hip,
csrc/sgemm_body.h) and the transposed copy of mobgt_bias_act_fwd_t (csrc/layer.hip) through every entry point of their C ABI,
against the float64 restatement of tests/maskgemm_reference.py.

Exact family: integer and dyadic operands, so every output must equal the reference BIT FOR BIT whatever the wave split or
summation order -- a dropped k-step, a part table in the wrong place, a wrong tail row or a wrongly rounded bf16 element is a
mismatch.  Rounding family: real operands, within the bound derived in maskgemm_reference's docstring; the worst error / bound per
case is printed.  Every output is a view into a larger sentinel-filled buffer whose guard rows and columns must stay untouched;
strided operands are views into wider buffers whose other columns hold 1000.  Each entry runs on inputs of its own: nothing is
chained.  tests/test_host_maskgemm_reference.py shows on the CPU that these verdicts reject the defects they are meant to reject."""
import numpy as np
import pytest
import torch

import maskgemm_abi as abi
import maskgemm_reference as mr

from matrix_helpers import BF, DEV, F32, Guarded, dev, opt, place

pytestmark = pytest.mark.gpu
SPECS = mr.matrix_specs()


def stage_mask(bits, words, min_words):
    """The bitmask on the device (int32 words); words beyond the kernels' reach (>= min_words) are all ones."""
    m = mr.pack_bits(bits, words)
    m[:, min_words:] = 0xFFFFFFFF
    return dev(m.view(np.int32))


def stage_xt(vals_t, K, ld):
    """A transposed bf16 operand [n, ld]: the values in columns < K, zeros up to roundup(K, 128), 1000 beyond."""
    n = vals_t.shape[0]
    a = np.zeros((n, ld), dtype=np.float32)
    a[:, :K] = vals_t
    a[:, mr.roundup(K, 128):] = 1000.0
    return dev(a, BF)


def seed_args(c):
    sd = torch.tensor([c["seed_dev"]], dtype=torch.int64, device=DEV) if c.get("seed_dev") else None
    return (c["p"] if c.get("drop") else 0.0), c["seed"], sd, c["salt"]


# ------------------------------------------------------------------------------------------------ one launcher per entry
def run_mask_gemm(c):
    s = c["spec"]
    M, K, N = s["M"], s["K"], s["N"]
    ldxt = mr.roundup(K, 128)
    words = ldxt // 32 + (4 if s["wide"] else 0)
    assert abi.workspace_bytes(K, N) == N * ldxt * 2
    mask = stage_mask(c["bits"], words, ldxt // 32)
    work = Guarded(N, ldxt, BF, init=float("nan"))
    if s["x_null"]:                                    # the producer's job: the operand, scaled, rounded, transposed, zero beyond K
        bits = mr.bf16_bits(mr.restate(c)["work"]["ref"])
        work.view.copy_(dev(bits.view(np.int16)).view(BF))
        x, ldx = None, 0
    else:
        x, ldx = place(c["x"])
    out = Guarded(M, N, off=4, pad=4)
    st = abi.mask_gemm(mask, words, x, ldx, opt(c["bscale"]), opt(c["rscale"]), opt(c["bias"]), out.view, out.ld, work.view, M, K, N)
    return st, lambda: dict(out=out.result(), work=work.result())


def run_l1(c):
    s = c["spec"]
    M, K = s["M"], s["K"]
    ldxt = mr.roundup(K, 128)
    words = ldxt // 32 + (4 if s["wide"] else 0)
    ld_y0t = ldxt + (8 if s["wide"] else 0)
    mask = stage_mask(c["bits"], words, ldxt // 32)
    y0t = stage_xt(c["y0"].T, K, ld_y0t)
    t, y = Guarded(M, mr.GI), Guarded(M, mr.GH)
    yt = Guarded(mr.GH, M, BF, off=2, pad=mr.roundup(M, 2) - M + 4)
    grid = mr.cdiv(M, 32)
    nz = (0, 4, 4 * (grid * 1024 + 5))[s["zero"]]
    zero = Guarded(1, nz, off=4, pad=4, gr=1, init=7.0) if nz else None
    p, seed, sd, salt = seed_args(c)
    st = abi.l1_fwd(mask, words, dev(c["rscale"]), y0t, ld_y0t, t.view, dev(c["w1"]), dev(c["b1"]), c["slope"], p, seed, sd, salt,
                    y.view, yt.view, yt.ld, zero.view if zero else None, nz, M, K)

    def collect():
        if zero:
            assert not zero.result().any(), "the zero side job left something"
        return dict(t=t.result(), y=y.result(), yt=yt.result())
    return st, collect


def run_rows_fwd(c):
    s = c["spec"]
    R, K, NO = s["R"], s["K"], s["NO"]
    ldxt = mr.roundup(K, 128)
    words = ldxt // 32 + (4 if s["wide"] else 0)
    mask = stage_mask(c["bits"], words, ldxt // 32)
    y1t = stage_xt(c["y1"].T, K, ldxt)
    u, parts = Guarded(R, mr.GH), Guarded(4 * R, NO)
    rs_rows = Guarded(1, R, off=4, pad=4) if s["rs_rows"] else None
    st = abi.rows_fwd(mask, words, dev(c["rows"]), dev(c["rscale"]), y1t, ldxt, dev(c["w2"]), opt(c["b2"]), u.view, parts.view,
                      rs_rows.view if rs_rows else None, R, K, NO)

    def collect():
        got = dict(u=u.result(), parts=parts.result().reshape(4, R, NO))
        if rs_rows:
            got["rs_rows"] = rs_rows.result().reshape(R)
        if s["family"] == "exact":                      # the consumer's sum, in the documented order, on the device
            p = parts.view.reshape(4, R, NO)
            got["sum"] = (((p[0] + p[1]) + p[2]) + p[3]).cpu().numpy()
        return got
    return st, collect


def run_rows_bwd(c):
    s = c["spec"]
    R, P, ldm = s["R"], s["P"], s["ldm"]
    if s["is_max"]:                                    # the largest R the library's own LDS function admits
        top = 128
        while abi.rows_bwd_lds_bytes(ldm, top + 128) <= mr.LDS_LIMIT:
            top += 128
        assert R == top and abi.rows_bwd_lds_bytes(ldm, R + 1) > mr.LDS_LIMIT
    ldg = mr.roundup(R, 128)
    mask_t = stage_mask(c["bits"].T, ldm, mr.cdiv(P, 32))
    gut = stage_xt(c["gu"].T, R, ldg)
    dy1 = Guarded(P, mr.GH)
    dtt = Guarded(mr.GI, P, BF, off=1, pad=2)
    st = abi.rows_bwd(mask_t, ldm, dev(c["rows"]), gut, ldg, dev(c["y1"]), c["mask_vals"], dev(c["w1"]), dev(c["bscale"]), dy1.view,
                      dtt.view, dtt.ld, R, P)
    return st, lambda: dict(dy1=dy1.result(), dtt=dtt.result())


def run_sgemm(c):
    s = c["spec"]
    M, N, K = s["M"], s["N"], s["K"]
    lda, aoff, ldb, boff = mr.sgemm_layout(s)
    a, lda_ = place(c["a"], off=aoff, pad=lda - aoff - K)
    am = place(c["a_mask"], off=aoff, pad=lda - aoff - K, fill=1.0)[0] if c["a_mask"] is not None else None
    bw = c["b"].shape[1]
    b, ldb_ = place(c["b"], off=boff, pad=ldb - boff - bw)
    assert (lda_, ldb_) == (lda, ldb)
    cdt = F32 if s["c_dtype"] == mr.F32C else BF
    C = Guarded(M, N, cdt, off=2, pad=3) if s["ct"] != "only" else None
    ct = Guarded(N, M, BF, off=1, pad=2) if s["ct"] else None
    p, seed, sd, salt = seed_args(c)
    st = abi.small_gemm_act(a, lda, am, c["mask_vals"], b, ldb, s["b_is_nk"], opt(c["bias"]), int(s["act"] > 0), c["slope"], p, seed,
                            sd, salt, C.view if C else None, C.ld if C else 0, s["c_dtype"], ct.view if ct else None,
                            ct.ld if ct else 0, opt(c["ct_scale"]), M, N, K, s["k_b"])

    def collect():
        got = {}
        if C:
            got["c"] = C.result()
        if ct:
            got["ct"] = ct.result()
        return got
    return st, collect


def run_bias_act(c):
    s = c["spec"]
    R, C = s["R"], s["C"]
    x, bias = dev(c["x"]), opt(c["bias"])
    y, y2 = Guarded(R, C), Guarded(R, C)
    y_t = Guarded(C, R, BF, off=1, pad=2) if s["y_t"] else None
    p, seed, sd, salt = seed_args(c)
    st = abi.bias_act_fwd_t(x, bias, y.view, y_t.view if y_t else None, y_t.ld if y_t else 0, R, C, c["slope"], p, seed, sd, salt)
    st2 = abi.bias_act_fwd(x, bias, y2.view, R, C, c["slope"], p, seed, sd, salt)

    def collect():
        got = dict(y=y.result())
        assert st2 == 0 and np.array_equal(got["y"].view(np.uint32), y2.result().view(np.uint32)), "y differs from mobgt_bias_act_fwd's"
        if y_t:
            got["y_t"] = y_t.result()
            assert np.array_equal(got["y_t"], mr.bf16_bits(got["y"]).T), "y_t is not bf16(y) transposed"
        return got
    return st, collect


RUN = dict(mask_gemm=run_mask_gemm, l1=run_l1, rows_fwd=run_rows_fwd, rows_bwd=run_rows_bwd, sgemm=run_sgemm, bias_act=run_bias_act)


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s["id"])
def test_entry(spec):
    c = mr.build_case(spec)
    st, collect = RUN[spec["entry"]](c)
    assert st == 0
    torch.cuda.synchronize()
    got = collect()
    ok, ratio = mr.verdict(c, got)
    if spec["family"] == "round":
        print(f"maskgemm-ratio {spec['id']} {ratio:.4f}")
    assert ok, (spec["id"], ratio)


# ------------------------------------------------------------------------------------------------ refusals: status codes only
class Refusal:
    """Small valid operands whose destinations hold the sentinel; every refused call must leave them untouched."""

    def __init__(self):
        ones = lambda *shape, dt=F32: torch.ones(*shape, dtype=dt, device=DEV)          # noqa: E731
        self.mask = torch.zeros(64, 8, dtype=torch.int32, device=DEV)
        self.rows = torch.zeros(16, dtype=torch.int64, device=DEV)
        self.f = ones(64, 64)
        self.xt = ones(64, 256, dt=BF)
        self.out, self.work = Guarded(8, 16, off=4, pad=4), Guarded(16, 128, BF)
        self.t, self.y, self.yt = Guarded(8, 16), Guarded(8, 64), Guarded(64, 8, BF, off=2, pad=2)
        self.zero = Guarded(1, 8, off=4, pad=4)
        self.u, self.parts, self.rs = Guarded(8, 64), Guarded(32, 8), Guarded(1, 8, off=4, pad=4)
        self.dy1, self.dtt = Guarded(40, 64), Guarded(16, 40, BF)
        self.c, self.ct = Guarded(8, 8), Guarded(8, 8, BF)
        self.by, self.byt = Guarded(8, 16), Guarded(16, 8, BF)
        self.outs = (self.out, self.work, self.t, self.y, self.yt, self.zero, self.u, self.parts, self.rs, self.dy1, self.dtt, self.c,
                     self.ct, self.by, self.byt)
        ldm = 2
        self.max_R = 128
        while abi.rows_bwd_lds_bytes(ldm, self.max_R + 128) <= mr.LDS_LIMIT:
            self.max_R += 128

    def mg(self, **kw):
        a = dict(mask=self.mask, words=4, x=self.f, ldx=64, bscale=self.f, rscale=self.f, bias=self.f, out=self.out.view,
                 ld_out=self.out.ld, work=self.work.view, M=8, K=40, N=16)
        a.update(kw)
        return abi.mask_gemm(a["mask"], a["words"], a["x"], a["ldx"], a["bscale"], a["rscale"], a["bias"], a["out"], a["ld_out"],
                             a["work"], a["M"], a["K"], a["N"])

    def l1(self, **kw):
        a = dict(mask=self.mask, words=4, rscale=self.f, y0t=self.xt, ld_y0t=256, t=self.t.view, w1=self.f, b1=self.f, p=0.0, y=self.y.view,
                 yt=self.yt.view, ld_yt=self.yt.ld, zero=self.zero.view, nz=8, M=8, K=40)
        a.update(kw)
        return abi.l1_fwd(a["mask"], a["words"], a["rscale"], a["y0t"], a["ld_y0t"], a["t"], a["w1"], a["b1"], 0.5, a["p"], 1, None, 2,
                          a["y"], a["yt"], a["ld_yt"], a["zero"], a["nz"], a["M"], a["K"])

    def rf(self, **kw):
        a = dict(mask=self.mask, words=4, rows=self.rows, rscale=self.f, y1t=self.xt, ld_y1t=128, w2=self.f, b2=self.f, u=self.u.view,
                 parts=self.parts.view, rs=self.rs.view, R=8, K=40, NO=8)
        a.update(kw)
        return abi.rows_fwd(a["mask"], a["words"], a["rows"], a["rscale"], a["y1t"], a["ld_y1t"], a["w2"], a["b2"], a["u"], a["parts"],
                            a["rs"], a["R"], a["K"], a["NO"])

    def rb(self, **kw):
        a = dict(mask_t=self.mask, words=2, rows=self.rows, gut=self.xt, ld_gut=128, y1=self.f, w1=self.f, bscale=self.f,
                 dy1=self.dy1.view, dtt=self.dtt.view, ld_dtt=self.dtt.ld, R=8, P=40)
        a.update(kw)
        return abi.rows_bwd(a["mask_t"], a["words"], a["rows"], a["gut"], a["ld_gut"], a["y1"], (2, 1, 0), a["w1"], a["bscale"], a["dy1"],
                            a["dtt"], a["ld_dtt"], a["R"], a["P"])

    def sg(self, **kw):
        a = dict(a=self.f, lda=64, am=None, b=self.f, ldb=64, nk=0, c=self.c.view, ldc=self.c.ld, cdt=abi.F32, ct=self.ct.view,
                 ld_t=self.ct.ld, M=8, N=8, K=16, k_b=0)
        a.update(kw)
        return abi.small_gemm_act(a["a"], a["lda"], a["am"], (2, 1, 0), a["b"], a["ldb"], a["nk"], None, 1, 0.5, 0.0, 1, None, 2, a["c"],
                                  a["ldc"], a["cdt"], a["ct"], a["ld_t"], None, a["M"], a["N"], a["K"], a["k_b"])

    def ba(self, ld_t=None, R=8, C=16):
        return abi.bias_act_fwd_t(self.f, self.f, self.by.view, self.byt.view, self.byt.ld if ld_t is None else ld_t, R, C, 0.5, 0.0, 1,
                                  None, 2)


def _p(t, off):
    return t.data_ptr() + off


BAD, ALIGN = abi.EBADDIM, abi.EALIGN
REFUSALS = {
    # mobgt_mask_gemm
    "mg-N0": (lambda r: r.mg(N=0), BAD), "mg-N8": (lambda r: r.mg(N=8), BAD), "mg-N80": (lambda r: r.mg(N=80), BAD),
    "mg-ld_out-odd": (lambda r: r.mg(ld_out=25), BAD), "mg-words-5": (lambda r: r.mg(words=5), BAD),
    "mg-words-below-K": (lambda r: r.mg(words=1), BAD), "mg-words-below-roundup": (lambda r: r.mg(words=4, K=200), BAD),
    "mg-work-null": (lambda r: r.mg(work=None), BAD), "mg-out-off-4": (lambda r: r.mg(out=_p(r.out.view, 4)), ALIGN),
    "mg-bias-off-4": (lambda r: r.mg(bias=_p(r.f, 4)), ALIGN), "mg-work-off-2": (lambda r: r.mg(work=_p(r.work.view, 2)), ALIGN),
    "mg-M0": (lambda r: r.mg(M=0), 0), "mg-K0": (lambda r: r.mg(K=0), 0),
    # mobgt_mask_gemm_l1_fwd
    "l1-ld_yt-below-M": (lambda r: r.l1(ld_yt=6), BAD), "l1-ld_yt-odd": (lambda r: r.l1(ld_yt=13), BAD),
    "l1-zero_floats-6": (lambda r: r.l1(nz=6), BAD), "l1-words-5": (lambda r: r.l1(words=5), BAD),
    "l1-words-small": (lambda r: r.l1(words=4, K=200), BAD), "l1-ld_y0t-small": (lambda r: r.l1(ld_y0t=64), BAD),
    **{f"l1-{k}-null": (lambda r, k=k: r.l1(**{k: None}), BAD) for k in ("mask", "rscale", "y0t", "t", "w1", "b1", "y", "yt")},
    "l1-y0t-off-2": (lambda r: r.l1(y0t=_p(r.xt, 2)), ALIGN), "l1-mask-off-4": (lambda r: r.l1(mask=_p(r.mask, 4)), ALIGN),
    "l1-y-off-4": (lambda r: r.l1(y=_p(r.y.view, 4)), ALIGN), "l1-yt-off-2": (lambda r: r.l1(yt=_p(r.yt.view, 2)), ALIGN),
    "l1-zero-off-4": (lambda r: r.l1(zero=_p(r.zero.view, 4)), ALIGN),
    "l1-M0": (lambda r: r.l1(M=0), 0), "l1-K0": (lambda r: r.l1(K=0), 0),
    # mobgt_mask_rows_fwd
    "rf-NO0": (lambda r: r.rf(NO=0), BAD), "rf-NO6": (lambda r: r.rf(NO=6), BAD), "rf-NO196": (lambda r: r.rf(NO=196), BAD),
    "rf-ld_y1t-256": (lambda r: r.rf(ld_y1t=256), BAD), "rf-words-5": (lambda r: r.rf(words=5), BAD),
    **{f"rf-{k}-null": (lambda r, k=k: r.rf(**{k: None}), BAD) for k in ("mask", "rows", "rscale", "y1t", "w2", "u", "parts")},
    "rf-w2-off-4": (lambda r: r.rf(w2=_p(r.f, 4)), ALIGN), "rf-y1t-off-2": (lambda r: r.rf(y1t=_p(r.xt, 2)), ALIGN),
    "rf-mask-off-4": (lambda r: r.rf(mask=_p(r.mask, 4)), ALIGN),
    "rf-R0": (lambda r: r.rf(R=0), 0), "rf-K0": (lambda r: r.rf(K=0), 0),
    # mobgt_mask_rows_bwd
    "rb-ld_gut-256": (lambda r: r.rb(ld_gut=256), BAD), "rb-ld_dtt-below-P": (lambda r: r.rb(ld_dtt=39), BAD),
    "rb-words-below-P": (lambda r: r.rb(words=1), BAD),
    **{f"rb-{k}-null": (lambda r, k=k: r.rb(**{k: None}), BAD) for k in ("mask_t", "rows", "gut", "y1", "w1", "bscale", "dy1", "dtt")},
    "rb-gut-off-8": (lambda r: r.rb(gut=_p(r.xt, 8)), ALIGN), "rb-y1-off-4": (lambda r: r.rb(y1=_p(r.f, 4)), ALIGN),
    "rb-dy1-off-4": (lambda r: r.rb(dy1=_p(r.dy1.view, 4)), ALIGN),
    "rb-R-one-step-past-the-LDS-limit": (lambda r: r.rb(R=r.max_R + 1, ld_gut=r.max_R + 128), BAD),
    "rb-R0": (lambda r: r.rb(R=0), 0), "rb-P0": (lambda r: r.rb(P=0), 0),
    # mobgt_small_gemm_f32_act (its header admits M, N, K >= 1 only: a zero size is a refusal, not an empty launch)
    "sg-ld_t-below-M": (lambda r: r.sg(ld_t=7), BAD), "sg-c-and-ct-null": (lambda r: r.sg(c=None, ct=None), BAD),
    "sg-nk-with-k_b": (lambda r: r.sg(nk=1, k_b=8), BAD), "sg-k_b-above-K": (lambda r: r.sg(k_b=17), BAD),
    "sg-c_dtype-99": (lambda r: r.sg(cdt=99), abi.EDTYPE), "sg-a-off-2": (lambda r: r.sg(a=_p(r.f, 2)), ALIGN),
    "sg-a_mask-off-2": (lambda r: r.sg(am=_p(r.f, 2)), ALIGN), "sg-c-off-2": (lambda r: r.sg(c=_p(r.c.view, 2)), ALIGN),
    "sg-M0": (lambda r: r.sg(M=0), BAD), "sg-N0": (lambda r: r.sg(N=0), BAD), "sg-K0": (lambda r: r.sg(K=0), BAD),
    # mobgt_bias_act_fwd_t
    "ba-ld_t-below-R": (lambda r: r.ba(ld_t=7), BAD), "ba-C6": (lambda r: r.ba(C=6), BAD), "ba-C0": (lambda r: r.ba(C=0), BAD),
    "ba-R0": (lambda r: r.ba(R=0), 0),
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
        assert o.untouched()
