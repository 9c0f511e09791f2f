"""The one-launch category GCN (csrc/smallgcn.hip) and the CSR adjacency products (csrc/spmm.hip) through every entry point of
their C ABI, against the float64 restatement of tests/gcn_reference.py.

Exact family: small integers and dyadic scales, so every output must equal the reference BIT FOR BIT whatever the chunking, the
wave split or the order of the atomics -- a stale staging area, a dropped chunk tail, a wrong last row or a gradient that
overwrites is a mismatch.  Rounding family: real operands, within the bound derived in gcn_reference's docstring; each saved
activation of the forward is also judged against its stage function applied to the device's own previous stage; the worst error /
bound per case is printed.  Every output is a view into a larger sentinel-filled buffer whose guards must stay untouched; strided
operands are views into wider buffers whose other columns hold 1000.  The hand-over counter must end at 2 ceil(n / 16) with its
neighbours untouched, and no workgroup may have given up at a barrier.  Forward and backward run on inputs of their own: nothing
is chained.  tests/test_host_gcn_reference.py shows on the CPU that these verdicts reject the defects they are meant to reject."""
import numpy as np
import pytest
import torch

import gcn_abi as abi
import gcn_reference as gr
from matrix_helpers import DEV, Guarded, dev, opt, place

pytestmark = pytest.mark.gpu
SPECS = gr.matrix_specs()
MARK = 7777


def filled(a):
    """A contiguous guarded destination that starts as the array a."""
    a2 = np.atleast_2d(a)
    g = Guarded(*a2.shape)
    g.view.copy_(dev(a2))
    return g


class IntGuarded:
    """`count` int32 words starting as `init` between four marked words on either side."""

    def __init__(self, count, init):
        self.buf = torch.full((count + 8,), MARK, dtype=torch.int32, device=DEV)
        self.view = self.buf[4:4 + count]
        self.view.fill_(init)

    def result(self):
        b = self.buf.cpu().numpy()
        assert (b[:4] == MARK).all() and (b[-4:] == MARK).all(), "a word beside the buffer was written"
        return b[4:-4]


def drop_args(c):
    v, n = c["v"], c["net"]
    sd = torch.tensor([v["seed_dev"]], dtype=torch.int64, device=DEV) if v["seed_dev"] else None
    return n["slope"], v["p"], n["seed"], sd, n["salt"]


def stage_fwd(c):
    n = c["net"]
    ins = dict(ax=dev(n["ax"]), a=dev(n["a"]), ws=[dev(w) for w in n["ws"]])
    outs = [Guarded(n["n"], w) for w in (gr.H1, gr.H1, gr.H2, gr.H2, gr.H3)]
    return ins, outs, IntGuarded(1, 0)


def collect_fwd(c, outs, counter):
    got = {k: o.result() for k, o in zip(("h1", "t", "h2", "t2", "out"), outs)}
    assert counter.result()[0] == 2 * gr.cdiv(c["net"]["n"], gr.RB)
    return got


def run_fwd(c):
    n = c["net"]
    ins, outs, counter = stage_fwd(c)
    st = abi.small_gcn_fwd(ins["ax"], ins["a"], ins["ws"], [o.view for o in outs], counter.view, n["n"], n["K0"], gr.WIDTHS, *drop_args(c))
    return st, lambda: collect_fwd(c, outs, counter)


def run_bwd(c):
    n, v = c["net"], c["v"]
    saved = [dev(v["saved"][k]) for k in ("h1", "t", "h2", "t2")]
    grads = [filled(n["init"][k]) for k in gr.GRADS]
    dt2, dt = Guarded(n["n"], gr.H2), Guarded(n["n"], gr.H1)
    counter = IntGuarded(1, 0)
    st = abi.small_gcn_bwd(dev(n["g"]), dev(n["ax"]), dev(n["a_t"]), dev(n["ws"][2]), dev(n["ws"][4]), saved, [g.view for g in grads],
                           dt2.view, dt.view, counter.view, n["n"], n["K0"], gr.WIDTHS, *drop_args(c))

    def collect():
        dt2.result(), dt.result()                          # scratch: only its guards matter
        assert counter.result()[0] == 2 * gr.cdiv(n["n"], gr.RB)
        return {k: g.result().reshape(n["init"][k].shape) for k, g in zip(gr.GRADS, grads)}
    return st, collect


def spmm_graph(c):
    g = c["graph"]
    return dev(g["rowptr"]), dev(g["col"]), dev(g["val"]), opt(c["rows"] if c["R"] else None)


def run_csr(c):
    s = c["spec"]
    b, ldb = place(c["b"], view=s["wide"])
    out = Guarded(c["R"], s["C"], off=4 if s["wide"] else 0, pad=8 if s["wide"] else 0)
    st = abi.spmm_csr(*spmm_graph(c), b, ldb, opt(c["bias"]), out.view, out.ld, c["R"], s["C"])
    return st, lambda: dict(out=out.result())


def run_t_rows(c):
    s = c["spec"]
    g, ldg = place(c["g"], view=s["wide"])
    db = Guarded(gr.CSR_COLS, s["C"], off=4 if s["wide"] else 0, pad=8 if s["wide"] else 0)
    db.view.copy_(dev(c["init"]))
    st = abi.spmm_csr_t_rows(*spmm_graph(c), g, ldg, db.view, db.ld, c["R"], s["C"])
    return st, lambda: dict(db=db.result())


def run_gather(c):
    s = c["spec"]
    g, ldg = place(c["g"], view=s["wide"])
    db = Guarded(c["P"], s["C"], off=4 if s["wide"] else 0, pad=8 if s["wide"] else 0)
    head, nxt = IntGuarded(c["P"], -1), IntGuarded(max(c["R"], 1), MARK)
    st = abi.spmm_csr_t_rows_gather(*spmm_graph(c), head.view, nxt.view, g, ldg, db.view, db.ld, c["P"], c["R"], s["C"])

    def collect():
        nxt.result()
        return dict(db=db.result(), head=head.result().astype(np.float32))
    return st, collect


RUN = dict(fwd=run_fwd, bwd=run_bwd, csr=run_csr, t_rows=run_t_rows, gather=run_gather)


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s["id"])
def test_entry(spec):
    c = gr.build_case(spec)
    st, collect = RUN[spec["entry"]](c)
    assert st == 0
    torch.cuda.synchronize()
    got = collect()
    if spec["entry"] in ("fwd", "bwd"):
        assert abi.small_gcn_faults() == 0
    ok, ratio = gr.verdict(c, got)
    if spec["family"] == "round":
        print(f"gcn-ratio {spec['id']} {ratio:.4f}")
    assert ok, (spec["id"], ratio)


# ------------------------------------------------------------------------------------------------ the forward with passengers
@pytest.mark.parametrize("n,K0", gr.PACK_CASES)
def test_fwd_pack(n, K0):
    """mobgt_small_gcn_fwd_pack with one pack job, the node features' index derivation and the hop table's forward as passengers:
    the network's outputs bit-identical to the launch without passengers (and to the reference), the passengers' outputs
    bit-identical to their own launches."""
    from mobgt_amd import _lib
    c = gr.build_case(next(s for s in SPECS if s["id"] == f"fwd-exact-n{n}-K{K0}-d1"))
    net = c["net"]
    g = torch.Generator().manual_seed(n)
    src = torch.randn(192, 192, generator=g).to(DEV).bfloat16()
    G, N, P = 5, 9, 700
    x = torch.randint(1, P + 1, (G, N), generator=g)
    x[torch.arange(N)[None, :] >= torch.randint(3, N + 1, (G, 1), generator=g)] = 0
    x = x.to(DEV)
    tn = torch.rand(G, N, generator=g).to(DEV)
    poi2cat = torch.randint(1, 300, (P + 1,), generator=g).to(DEV)                    # [P + 1]: indexed by the POI id itself
    indeg, outdeg = (torch.randint(0, 64, (G, N), generator=g).to(DEV) for _ in range(2))
    D, E, H = 5, 7, 8
    ew, dw = torch.randn(E, H, generator=g).to(DEV), torch.randn(D * H * H, 1, generator=g).to(DEV)

    def run(passengers):
        ins, outs, counter = stage_fwd(c)
        dst = Guarded(1, src.numel(), torch.bfloat16, init=0.0)
        idx = torch.full((8, G, N), -7, dtype=torch.int64, device=DEV)
        real, tab = Guarded(G, N), Guarded(D, E * H)
        pack = abi.pack_arrays([(src, dst.view, 0)])
        ni = [x.data_ptr(), _lib.I64, x.stride(0), x.stride(1), tn.data_ptr(), tn.stride(0), tn.stride(1), poi2cat.data_ptr(),
              indeg.data_ptr(), outdeg.data_ptr(), _lib.I64, idx.data_ptr(), real.view.data_ptr(), G, N, 1]
        hop = [ew.data_ptr(), dw.data_ptr(), tab.view.data_ptr(), D, E, H, 1]
        args = (ins["ax"], ins["a"], ins["ws"], [o.view for o in outs], counter.view, n, K0, gr.WIDTHS, *drop_args(c))
        if passengers:
            assert abi.small_gcn_fwd_pack(*args, pack=pack, node_index=ni, hop=hop) == 0
        else:
            assert abi.small_gcn_fwd(*args) == 0
            assert abi.pack_mfma_b(pack) == 0 and abi.node_index(ni) == 0 and abi.hop_table_fwd(hop) == 0
        torch.cuda.synchronize()
        got = collect_fwd(c, outs, counter)
        return got, dict(pack=dst.result(), idx=idx.cpu().numpy(), real=real.result(), tab=tab.result())
    (g1, p1), (g0, p0) = run(True), run(False)
    assert abi.small_gcn_faults() == 0
    for k in g0:
        assert np.array_equal(g1[k].view(np.uint32), g0[k].view(np.uint32)), k
    assert gr.verdict(c, g1)[0]
    for k in p0:
        assert np.array_equal(p1[k], p0[k]), k
    assert p1["pack"].any() and (p1["idx"] != -7).any() and np.abs(p1["tab"]).sum() > 0


# ------------------------------------------------------------------------------------------------ refusals: status codes only
class Refusal:
    """Small valid operands whose destinations hold the sentinel; every refused call must leave them and the counter untouched."""

    def __init__(self):
        ones = lambda *shape: torch.ones(*shape, dtype=torch.float32, device=DEV)          # noqa: E731
        self.f = ones(64, 64)
        self.i64 = torch.zeros(16, dtype=torch.int64, device=DEV)
        self.i32 = torch.zeros(64, dtype=torch.int32, device=DEV)
        self.acts = [Guarded(8, w) for w in (16, 16, 64, 64, 32)]
        self.grads = [Guarded(*s) for s in ((8, 16), (1, 16), (16, 64), (1, 64), (64, 32), (1, 32))]
        self.dt2, self.dt = Guarded(8, 64), Guarded(8, 16)
        self.counter = IntGuarded(1, 0)
        self.out, self.db = Guarded(8, 16, off=4, pad=4), Guarded(8, 16, off=4, pad=4)
        self.head, self.nxt = IntGuarded(8, -1), IntGuarded(8, MARK)
        self.outs = (*self.acts, *self.grads, self.dt2, self.dt, self.out, self.db)

    def fwd(self, n=8, K0=8, widths=gr.WIDTHS, **kw):
        a = dict(w0=self.f, w1=self.f, w2=self.f, h1=self.acts[0].view, h2=self.acts[2].view)
        a.update(kw)
        outs = [a["h1"], self.acts[1].view, a["h2"], self.acts[3].view, self.acts[4].view]
        return abi.small_gcn_fwd(self.f, self.f, [a["w0"], self.f, a["w1"], self.f, a["w2"], self.f], outs, self.counter.view, n, K0,
                                 widths, 0.5, 0.5, 1, None, 2)

    def bwd(self, n=8, K0=8, widths=gr.WIDTHS, **kw):
        a = dict(w1=self.f, w2=self.f, dt2=self.dt2.view, dt=self.dt.view)
        a.update(kw)
        return abi.small_gcn_bwd(self.f, self.f, self.f, a["w1"], a["w2"], [self.f] * 4, [g.view for g in self.grads], a["dt2"], a["dt"],
                                 self.counter.view, n, K0, widths, 0.5, 0.5, 1, None, 2)

    def csr(self, R=8, C=16, **kw):
        a = dict(b=self.f, ldb=64, bias=self.f, out=self.out.view, ld_out=self.out.ld)
        a.update(kw)
        return abi.spmm_csr(self.i64, self.i32, self.f, None, a["b"], a["ldb"], a["bias"], a["out"], a["ld_out"], R, C)

    def t_rows(self, R=8, C=16):
        return abi.spmm_csr_t_rows(self.i64, self.i32, self.f, None, self.f, 64, self.db.view, self.db.ld, R, C)

    def gather(self, P=8, R=4, C=16, **kw):
        a = dict(g=self.f, ldg=64, db=self.db.view, ld_db=self.db.ld)
        a.update(kw)
        return abi.spmm_csr_t_rows_gather(self.i64, self.i32, self.f, self.i64, self.head.view, self.nxt.view, a["g"], a["ldg"], a["db"],
                                          a["ld_db"], P, R, C)


def _p(t, off):
    return t.data_ptr() + off


BAD, ALIGN = abi.EBADDIM, abi.EALIGN
REFUSALS = {
    # mobgt_small_gcn_fwd / _bwd
    **{f"{e}-widths-{w}": (lambda r, e=e, w=w: getattr(r, e)(widths=w), BAD) for e in ("fwd", "bwd")
       for w in ((16, 64, 64), (32, 64, 32), (16, 32, 32), (0, 64, 32))},
    **{f"{e}-{k}-{v}": (lambda r, e=e, k=k, v=v: getattr(r, e)(**{k: v}), BAD) for e in ("fwd", "bwd")
       for k, v in (("n", 0), ("K0", 0), ("n", 4097), ("n", -1))},
    **{f"fwd-{k}-off-4": (lambda r, k=k: r.fwd(**{k: _p(r.f, 4)}), ALIGN) for k in ("w0", "w1", "w2")},
    "fwd-h1-off-4": (lambda r: r.fwd(h1=_p(r.acts[0].view, 4)), ALIGN), "fwd-h2-off-8": (lambda r: r.fwd(h2=_p(r.acts[2].view, 8)), ALIGN),
    **{f"bwd-{k}-off-4": (lambda r, k=k: r.bwd(**{k: _p(r.f, 4)}), ALIGN) for k in ("w1", "w2")},
    "bwd-dt2-off-4": (lambda r: r.bwd(dt2=_p(r.dt2.view, 4)), ALIGN), "bwd-dt-off-12": (lambda r: r.bwd(dt=_p(r.dt.view, 12)), ALIGN),
    # mobgt_spmm_csr
    "csr-C6": (lambda r: r.csr(C=6), BAD), "csr-C0": (lambda r: r.csr(C=0), BAD), "csr-ldb-66": (lambda r: r.csr(ldb=66), BAD),
    "csr-ld_out-25": (lambda r: r.csr(ld_out=25), BAD), "csr-b-off-4": (lambda r: r.csr(b=_p(r.f, 4)), ALIGN),
    "csr-out-off-8": (lambda r: r.csr(out=_p(r.out.view, 8)), ALIGN), "csr-bias-off-4": (lambda r: r.csr(bias=_p(r.f, 4)), ALIGN),
    "csr-R0": (lambda r: r.csr(R=0), 0), "csr-R-negative": (lambda r: r.csr(R=-3), 0),
    # mobgt_spmm_csr_t_rows
    "t_rows-C0": (lambda r: r.t_rows(C=0), BAD), "t_rows-R0": (lambda r: r.t_rows(R=0), 0),
    # mobgt_spmm_csr_t_rows_gather
    "gather-C6": (lambda r: r.gather(C=6), BAD), "gather-C516": (lambda r: r.gather(C=516), BAD), "gather-C0": (lambda r: r.gather(C=0), BAD),
    "gather-ldg-66": (lambda r: r.gather(ldg=66), BAD), "gather-ld_db-25": (lambda r: r.gather(ld_db=25), BAD),
    "gather-g-off-4": (lambda r: r.gather(g=_p(r.f, 4)), ALIGN), "gather-db-off-8": (lambda r: r.gather(db=_p(r.db.view, 8)), ALIGN),
    "gather-P0": (lambda r: r.gather(P=0), 0), "gather-P0-R0": (lambda r: r.gather(P=0, R=0), 0),
}


@pytest.fixture(scope="module")
def refusal():
    return Refusal()


@pytest.mark.parametrize("name", list(REFUSALS), ids=list(REFUSALS))
def test_refusal(refusal, name):
    """Host-side checks: the status code comes back, no kernel runs, no destination and no counter changes."""
    fn, code = REFUSALS[name]
    assert fn(refusal) == code
    torch.cuda.synchronize()
    for o in refusal.outs:
        assert o.untouched()
    assert refusal.counter.result()[0] == 0 and (refusal.head.result() == -1).all() and (refusal.nxt.result() == MARK).all()
