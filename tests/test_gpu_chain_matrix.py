"""The encoder chain kernels (csrc/chain.hip) across their dispatch matrix, through the C ABI (tests/chain_abi.py), every case against
the float64 reference of tests/chain_reference.py.

Tolerances, per case and tensor: 2 x what the float64 EMULATION of the kernels' documented rounding points gives against the float64
reference on that very case (chain_reference.tolerances; the factor covers summation order, FMA contraction, the approximated erf and
the order of the atomics), in the per-row metric, the whole-tensor relative L2 and the largest element error; never below the f32
floor (chain_reference.TOL_FLOOR, sum_floor for what is summed over R rows) and, outside the common-mode and flat-row families,
never above what the existing chain tests allow.  tests/test_host_chain_reference.py shows on the CPU that these tolerances reject a
lost inv_keep, a swapped mask, a short column sum, a skipped k-step and the other mutants of chain_reference.mutant.

A "bwd" case feeds the backward the saved tensors (x1, x2, u, statistics) of the EMULATION, rounded to their storage types: the
backward is judged on its own.  A "both" case runs the device's forward and then its backward on the device's own saved tensors.
Every output buffer has guard rows past R (and guard columns where there is a leading dimension) that must stay untouched; where the
replayed mask drops an element the results are exact; the sparse family's zero rows are exactly zero.  The test ids name direction,
the form the dispatch reaches on this device (from its compute-unit count, as pick_ncl), width, R, family, layer kind, dropout."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import chain_abi as abi                                       # noqa: E402
import chain_reference as cr                                  # noqa: E402
from mobgt_amd import _lib, fused_layer, ops                  # noqa: E402
from mobgt_amd.fused_layer import chain_workspace             # noqa: E402

DEV = "cuda"
SEED = 77
GUARD, SENT = 3, 123.0
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
SPECS = cr.matrix_specs(CUS)
BF, F32 = torch.bfloat16, torch.float32


def device_keep(seed, salt, R, C, p):
    return ops.dropout_site_mask(seed, salt, R, C, p)


def seeds(mode, seed=SEED):
    """(host seed, device word): the effective seed is their sum."""
    if mode == "split":
        return seed - 11, torch.tensor([11], dtype=torch.int64, device=DEV)
    return seed, None


_W = {}


def weights(c):
    """The case's weights on the device, packed both ways (cached per width and family: they do not depend on R)."""
    k = (c.C, c.F, c.family)
    if k not in _W:
        if len(_W) > 8:
            _W.pop(next(iter(_W)))
        bf = lambda t: t.to(F32).to(BF).to(DEV)                # noqa: E731
        f = lambda t: t.to(F32).to(DEV)                        # noqa: E731
        wo, w1, w2, wq = bf(c.wo), bf(c.w1), bf(c.w2), bf(c.wq)
        _W[k] = dict(wo=abi.pack(wo), w1=abi.pack(w1), w2=abi.pack(w2), wq=abi.pack(wq), wot=abi.pack(wo, True), w1t=abi.pack(w1, True),
                     w2t=abi.pack(w2, True), wqt=abi.pack(wq, True), bo=bf(c.bo), b1=bf(c.b1), b2=bf(c.b2), bq=bf(c.bq),
                     n1w=f(c.n1w), n1b=f(c.n1b), nxw=f(c.nxw), nxb=f(c.nxb))
    w = dict(_W[k])
    if not c.has_norm:
        for n in ("nxw", "nxb"):
            del w[n]
    if c.last:
        for n in ("wq", "bq"):
            del w[n]
    return w


class Buffers:
    """Output buffers with GUARD sentinel rows past R (2-D) or GUARD sentinel elements past the end (1-D)."""

    def __init__(self):
        self.full, self.view = {}, {}

    def add(self, name, shape, dtype, fill=None, ld=None):
        if len(shape) == 2:
            full = torch.full((shape[0] + GUARD, ld or shape[1]), SENT, dtype=dtype, device=DEV)
            view = full[:shape[0], :shape[1]]
        else:
            full = torch.full((shape[0] + GUARD,), SENT, dtype=dtype, device=DEV)
            view = full[:shape[0]]
        if fill is not None:
            view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
        self.full[name], self.view[name] = full, view
        return view

    def assert_guards(self, label):
        for name, full in self.full.items():
            v = self.view[name]
            assert bool((full[v.shape[0]:] == SENT).all()), (label, name, "rows past R were written")
            if full.dim() == 2 and full.shape[1] > v.shape[1]:
                assert bool((full[:, v.shape[1]:] == SENT).all()), (label, name, "columns past N were written")

    def cpu(self):
        return {n: v.detach().to(torch.float64).cpu() for n, v in self.view.items()}


def workspace(s, c):
    return chain_workspace(torch.device(DEV, torch.cuda.current_device()), c.C, c.R) if s["form"] in ("cl4", "cl2", "ws_one") else None


def run_forward(s, c, seed=SEED):
    w, R, C, F = weights(c), c.R, c.C, c.F
    i = dict(a=c.a.to(F32).to(BF).to(DEV), x=c.x.to(F32).to(DEV))
    b = Buffers()
    for n, (N, dt) in dict(x1=(C, F32), z=(C, BF), u=(F, BF), h=(F, BF), x2=(C, F32)).items():
        b.add(n, (R, N), dt)
    for n in ("mean1", "rstd1"):
        b.add(n, (R,), F32)
    if c.has_norm:
        b.add("out_a", (R, C), BF)
        b.add("mean2", (R,), F32)
        b.add("rstd2", (R,), F32)
        if not c.preln:
            b.add("out", (R, C), F32)
        if not c.last:
            b.add("qkv", (R, 3 * C), BF)
    hs, sd = seeds(s["seed_mode"], seed)
    ws = workspace(s, c)
    for _ in range(2 if ws is not None else 1):                  # (the hand-over counters of the cluster forms must carry over)
        _lib.check(abi.chain_fwd(w, i, b.view, R, C, F, c.p_drop, hs, sd, ws), "mobgt_layer_chain_fwd")
    torch.cuda.synchronize()
    b.assert_guards(cr.spec_id(s, CUS))
    return b


def run_backward(s, c, saved, seed=SEED, prefill=0.0):
    """`saved`: x1, x2, u, statistics as float64 CPU tensors (the emulation's) or device tensors (the device forward's)."""
    w, R, C, F = weights(c), c.R, c.C, c.F
    dev = lambda t, dt: t if t.is_cuda else t.to(F32).to(dt).to(DEV)           # noqa: E731
    sv = {n: dev(t, BF if n == "u" else F32).contiguous() for n, t in saved.items()}
    i = dict(dout=c.dout.to(F32).to(DEV))
    if c.tail:
        i["dqkv"] = c.dqkv.to(F32).to(BF).to(DEV)
    b = Buffers()
    for n, (N, dt) in dict(df=(C, BF), du=(F, BF), dy=(C, BF), da=(C, BF), dx1=(C, F32)).items():
        b.add(n, (R, N), dt)
    for n in cr.SUMS:
        b.add(n, (C,), F32, fill=prefill)
    big = s["form"] == "bwd_big"
    if big:
        b.add("db1", (F,), F32, fill=prefill)
    pas = []
    for k, p in enumerate(c.wg):                                 # operands and results with leading dimensions wider than their rows
        g = torch.full((R, p.M + 8), SENT, dtype=BF, device=DEV)
        x = torch.full((R, p.N + 16), SENT, dtype=BF, device=DEV)
        g[:, :p.M], x[:, :p.N] = p.g.to(F32).to(BF).to(DEV), p.x.to(F32).to(BF).to(DEV)
        q = dict(g=g[:, :p.M], x=x[:, :p.N], dw=b.add("pw%d" % k, (p.M, p.N), F32, fill=prefill, ld=p.N + 4))
        if c.with_db:
            q["db"] = b.add("pb%d" % k, (p.M,), F32, fill=prefill)
        pas.append(q)
    hs, sd = seeds(s["seed_mode"], seed)
    if big:
        _lib.check(abi.chain_bwd_big(w, sv, i, b.view, R, C, F, c.p_drop, hs, sd), "mobgt_layer_chain_bwd_big")
    else:
        _lib.check(abi.chain_bwd(w, sv, i, b.view, R, C, F, c.p_drop, hs, sd, workspace(s, c), pas, preln=c.preln), "mobgt_layer_chain_bwd")
    torch.cuda.synchronize()
    b.assert_guards(cr.spec_id(s, CUS))
    return b


def check_dropped_forward(c, b):
    """Where the replayed mask drops an element the residual passes bit for bit."""
    if not c.p_drop:
        return
    x = c.x.to(F32).to(DEV)
    d1, d2 = (c.keep1 == 0).to(DEV), (c.keep2 == 0).to(DEV)
    assert abs(float(d1.double().mean()) - c.p_drop) < 0.03 or c.R * c.C < 4096
    assert torch.equal(b.view["x1"][d1], x[d1]) and torch.equal(b.view["x2"][d2], b.view["x1"][d2])
    if bool(d1.any()):
        assert not torch.equal(b.view["x1"][~d1], x[~d1])


def check_dropped_backward(c, b):
    if c.p_drop:
        d1, d2 = (c.keep1 == 0).to(DEV), (c.keep2 == 0).to(DEV)
        assert float(b.view["df"][d2].float().abs().sum()) == 0.0 and float(b.view["dy"][d1].float().abs().sum()) == 0.0
    if c.family == "sparse":
        zero = torch.ones(c.R, dtype=torch.bool)
        zero[c.nonzero] = False
        for n in ("df", "du", "dy", "da", "dx1"):
            assert float(b.view[n][zero.to(DEV)].float().abs().sum()) == 0.0, (n, "a zero row of dout leaked")


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: cr.spec_id(s, CUS))
def test_chain_matrix(spec):
    s = spec
    label = cr.spec_id(s, CUS)
    c = cr.spec_case(s, keep_fn=device_keep, seed=SEED)
    ref, emu = cr.case_reference(c), cr.case_emulation(c, cr.spec_split(s))
    saved = cr.saved_of(emu)
    if s["dir"] in ("fwd", "both"):
        b = run_forward(s, c)
        check_dropped_forward(c, b)
        # (y and f stay inside the kernels; a pre-LN layer's norm output leaves as bf16 only)
        names = [n for n in cr.fwd_names(c) if n not in ("y", "f") and (n != "out" or not c.preln)]
        cr.check(b.cpu(), ref, cr.tolerances(c, names, cr.spec_split(s)), label, emu)
        if "out" in b.view:
            assert torch.equal(b.view["out_a"], b.view["out"].to(BF))
        saved = {n: b.view[n] for n in saved}
    if s["dir"] in ("bwd", "both"):
        b = run_backward(s, c, saved)
        check_dropped_backward(c, b)
        names = cr.bwd_names(c, big=s["form"] == "bwd_big")
        cr.check(b.cpu(), ref, cr.tolerances(c, names, cr.spec_split(s)), label, emu)


FORM_CASES = [("one", 192, 33), ("cl4", 256, 65), ("cl2", 128, 16 * (min(CUS, 256) // 4) + 1), ("big64", 128, 4150), ("bwd_big", 192, 70)]
FORM_IDS = [f[0] for f in FORM_CASES]


def _spec(form, C, R, **kw):
    s = dict(dir="bwd", form=form, C=C, R=R, family="plain", p=0.0, seed_mode="host", preln=False, successor=True, last=False, tail=False,
             n_wg=0, with_db=True)
    s.update(kw)
    return s


@pytest.mark.parametrize("form,C,R", FORM_CASES, ids=FORM_IDS)
def test_without_dropout_the_seed_is_not_read(form, C, R):
    """p = 0: every output is identical to a run with any other seed (host and device word)."""
    s = _spec(form, C, R, tail=form != "big64")
    c = cr.spec_case(s)
    saved = cr.saved_of(cr.case_emulation(c, cr.spec_split(s)))
    runs = []
    for seed, mode in ((SEED, "host"), (0x1234567812345678, "split")):
        s2 = dict(s, seed_mode=mode)
        f = run_forward(s2, c, seed) if form != "bwd_big" else None
        runs.append((f, run_backward(s2, c, saved, seed)))
    for a, b in zip(*runs):
        if a is None:
            continue
        for n in a.view:
            if n in cr.SUMS or n == "db1":
                continue                                            # (f32 atomics: not bitwise repeatable)
            assert torch.equal(a.view[n], b.view[n]), (form, n)


@pytest.mark.parametrize("form,C,R", [f for f in FORM_CASES if f[0] != "big64"] + [("one", 128, 1040)], ids=FORM_IDS[:3] + FORM_IDS[4:] + ["one-split"])
def test_small_gradients_add_to_what_the_buffers_held(form, C, R):
    """The six [C] sums, db1 and the passengers' dw / db are ACCUMULATED: a run from a nonzero prefill gives the run from zeros plus the
    prefill, to f32 addition (one rounding of prefill + sum, and the order of the atomics: sum_floor(R) of the column's magnitude)."""
    s = _spec(form, C, R, p=0.1, tail=True, n_wg=0 if form == "bwd_big" else 4)
    c = cr.spec_case(s, keep_fn=device_keep, seed=SEED)
    saved = cr.saved_of(cr.case_emulation(c, cr.spec_split(s)))
    zero, pre = run_backward(s, c, saved), run_backward(s, c, saved, prefill=3.25)
    for n in cr.bwd_names(c, big=form == "bwd_big"):
        z, p = zero.view[n].double(), pre.view[n].double()
        if cr.kind_of(n) != "sums":
            continue
        assert float(z.abs().max()) > 0.0, n
        mag = 3.25 + float(z.abs().max())
        assert float((p - 3.25 - z).abs().max()) <= (2.0 ** -22 + cr.sum_floor(R)) * mag, (form, n)


@pytest.mark.parametrize("C,R,p", [(192, 185, 0.1), (256, 16 * (min(CUS, 256) // 4) + 16, 0.1), (128, 70, 0.0)])
def test_two_launches_on_one_workspace_repeat_and_match_the_one_workgroup_form(C, R, p):
    """The cluster forms, launched twice on the same workspace: everything in front of the first split-K sum (x1, z, u, h and the first
    norm's statistics; df, du) has identical bits both times AND the bits of the one-workgroup form."""
    s_cl = _spec("cl4", C, R, p=p, tail=True, seed_mode="split")
    assert cr.expected_form(R, True, CUS) in ("cl4", "cl2")
    s_one = dict(s_cl, form="one")
    c = cr.spec_case(s_cl, keep_fn=device_keep, seed=SEED)
    saved = cr.saved_of(cr.case_emulation(c, 1))
    f1, f2, f0 = run_forward(s_cl, c), run_forward(s_cl, c), run_forward(s_one, c)
    for n in ("x1", "z", "u", "h", "mean1", "rstd1"):
        assert torch.equal(f1.view[n], f2.view[n]) and torch.equal(f1.view[n], f0.view[n]), n
    b1, b2, b0 = run_backward(s_cl, c, saved), run_backward(s_cl, c, saved), run_backward(s_one, c, saved)
    for n in ("df", "du"):
        assert torch.equal(b1.view[n], b2.view[n]) and torch.equal(b1.view[n], b0.view[n]), n


def test_argument_checks_return_without_launching():
    """What the header promises to refuse: MOBGT_EBADDIM / MOBGT_EALIGN, and no output is touched."""
    s = _spec("one", 128, 33, tail=True)
    c = cr.spec_case(s)
    w, R, C, F = weights(c), c.R, c.C, c.F
    i = dict(a=c.a.to(F32).to(BF).to(DEV), x=c.x.to(F32).to(DEV))
    o = {n: torch.full((R, N), SENT, dtype=dt, device=DEV) for n, (N, dt) in
         dict(x1=(C, F32), z=(C, BF), u=(F, BF), h=(F, BF), x2=(C, F32), out=(C, F32), out_a=(C, BF), qkv=(3 * C, BF)).items()}
    o.update({n: torch.full((R,), SENT, device=DEV) for n in ("mean1", "rstd1", "mean2", "rstd2")})
    fwd = lambda w_, i_, o_, C_=C, F_=F: abi.chain_fwd(w_, i_, o_, R, C_, F_, 0.0, 0, None, None)            # noqa: E731
    no = lambda d, *ks: {k: v for k, v in d.items() if k not in ks}                                          # noqa: E731
    assert fwd(no(w, "wq", "bq"), i, o) == abi.EBADDIM                      # qkv_next without wq_next
    assert fwd(w, i, no(o, "qkv")) == abi.EBADDIM                           # ... and the reverse
    assert fwd(no(w, "nxw", "nxb"), i, o) == abi.EBADDIM                    # !nxw && wq_next
    assert fwd(w, i, o, 160, F) == abi.EBADDIM and fwd(w, i, o, C, 512) == abi.EBADDIM       # an unsupported (C, F)
    a_off = torch.zeros(R * C + 8, dtype=BF, device=DEV)[4:4 + R * C].view(R, C)             # 8 bytes off a 16-byte boundary
    assert a_off.data_ptr() % 16 == 8
    assert fwd(w, dict(i, a=a_off), o) == abi.EALIGN
    saved = {n: t.to(F32).to(BF if n == "u" else F32).to(DEV) for n, t in cr.saved_of(cr.case_emulation(c, 1)).items()}
    bi = dict(dout=c.dout.to(F32).to(DEV), dqkv=c.dqkv.to(F32).to(BF).to(DEV))
    bo = {n: torch.full((R, N), SENT, dtype=dt, device=DEV) for n, (N, dt) in dict(df=(C, BF), du=(F, BF), dy=(C, BF), da=(C, BF), dx1=(C, F32)).items()}
    bo.update({n: torch.full((C,), SENT, device=DEV) for n in cr.SUMS})
    assert abi.chain_bwd(w, saved, bi, bo, R, C, F, 0.0, 0, None, None, n_wg=5) == abi.EBADDIM
    assert abi.chain_bwd(w, saved, bi, bo, R, 160, F, 0.0, 0, None, None) == abi.EBADDIM
    assert abi.chain_bwd(no(w, "nxw"), saved, bi, bo, R, C, F, 0.0, 0, None, None) == abi.EBADDIM                 # post-LN without its norm
    assert abi.chain_bwd(no(w, "nxw"), saved, bi, bo, R, C, F, 0.0, 0, None, None, preln=True) == abi.EBADDIM     # a tail without the successor's norm
    assert abi.chain_bwd_big(no(w, "nxw"), saved, bi, bo, R, C, F, 0.0, 0, None) == abi.EBADDIM
    # the refusals of the 64-row dispatch: past 4 096 rows no tail, no passengers, no pre-LN through the common entry points
    Rb = cr.BIG_ROWS + 4
    big = lambda N, dt=F32: torch.zeros(Rb, N, dtype=dt, device=DEV)                                          # noqa: E731
    sv = dict(x1=big(C), x2=big(C), u=big(F, BF), mean1=torch.zeros(Rb, device=DEV), rstd1=torch.ones(Rb, device=DEV),
              mean2=torch.zeros(Rb, device=DEV), rstd2=torch.ones(Rb, device=DEV))
    ob = dict(df=big(C, BF), du=big(F, BF), dy=big(C, BF), da=big(C, BF), dx1=big(C), **{n: bo[n] for n in cr.SUMS})
    assert abi.chain_bwd(w, sv, dict(dout=big(C), dqkv=big(3 * C, BF)), ob, Rb, C, F, 0.0, 0, None, None) == abi.EBADDIM
    assert abi.chain_bwd(w, sv, dict(dout=big(C)), ob, Rb, C, F, 0.0, 0, None, None, preln=True) == abi.EBADDIM
    q = dict(g=big(C, BF), x=big(C, BF), dw=torch.zeros(C, C, device=DEV))
    assert abi.chain_bwd(w, sv, dict(dout=big(C)), ob, Rb, C, F, 0.0, 0, None, None, [q]) == abi.EBADDIM
    torch.cuda.synchronize()
    for d in (o, bo):
        for n, t in d.items():
            assert bool((t == SENT).all()), (n, "a refused call wrote")
    assert float(q["dw"].abs().max()) == 0.0


def test_the_workspace_key_follows_the_library_cluster_size(monkeypatch):
    """mobgt_chain_cluster_size answers what pick_ncl picks on this device -- 4 while 4 workgroups per 16-row block fit on its compute
    units (at most 256 count), then 2, then 1 -- and chain_workspace keys by that answer, not by a copy of the rule: with the entry
    point answering 2 where the library says 4, the same (device, C, R) gets another workspace.  No kernel runs."""
    lib, cus = _lib.lib(), min(CUS, 256)
    rows = (16, 4 * cus, 4 * cus + 16, 8 * cus, 8 * cus + 16)
    assert [lib.mobgt_chain_cluster_size(R) for R in rows] == [4, 4, 2, 2, 1]
    dev = torch.device(DEV, torch.cuda.current_device())
    own = chain_workspace(dev, 192, 16)
    assert chain_workspace(dev, 192, 4 * cus) is own and chain_workspace(dev, 192) is own
    monkeypatch.setattr(lib, "mobgt_chain_cluster_size", lambda R: 2)
    monkeypatch.setattr(fused_layer, "_CHAIN_NCL", {})       # (the answers are kept per device and row count: ask again)
    other = chain_workspace(dev, 192, 16)
    assert other is not own and other.data_ptr() != own.data_ptr()
    assert other is chain_workspace(dev, 192, 4 * cus + 16)
