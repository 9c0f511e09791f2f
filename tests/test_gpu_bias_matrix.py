"""The bias assembly kernels (csrc/bias.hip) across their dispatch matrix, through the C ABI (tests/bias_abi.py), against the float64
reference of tests/bias_reference.py: every form `launch_build` / `launch_build_bwd` / DISPATCH_IDX / mobgt_bias_pack can reach, each
case in both input families -- EXACT (the device must return the reference's bits) and ROUNDING (bounds from u = 2^-24 and the
documented rounding points).  Every output and accumulator carries GUARD sentinel elements past its end; the accumulators start from
non-zero values; the padding columns [T, ld) and row 0 of dBias hold NaN.  The last test prints the worst err / bound per form."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bias_reference as br                                             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
HAVE = torch.cuda.is_available()
CUS = torch.cuda.get_device_properties(0).multi_processor_count if HAVE else 256
SPECS = br.matrix_specs(CUS)
WORST, COUNT = {}, {}
_INPUTS, _FREF, _GRAD = {}, {}, {}


def abi():
    import bias_abi
    return bias_abi


def codes(s):
    a = abi()
    c = dict(i64=a.I64, i32=a.I32, i16=a.I16, u8=a.U8, f32=a.F32, bf16=a.BF16)
    return c[s["idx"]], c[s["edge"]]


class Buffers:
    """Flat device buffers with GUARD sentinel elements past the end; `view[name]` is the tensor the kernel is given."""

    def __init__(self):
        self.full, self.view = {}, {}

    def add(self, name, shape, dtype, fill=None):
        n = 1
        for v in shape:
            n *= v
        full = torch.full((n + GUARD,), br.SENT, dtype=dtype, device=DEV)
        view = full[:n].view(shape)
        if fill is not None:
            view.copy_(fill)
        self.full[name], self.view[name] = full, view
        return view

    def assert_guards(self, label):
        for name, full in self.full.items():
            n = self.view[name].numel()
            assert bool((full[n:] == torch.tensor(br.SENT, dtype=full.dtype)).all()), (label, name, "elements past the end were written")

    def assert_untouched(self, label, fills):
        self.assert_guards(label)
        for name, v in self.view.items():
            want = fills.get(name)
            same = torch.equal(v, want) if want is not None else bool((v == torch.tensor(br.SENT, dtype=v.dtype)).all())
            assert same, (label, name, "a refused call wrote")


def inputs(s, family):
    key = br.input_key(s, family)
    if key not in _INPUTS:
        _INPUTS[key] = br.build_inputs(s, family, DEV)
    return _INPUTS[key]


def kernel_inputs(s, inp):
    D = s["D"]
    i = {k: inp[k] for k in ("attn_bias", "rel_pos", "poi_pos", "rel_table", "poi_table", "vdist")}
    i["edge_input"] = inp["edge_input"] if D > 0 else None                       # D = 0: edge_input dropped
    i["hop_table"] = inp["hop_table"][:D].contiguous() if D > 0 else None        # [D, n_edge, H]: the kernel's table ends at D
    return i


def dims(s, **kw):
    return dict({k: s[k] for k in ("G", "N", "H", "D_in", "D", "F", "n_rel", "n_poi", "n_edge", "ld")}, **kw)


def note(s, ratio):
    f = br.form_of(s) + (" " + s["out"] if s["dir"] == "fwd" else "")
    WORST[f] = max(WORST.get(f, 0.0), ratio)
    COUNT[f] = COUNT.get(f, 0) + 1


def forward_reference(s, family):
    key = br.input_key(s, family)
    if key not in _FREF:
        _FREF[key] = br.forward(inputs(s, family), s["D"])
    return _FREF[key]


def run_forward(s, family, check=True):
    t0 = time.time()
    a, inp = abi(), inputs(s, family)
    G, H, T, ld = s["G"], s["H"], s["T"], s["ld"]
    b = Buffers()
    b.add("bias", (G, H, T, ld), br.OUT[s["out"]])
    if s["bias_t"]:
        b.add("bias_t", (G, H, T, ld), br.OUT[s["out"]])
    rc = a.build_bias(kernel_inputs(s, inp), b.view, dims(s), *codes(s), a.BF16 if s["out"] == "bf16" else a.F32)
    assert rc == 0, (s["id"], rc)
    torch.cuda.synchronize()
    b.assert_guards(s["id"])
    if check:
        ref, mag = forward_reference(s, family)
        ok, worst, why = br.forward_verdict(s, family, b.view["bias"], b.view.get("bias_t"), ref, mag)
        print("%s %s err/bound %.3g (%.2f s)" % (s["id"], family, worst, time.time() - t0))
        assert ok, (s["id"], family, why, worst)
        note(s, worst)
    return b


def gradient(s, family):
    key = br.input_key(s, family) + (s["ld"], s["L"], s["db"], s["special"])
    if key not in _GRAD:
        inp, init = inputs(s, family), br.init_tables(s, DEV)
        x, K, spot = br.build_grad(s, inp, family, DEV)
        ref = br.backward(inp, x, s["D"], init, stats=family == "round")
        mx = float(torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).max())
        _GRAD[key] = (init, x, K, spot, ref, mx)
    return _GRAD[key]


def run_backward(s, family, call=None):
    t0 = time.time()
    a, inp = abi(), inputs(s, family)
    init, x, K, spot, ref, mx = gradient(s, family)
    G, H, T, ld, L = s["G"], s["H"], s["T"], s["ld"], s["L"]
    one = G * H * T * ld
    stride = one + s["gap"]
    dt = BF if s["db"] == "bf16" else F32
    src = torch.full((L * stride,), float("nan"), dtype=dt, device=DEV)           # (the gaps between the slices: NaN as well)
    for l in range(L):
        src[l * stride:l * stride + one].view(G, H, T, ld).copy_(x[l])
    b = Buffers()
    for name in ("d_rel", "d_poi", "d_hop", "d_vdist"):
        if init[name] is not None:
            b.add(name, tuple(init[name].shape), F32, init[name])
    g = dict(b.view, dbias=src)
    args = (kernel_inputs(s, inp), g, dims(s), a.BF16 if s["db"] == "bf16" else a.F32, L, stride, *codes(s))
    rc = (call or a.build_bias_bwd)(*args)
    assert rc == 0, (s["id"], rc)
    torch.cuda.synchronize()
    b.assert_guards(s["id"])
    ok, worst, why = br.backward_verdict(s, family, b.view, ref, init, mx)
    print("%s %s K=%s err/bound %.3g (%.2f s)" % (s["id"], family, K, worst, time.time() - t0))
    assert ok, (s["id"], family, why, worst)
    note(s, worst)
    return b, spot


# ------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("s", [s for s in SPECS if s["dir"] == "fwd"], ids=lambda s: s["id"])
def test_forward(s):
    for family in ("exact", "round"):
        run_forward(br.for_family(s, family), family)


@pytest.mark.parametrize("s", [s for s in SPECS if s["dir"] == "bwd"], ids=lambda s: s["id"])
def test_backward(s):
    a = abi()
    families = ("exact",) if s["special"] else ("exact", "round")                 # (the fixed-point fallbacks: EXACT only)
    for family in families:
        sf = br.for_family(s, family)
        if s["wg"] is None:
            _, spot = run_backward(sf, family)
            if s["special"] == "nan":
                assert spot is not None
            continue
        try:                                                                       # fewer persistent workgroups: no effect on results
            assert a.set_workgroups(s["wg"]) == 0
            run_backward(sf, family)
        finally:
            assert a.set_workgroups(0) == 0
        run_backward(sf, family)


def test_long_bf16_pack_is_the_rounding_of_the_f32_pack():
    """Long form: the bf16 output keeps its tile in the output type and sends the direct copy through LDS; it must be, bit for bit,
    the round-to-nearest-even of what the f32 instantiation writes (ROUNDING inputs: the values need rounding)."""
    s32 = next(s for s in SPECS if s["dir"] == "fwd" and br.fwd_form(s) == "long" and s["out"] == "f32" and s["bias_t"] and s["N"] == 255)
    b32 = run_forward(s32, "round", check=False)
    b16 = run_forward(dict(s32, out="bf16"), "round", check=False)
    for name in ("bias", "bias_t"):
        assert torch.equal(b32.view[name].to(BF), b16.view[name]), name


# ------------------------------------------------------------------------------------------------ mobgt_bias_pack
@pytest.mark.parametrize("T", [1, 31, 32, 33, 65])
@pytest.mark.parametrize("pair", ["f32-f32", "f32-bf16", "bf16-f32", "bf16-bf16"])
def test_bias_pack(pair, T):
    a = abi()
    sd, od = pair.split("-")
    code = dict(f32=a.F32, bf16=a.BF16)
    gen = torch.Generator(device=DEV).manual_seed(T)
    for G, H in ((1, 1), (2, 3)):
        for layout in ("contiguous", "broadcast heads", "swapped", "padded pitch"):
            for ldq, with_t in ((32, True), (64, True), (32, False)):
                ld = -(-T // ldq) * ldq
                Hs = 1 if layout == "broadcast heads" else H
                base = torch.randn((G, Hs, T, T + (3 if layout == "padded pitch" else 0)), generator=gen, device=DEV).to(br.OUT[sd])
                base[torch.rand(base.shape, generator=gen, device=DEV) < 0.1] = float("-inf")
                src = base[..., :T]
                if layout == "swapped":
                    src = src.transpose(2, 3)
                st = list(src.stride())
                if layout == "broadcast heads":
                    st[1] = 0
                b = Buffers()
                b.add("bias", (G, H, T, ld), br.OUT[od])
                if with_t:
                    b.add("bias_t", (G, H, T, ld), br.OUT[od])
                rc = a.bias_pack(src, code[sd], st, b.view["bias"], b.view.get("bias_t"), code[od], G, H, T, ld)
                label = (pair, T, G, H, layout, ld, with_t)
                assert rc == 0, label
                torch.cuda.synchronize()
                b.assert_guards(label)
                want, want_t = br.pack_reference(src.expand(G, H, T, T), ld, od)
                assert br.same_bits(b.view["bias"], want), label
                assert bool(torch.equal(torch.isneginf(b.view["bias"][..., :T]), torch.isneginf(src.expand(G, H, T, T)))), label
                if with_t:
                    assert br.same_bits(b.view["bias_t"], want_t), label


# ------------------------------------------------------------------------------------------------ the small GEMM riding along
def test_front_small_gemm_job_rides_in_the_short_h8_launch_only():
    a = abi()
    M, N, K = 1024, 16, 128
    gen = torch.Generator(device=DEV).manual_seed(3)
    A, B = torch.randn((M, K), generator=gen, device=DEV), torch.randn((K, N), generator=gen, device=DEV)
    c = Buffers()
    c.add("c", (M, N), F32)
    short8 = next(s for s in SPECS if s["dir"] == "fwd" and br.fwd_form(s) == "short8" and s["N"] == 65 and s["out"] == "f32")
    short4 = next(s for s in SPECS if s["dir"] == "fwd" and br.fwd_form(s) == "short4" and s["N"] == 65)
    long8 = next(s for s in SPECS if s["dir"] == "fwd" and br.fwd_form(s) == "long" and s["out"] == "f32")
    plain = run_forward(short8, "round")
    try:
        assert a.front_sgemm_pending() == 0
        assert a.front_sgemm_job(A, B, None, 0, 0.0, c.view["c"], M, N, K, K) == 0
        assert a.front_sgemm_pending() == 1
        run_forward(short4, "exact")
        assert a.front_sgemm_pending() == 1                                       # an H = 4 launch leaves it
        run_forward(long8, "exact")
        assert a.front_sgemm_pending() == 1                                       # so does a long launch
        riding = run_forward(short8, "round")
        assert a.front_sgemm_pending() == 0                                       # the short H = 8 launch takes it
    finally:
        assert a.front_sgemm_job(None, None, None, 0, 0.0, None, 0, 0, 0, 0) == 0
    for name in ("bias", "bias_t"):
        assert torch.equal(plain.view[name], riding.view[name]), name
    c.assert_guards("front job")
    ref = A.to(F64) @ B.to(F64)
    ok, worst = br.within(c.view["c"], ref, (K + 8) * br.U * (A.to(F64).abs() @ B.to(F64).abs()))
    assert ok, worst


# ------------------------------------------------------------------------------------------------ the passenger form
def _gcn_side(n=16, K0=16, H1=16, H2=64, H3=32):
    z = lambda *shape: torch.zeros(shape, dtype=F32, device=DEV)                  # noqa: E731
    gen = torch.Generator(device=DEV).manual_seed(9)
    r = lambda *shape: torch.randn(shape, generator=gen, device=DEV)             # noqa: E731
    w = dict(g=z(n, H3), ax=r(n, K0), a_t=r(n, n), w1=r(H1, H2), w2=r(H2, H3), h1=r(n, H1), t=r(n, H1), h2=r(n, H2), t2=r(n, H2),
             dw0=z(K0, H1), db0=z(H1), dw1=z(H1, H2), db1=z(H2), dw2=z(H2, H3), db2=z(H3), dt2=z(n, H2), dt=z(n, H1), counter=z(4))
    return dict(n=n, K0=K0, H1=H1, H2=H2, H3=H3), w


@pytest.mark.parametrize("D,D_in", [(3, 4), (20, 20)])
def test_backward_as_passenger_of_the_category_gcn_launch(D, D_in):
    """mobgt_small_gcn_bwd_bias with with_bias = 1 beside a single GCN workgroup whose incoming gradient is all zeros: the bias
    tables' gradients must be the reference's bits (EXACT family); and the shapes it does not cover are refused."""
    a = abi()
    s = dict(br.spec(N=33, G=3, D=D, D_in=D_in, n_edge=40, big_ids=True, ragged=True, db="bf16", L=2, tag="passenger"), dir="bwd")
    s["id"] = br.spec_id(s, CUS)

    def call(*args):
        n_, w = _gcn_side()
        return a.small_gcn_bwd_bias(n_, w, *args)
    run_backward(s, "exact", call=call)
    inp = inputs(s, "exact")
    init, x, _, _, _, _ = gradient(s, "exact")
    i = kernel_inputs(s, inp)
    for label, ki, kd, idx_code in (("I64 ids", i, {}, a.I64), ("H = 4", i, dict(H=4), a.I16), ("F = 2", i, dict(F=2), a.I16),
                                    ("D = 21", i, dict(D=21, D_in=21), a.I16), ("edge_input NULL", dict(i, edge_input=None), {}, a.I16),
                                    ("G T^2 >= 2^20", i, dict(G=16, N=255, ld=256), a.I16)):
        b = Buffers()
        for name in ("d_rel", "d_poi", "d_hop", "d_vdist"):
            b.add(name, tuple(init[name].shape), F32, init[name])
        g = dict(b.view, dbias=x.to(BF).contiguous())
        n_, w = _gcn_side()
        rc = a.small_gcn_bwd_bias(n_, w, ki, g, dims(s, **kd), a.BF16, 2, x[0].numel(), idx_code, a.U8)
        assert rc == a.EBADDIM, (label, rc)
        torch.cuda.synchronize()
        b.assert_untouched(label, init)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_every_buffer_untouched():
    """(MOBGT_I32 and MOBGT_BF16 are both 1 in the header, so 'bias dtype I32' IS bf16 and cannot be refused: the unknown bias /
    dBias dtype codes tried here are 2 (MOBGT_I16 as a number) and 7.)"""
    a = abi()
    s = dict(br.spec(N=33, G=3, D=3, D_in=4, db="bf16", L=2), dir="bwd")
    inp = inputs(s, "exact")
    init, x, _, _, _, _ = gradient(s, "exact")
    i = kernel_inputs(s, inp)
    ic, ec = codes(s)
    G, H, T, ld = s["G"], s["H"], s["T"], s["ld"]
    bad = [("H = 2", dict(H=2), ic, ec, a.F32, 2, a.EBADDIM), ("H = 16", dict(H=16), ic, ec, a.F32, 2, a.EBADDIM),
           ("G = 0", dict(G=0), ic, ec, a.F32, 2, a.EBADDIM), ("N = 0", dict(N=0), ic, ec, a.F32, 2, a.EBADDIM),
           ("D > D_in", dict(D=5), ic, ec, a.F32, 2, a.EBADDIM), ("F = 0", dict(F=0), ic, ec, a.F32, 2, a.EBADDIM),
           ("n_slices = 0", {}, ic, ec, a.F32, 0, a.EBADDIM),
           ("ld % 32 != 0", dict(ld=ld + 8), ic, ec, a.F32, 2, a.EALIGN), ("ld < N + 1", dict(ld=32), ic, ec, a.F32, 2, a.EALIGN),
           ("(I16, I16)", {}, a.I16, a.I16, a.F32, 2, a.EDTYPE), ("(I64, I32)", {}, a.I64, a.I32, a.F32, 2, a.EDTYPE),
           ("dtype code 2", {}, ic, ec, 2, 2, a.EDTYPE), ("dtype code 7", {}, ic, ec, 7, 2, a.EDTYPE)]
    for label, kd, idx_code, edge_code, dt_code, n_slices, want in bad:
        f, b = Buffers(), Buffers()
        f.add("bias", (G, H, T, ld), F32)
        f.add("bias_t", (G, H, T, ld), F32)
        for name in ("d_rel", "d_poi", "d_hop", "d_vdist"):
            b.add(name, tuple(init[name].shape), F32, init[name])
        if label != "n_slices = 0":
            rc = a.build_bias(i, f.view, dims(s, **kd), idx_code, edge_code, dt_code)
            assert rc == want, ("fwd", label, rc)
        db_code = dt_code if label.startswith("dtype code") else a.BF16
        rc = a.build_bias_bwd(i, dict(b.view, dbias=x.to(BF).contiguous()), dims(s, **kd), db_code, n_slices, x[0].numel(), idx_code, edge_code)
        assert rc == want, ("bwd", label, rc)
        torch.cuda.synchronize()
        f.assert_untouched(label, {})
        b.assert_untouched(label, init)
    assert a.set_workgroups(-1) == a.EBADDIM
    assert a.set_workgroups(0) == 0


def test_zz_report_worst_ratio_per_form(capsys):
    """For docs/NOTEBOOK.md: per form, the cases run and the worst err / bound of the ROUNDING family (EXACT cases count as 0)."""
    with capsys.disabled():
        print("\nbias matrix: form, verdicts, worst err/bound")
        for f in sorted(COUNT):
            print("  %-16s %4d  %.4f" % (f, COUNT[f], WORST[f]))
    assert all(v <= 1.0 for v in WORST.values())
