"""The bf16 attention kernels (csrc/attn.hip) across their whole dispatch matrix, and the f32 body (csrc/attn_f32_body.h) on the
families the old f32 tests lack -- every case against the float64 reference of tests/attn_reference.py, through ops.pack_bias /
ops.attention / ops.attention_qkv.

bf16 tolerances, per case and tensor: 2 x what the float64 EMULATION of the kernels' documented rounding points gives against the
float64 reference on that very case (attn_reference.tolerances; the factor covers summation order, FMA contraction and the order
of the one-pass dQ atomics), in the per-head-row metric, the whole-tensor relative L2 and the largest element error; outside the
common-mode family never above the c5 ceilings of test_gpu_c5.py.  tests/test_host_attn_reference.py shows on the CPU that these
tolerances reject a lost key, a skipped chunk, a transposed mask or bias, an overwritten second bias use and an inconsistent delta.
Gradients of padded keys (dk / dv rows, dbias columns) are asserted exactly zero.

Which kernel a case reaches (launch_nw / launch_one in attn.hip, _attn_bwd in ops.py): forward attn_fwd_kernel<D, bf16, TB, NW, DROP>
with NW = 1 (T <= 32), 2 (T <= 64), 4; backward form `slice` = attn_bwd_both_kernel (T <= 64) or attn_bwd_one_kernel +
attn_dq_finish_kernel (T > 64), `slice2p` = attn_bwd_dq_kernel + attn_bwd_dkv_kernel with a bf16 dBias slice, `f32acc` = the same
kernels with TB = float and the f32 dBias accumulator, `nodb` = no bias gradient.  The test ids name family, T, d, H, form, dropout.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_reference as ar                                   # noqa: E402
from mobgt_amd import ops                                     # noqa: E402

DEV = "cuda"
SEED = 0x5DEECE66D1234567
SPECS = ar.matrix_specs()


def device_keep(seed, G, H, T, p_drop):
    return ops.dropout_keep_mask(seed, G, H, T, p_drop)


def _dq_key(case):
    return (str(torch.device(DEV, torch.cuda.current_device())), int(torch.cuda.current_stream().cuda_stream), case.G * case.T * case.C)


def run_device(case, form, seed_mode="host", io=torch.bfloat16, fused_qkv=False):
    """The case on the device: dict like attn_reference._run's (out, dq, dk, dv [+ ...2], dbias), float64 on the CPU."""
    bias_dtype, want_db, _ = ar.FORMS[form]
    bt = torch.bfloat16 if bias_dtype == "bf16" else torch.float32
    bd = case.bias.to(torch.float32).to(DEV)
    if want_db:
        bd.requires_grad_(True)
    pack = ops.pack_bias(bd, case.G, case.H, case.T, dtype=bt)
    kw = {}
    if case.p_drop:
        kw = dict(p_drop=case.p_drop, seed=SEED, seed_dev=None)
        if seed_mode == "split":
            kw.update(seed=SEED - 11, seed_dev=torch.tensor([11], dtype=torch.int64, device=DEV))
    res, leaves, loss = {}, [], None
    for tag, (q, k, v, gy) in ar._uses(case):
        if fused_qkv:
            qkv = torch.cat([q, k, v], dim=2).to(io).to(DEV).requires_grad_(True)
            out = ops.attention_qkv(qkv, pack, case.scale, **kw)
            leaves.append((tag, qkv))
        else:
            qd, kd, vd = (t.to(io).to(DEV).requires_grad_(True) for t in (q, k, v))
            out = ops.attention(qd, kd, vd, pack, case.scale, **kw)
            leaves.append((tag, (qd, kd, vd)))
        assert out.dtype == io
        res["out" + tag] = out.detach()
        term = (out.float() * gy.to(torch.float32).to(DEV)).sum()
        loss = term if loss is None else loss + term
    loss.backward()
    torch.cuda.synchronize()
    C = case.C
    for tag, leaf in leaves:
        if fused_qkv:
            g = leaf.grad
            res["dq" + tag], res["dk" + tag], res["dv" + tag] = g[..., :C], g[..., C:2 * C], g[..., 2 * C:]
        else:
            res["dq" + tag], res["dk" + tag], res["dv" + tag] = (x.grad for x in leaf)
    if want_db:
        res["dbias"] = bd.grad
    return {n: t.detach().to(torch.float64).cpu() for n, t in res.items()}, {n: t.detach().clone() for n, t in res.items()}


def check_entry_point(case, form):
    """The one-pass form creates (or uses) its dQ accumulator and leaves it all zeros; no other form creates one."""
    key = _dq_key(case)
    if form == "slice" and case.T > 64:
        assert key in ops._DQ_ACC and not ops._DQ_ACC[key]["busy"]
        assert float(ops._DQ_ACC[key]["buf"].abs().max()) == 0.0
    else:
        assert key not in ops._DQ_ACC, (form, key)


@pytest.mark.parametrize("spec", SPECS, ids=ar.spec_id)
def test_bf16_matrix(spec, monkeypatch):
    monkeypatch.setattr(ops, "_DQ_ACC", {})
    monkeypatch.setattr(ops, "_ATTN_ONE_PASS", [not ar.FORMS[spec["form"]][2]])
    case = ar.spec_case(spec, keep_fn=device_keep)
    if case.p_drop:
        assert abs(1.0 - float(case.keep.mean()) - case.p_drop) < 0.03
    got, _ = run_device(case, spec["form"], spec["seed_mode"])
    check_entry_point(case, spec["form"])
    ar.assert_padding_zero(got, case)
    ar.check(got, ar.case_reference(case), ar.spec_tolerances(spec, case), case, ar.spec_id(spec))
    if case.family == "one_key" and not case.p_drop:
        # ONE valid key: P = 1, the output row IS v[g, 0] of its head
        v0 = ar._heads(case.v, case.H)[0, :, 0]
        assert torch.equal(ar._heads(got["out"], case.H)[0], v0.unsqueeze(1).expand(-1, case.T, -1))


@pytest.mark.parametrize("d", ar.D_ALL)
@pytest.mark.parametrize("T", [20, 50, 130])
def test_bf16_strided_qkv_is_bit_equal_and_right(T, d, monkeypatch):
    """attention_qkv (rows of one [G, T, 3C] projection, row stride 3C) against the separate-tensor call and the reference;
    with the bias gradient, dropout on at T = 50."""
    monkeypatch.setattr(ops, "_DQ_ACC", {})
    p = 0.1 if T == 50 else 0.0
    case = ar.make_case(T, d, ar.heads_for(T), p_drop=p, keep_fn=device_keep, seed=SEED)
    sep, sep_raw = run_device(case, "slice", "split")
    fused, fused_raw = run_device(case, "slice", "split", fused_qkv=True)
    for n in ("out", "dk", "dv", "dbias") + (("dq",) if T <= 64 else ()):      # (one-pass dQ: f32 atomics, not bitwise repeatable)
        assert torch.equal(sep_raw[n], fused_raw[n]), n
    ar.assert_padding_zero(fused, case)
    ar.check(fused, ar.case_reference(case), ar.tolerances(case, ar.emu_form(T, "slice")), case, "qkv-T%d-d%d" % (T, d))
    if T > 64:
        monkeypatch.setattr(ops, "_ATTN_ONE_PASS", [False])
        sep2, sep2_raw = run_device(case, "slice2p", "split")
        fused2, fused2_raw = run_device(case, "slice2p", "split", fused_qkv=True)
        for n in ("out", "dq", "dk", "dv", "dbias"):
            assert torch.equal(sep2_raw[n], fused2_raw[n]), n
        ar.check(fused2, ar.case_reference(case), ar.tolerances(case, "two"), case, "qkv2p-T%d-d%d" % (T, d))


# ------------------------------------------------------------------------------------------------ f32 I/O (attn_f32_body.h)
def _check_f32(got, ref, case):
    """The tolerances of test_attention_fwd_bwd_f32, against the UNROUNDED float64 reference."""
    for n, g in got.items():
        w = ref[n].numpy()
        if ar._kind(n) in ("out", "dbias"):
            np.testing.assert_allclose(g.numpy(), w, atol=1e-5, rtol=1e-4, err_msg=n)
        else:
            np.testing.assert_allclose(g.numpy(), w, atol=1e-4 * max(1.0, np.abs(w).max()), rtol=1e-4, err_msg=n)
    ar.assert_padding_zero(got, case)


@pytest.mark.parametrize("d", ar.D_ALL)
@pytest.mark.parametrize("T", [33, 64, 65, 130])
@pytest.mark.parametrize("family", ["dropout", "two_use", "strided"])
def test_f32_io_families(family, T, d, monkeypatch):
    monkeypatch.setattr(ops, "_DQ_ACC", {})
    p = {"dropout": 0.1 if (T + d) % 2 else 0.5, "two_use": 0.0, "strided": 0.1}[family]
    case = ar.make_case(T, d, ar.heads_for(T), family="two_use" if family == "two_use" else "plain", p_drop=p, bias_dtype="f32",
                        io="f32", keep_fn=device_keep, seed=SEED)
    got, raw = run_device(case, "f32acc", "split" if T % 2 else "host", io=torch.float32, fused_qkv=family == "strided")
    assert _dq_key(case) not in ops._DQ_ACC
    _check_f32(got, ar.case_reference(case), case)
    if family == "strided":
        _, raw2 = run_device(case, "f32acc", "split" if T % 2 else "host", io=torch.float32)
        for n in raw:
            assert torch.equal(raw[n], raw2[n]), n
