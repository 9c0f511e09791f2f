"""The verdicts of tests/head_reference.py reject what tests/test_gpu_head_matrix.py relies on them to reject: a float32 numpy
emulation of the classifier head and the two losses passes clean, and fails with each planted defect -- in both input families
for the products, under the loss gate for the losses.  No GPU."""
import numpy as np
import pytest

import head_reference as hr

# small shapes with more than one column tile, a ragged last tile, several non-empty dx slices, and G > 1
SHAPES = [(5, 64, 200), (16, 48, 33), (3, 260, 1030)]
ALPHA = 0.2


def product_verdicts(case, out):
    return {k: hr.product_verdict(case, k, out[k]) for k in ("y", "dx", "dW", "db")}


@pytest.mark.parametrize("family", ["exact", "round"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_clean_product_emulation_passes(shape, family):
    case = hr.build_case(*shape, family)
    res = product_verdicts(case, hr.emulate_products(case))
    assert all(ok for ok, _ in res.values()), res
    if family == "round":
        assert all(0 < r <= 1 for _, r in res.values()), res          # (and the bound is no formality: real error is measured)


@pytest.mark.parametrize("family", ["exact", "round"])
@pytest.mark.parametrize("defect", hr.PRODUCT_DEFECTS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_planted_product_defect_is_rejected(shape, defect, family):
    case = hr.build_case(*shape, family)
    res = product_verdicts(case, hr.emulate_products(case, defect))
    hit = {"dropped last column tile": "y", "bias added twice": "y", "dropped V-slice of dx": "dx", "doubled V-slice of dx": "dx",
           "db over the wrong axis": "db"}[defect]
    assert not res[hit][0], (defect, res)
    assert all(ok for k, (ok, _) in res.items() if k != hit), res


def test_product_without_bias_and_a_shape_mismatch():
    case = hr.build_case(4, 16, 40, "exact", bias=False)
    out = hr.emulate_products(case)
    assert all(ok for ok, _ in product_verdicts(case, out).values())
    with_bias = hr.build_case(4, 16, 40, "exact", bias=True)
    assert not hr.product_verdict(with_bias, "y", out["y"])[0]           # a bias that was not added
    assert not hr.exact_verdict(out["db"][:-1], case["ref"]["db"])
    r = hr.build_case(4, 16, 40, "round")
    assert not hr.round_verdict(np.full_like(r["ref"]["y"], np.nan), r["ref"]["y"], r["bound"]["y"])[0]


def test_builders_keep_their_own_conditions():
    for G, K, V in hr.PRODUCT_SHAPES[:4] + [(16, 512, 1030)]:
        if V > 5000:
            continue
        hr.check_case(hr.build_case(G, K, V, "exact"))
        case = hr.build_case(G, K, V, "round")
        assert float(np.abs(case["ref"]["y"]).max()) <= 8.0
        assert V < 1000 or float(np.abs(case["ref"]["y"]).max()) > 5.0   # (with many columns the range is used, not idle)
    assert 9 * 512 + 3 < 2 ** 24 and 9 * 40000 < 2 ** 24
    bad = hr.build_case(3, 16, 8, "exact")
    bad["ref"]["y"] = bad["ref"]["y"] + 0.5
    with pytest.raises(AssertionError):
        hr.check_case(bad)
    wide = hr.build_case(3, 16, 8, "round")
    wide["ref"]["y"] = wide["ref"]["y"] * 4
    with pytest.raises(AssertionError):
        hr.check_case(wide)


def test_the_shape_lists_cover_what_they_claim():
    Gs, Ks, Vs = ({s[i] for s in hr.PRODUCT_SHAPES} for i in range(3))
    assert Gs == {1, 3, 4, 5, 15, 16}
    assert Ks == {4, 16, 48, 64, 128, 192, 252, 256, 260, 320, 384, 448, 508, 512}
    assert Vs == {1, 3, 5, 15, 16, 17, 31, 32, 33, 255, 256, 257, 513, 1030, 2047, 2048, 2049, 4097, 32767, 32768, 32769}
    for kt in range(1, 8):
        assert any(K == 64 * kt and V < 256 for _, K, V in hr.PRODUCT_SHAPES)
        assert any(K == 64 * kt and V == 32769 for _, K, V in hr.PRODUCT_SHAPES)
    assert {hr.dx_slices(V) for _, K, V in hr.PRODUCT_SHAPES if K % 16 == 0 and V in (32767, 32768)} == {8, 32}
    assert {hr.gtl_blocks(V) for _, _, V in hr.GTL_SHAPES} >= {1, 2, 7, 8, 9, 1024}
    assert {K // 64 for _, K, _ in hr.GTL_SHAPES} == set(range(1, 8))
    assert {g for g, _ in hr.CE_SHAPES} == {1, 3, 16, 257, 4095} and {v for _, v in hr.CE_SHAPES} == {1, 2, 255, 256, 257, 1000, 10239, 10240}
    assert hr.forms_for(252) == ["fwd", "bwd"] and hr.forms_for(48) == ["fwd", "bwd", "dx", "bwd_both"]
    assert "gtl" in hr.forms_for(448) and "gtl" not in hr.forms_for(512)


def gtl_inputs(G, K, V, off):
    case = hr.build_case(G, K, V, "round")
    return case["ref"]["y"].astype(np.float32), hr.targets_for(G, V, off)


@pytest.mark.parametrize("off", [0, -1])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gtl_gate_accepts_f32_and_rejects_the_planted_defects(shape, off):
    G, _, V = shape
    z, t = gtl_inputs(*shape, off)
    ref_loss, ref_dz = hr.gtl(z, t, off, ALPHA)
    loss, dz = hr.gtl(z, t, off, ALPHA, np.float32)
    ok, e_loss, e_dz = hr.loss_verdict(loss, dz, ref_loss, ref_dz, hr.gtl_fixed_point(G, V))
    assert ok and np.isfinite(dz).all()
    # the f32 restatement sits far inside the gate at |z| <= 8: 1e-6 of scale at the most
    assert e_loss <= 1e-6 * ref_loss and e_dz <= 1e-6 * np.abs(ref_dz).max()
    for defect in hr.GTL_DEFECTS:
        if defect == "target_offset ignored" and off == 0:
            continue
        loss, dz = hr.gtl(z, t, off, ALPHA, np.float32, defect)
        assert not hr.loss_verdict(loss, dz, ref_loss, ref_dz, hr.gtl_fixed_point(G, V))[0], defect


def test_gtl_reference_is_the_reference_formula_and_its_derivative():
    """Against the formula of model_fqandtoyo.py:545-550 written out with a one-hot scatter, and a central difference."""
    G, V = 5, 40
    z, t = gtl_inputs(G, 64, V, -1)
    z = z.astype(np.float64)
    cls = t - 1
    loss, dz = hr.gtl(z, t, -1, ALPHA)
    oh = np.zeros((G, V))
    for g in range(G):
        if 0 <= cls[g] < V:
            oh[g, cls[g]] = 1
    assert oh.sum() == 3                                                # rows 1 and 3 match no column
    p = 1 / (1 + np.exp(-z))
    want = (-ALPHA * (1 - p) * oh * np.log(p) - (1 - oh) * p * np.log(1 - p)).mean()
    assert abs(loss - want) <= 1e-15
    for g, c in ((0, 0), (1, 7), (2, V - 1), (4, 3)):
        h = 1e-6
        zp, zm = z.copy(), z.copy()
        zp[g, c] += h
        zm[g, c] -= h
        num = (hr.gtl(zp, t, -1, ALPHA)[0] - hr.gtl(zm, t, -1, ALPHA)[0]) / (2 * h)
        assert abs(num - dz[g, c]) <= 1e-9


def test_cross_entropy_reference_and_its_gate():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    G, V = 9, 300
    z = (rng.standard_normal((G, V)) * 3).astype(np.float32)
    t = rng.integers(1, V, size=G)
    t[::3] = 0
    zr = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    ref = torch.nn.functional.cross_entropy(zr, torch.tensor(t), ignore_index=0)
    ref.backward()
    loss, dz = hr.cross_entropy(z, t, 0)
    assert abs(loss - float(ref.detach())) <= 1e-14 and np.abs(dz - zr.grad.numpy()).max() <= 1e-16
    # the header's rule: out-of-range targets count in the divisor, add nothing, get a zero row
    t2 = t.copy()
    t2[1], t2[2] = -5, V + 3
    loss2, dz2 = hr.cross_entropy(z, t2, 0)
    keep = [g for g in range(G) if t2[g] != 0 and 0 <= t2[g] < V]
    lse = np.log(np.exp(z.astype(np.float64)).sum(1))
    want = sum(lse[g] - z[g, t2[g]] for g in keep) / (len(keep) + 2)
    assert abs(loss2 - want) <= 1e-13 and not dz2[1].any() and not dz2[2].any() and dz2[4].any()
    l32, d32 = hr.cross_entropy(z, t2, 0, np.float32)
    assert abs(l32 - loss2) <= 2e-6 * abs(loss2) + 1e-6 and np.abs(d32 - dz2).max() <= 2e-6 * np.abs(dz2).max() + 1e-9
    for defect in hr.CE_DEFECTS:
        l, d = hr.cross_entropy(z, t2, 0, np.float32, defect)
        assert not (abs(l - loss2) <= 2e-6 * abs(loss2) + 1e-6), defect
        assert not (np.abs(d - dz2).max() <= 2e-6 * np.abs(dz2).max() + 1e-9), defect
    loss3, dz3 = hr.cross_entropy(z, np.zeros(G, dtype=np.int64), 0)
    assert np.isnan(loss3) and not dz3.any()
