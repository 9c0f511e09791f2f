"""CPU checks of the bitmask GCN matrix's reference side (tests/maskgemm_reference.py): its bit packing is MaskAdj.from_dense01's,
every restatement equals a plain dense float64 expression of modelGNN.py / _DistGcnFn's docstring, the exact family really is
exact, the matrix reaches every dispatch branch, and the verdicts the GPU test uses reject every planted defect."""
import numpy as np
import pytest

import maskgemm_reference as mr

SPECS = mr.matrix_specs()
_CASES = {}


def case_of(spec):
    if spec["id"] not in _CASES:
        _CASES[spec["id"]] = mr.build_case(spec)
    return _CASES[spec["id"]]


def of(entry, family):
    return [s for s in SPECS if s["entry"] == entry and s["family"] == family]


def test_ids_are_unique():
    ids = [s["id"] for s in SPECS]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("P", [1, 31, 32, 33, 127, 128, 129, 1003])
def test_packing_is_from_dense01s(P):
    from mobgt_amd.modelGNN import MaskAdj
    rng = np.random.default_rng(P)
    a = (rng.random((P, P)) < 0.3).astype(np.float64)
    np.fill_diagonal(a, 0)
    assert P < 3 or not np.array_equal(a, a.T)
    mask, mask_t, scale = MaskAdj.from_dense01(a)
    m = (a != 0) | np.eye(P, dtype=bool)
    for want, b in ((mask, m), (mask_t, m.T)):
        got = mr.pack_bits(b)
        assert got.shape == tuple(want.shape) and got.shape[1] % 4 == 0
        assert np.array_equal(got, want.numpy().astype(np.int64).astype(np.uint32) if want.numpy().dtype != np.uint32 else want.numpy())
        k = np.arange(got.shape[1] * 32)
        unpacked = (got[:, k >> 5] >> (k & 31).astype(np.uint32)) & 1
        assert np.array_equal(unpacked[:, :P], b.astype(np.uint32)) and not unpacked[:, P:].any()
    assert np.array_equal(scale.numpy(), (1.0 / (a.sum(1) + 1.0)).astype(np.float32))
    wide = mr.pack_bits(m, words=mask.shape[1] + 4)
    assert np.array_equal(wide[:, :mask.shape[1]], mr.pack_bits(m)) and not wide[:, mask.shape[1]:].any()


def test_bf16_rounding_is_nearest_even():
    import torch
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 100, np.float32([1 + 2 ** -8, 1 + 3 * 2 ** -8, -1 - 2 ** -8, 0.0, 65280.0])])
    want = torch.from_numpy(v).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(mr.bf16_bits(v), want)
    assert mr.bf16_bits(np.float32([1 + 2 ** -8]))[0] == 0x3F80 and mr.bf16_bits(np.float32([1 + 3 * 2 ** -8]))[0] == 0x3F82
    assert mr.bf16_bits(np.float32([1 + 3 * 2 ** -8]), truncate=True)[0] == 0x3F81


def test_family_constants():
    assert mr.dropout_threshold(0.5) == 32768 and mr.inv_keep(0.5) == 2.0
    c = case_of(of("l1", "exact")[0])
    assert c["mask_vals"] == (2.0, 1.0, 0.0) and c["slope"] == 0.5
    from mobgt_amd import ops
    r = case_of(of("l1", "round")[0])
    assert np.allclose(r["mask_vals"], ops.act_mask_values(0.2, 0.3), rtol=1e-6) and r["inv_keep"] == pytest.approx(1 / 0.7, rel=1e-4)


def test_exact_family_is_exact():
    """build_case asserts the 2^24 condition for every exact spec; here also: the same sums in float32 have the same bits."""
    worst = 0.0
    for s in SPECS:
        if s["family"] != "exact":
            continue
        c = case_of(s)
        worst = max(worst, c["_exact_worst"])
        for name, o in mr.restate(c).items():
            assert np.array_equal(o["ref"].astype(np.float32).astype(np.float64), o["ref"]), (s["id"], name)
    assert 2.0 ** 16 < worst < 2.0 ** 24
    c = case_of(next(s for s in of("mask_gemm", "exact") if s["K"] == 2081 and s["N"] == 16))
    x32 = (c["x"] * c["bscale"][:, None]) if c["bscale"] is not None else c["x"]
    acc = c["bits"].astype(np.float32) @ x32                                         # float32 accumulation, another order
    rs = c["rscale"][:, None] if c["rscale"] is not None else np.float32(1)
    out32 = rs * acc + (c["bias"] if c["bias"] is not None else np.float32(0))
    assert out32.dtype == np.float32 and np.array_equal(out32.astype(np.float64), mr.restate(c)["out"]["ref"])


def test_branch_coverage_holds():
    mr.check_coverage(SPECS)
    assert mr.prefetches(2049, 16) and not mr.prefetches(2048, 16) and mr.prefetches(1025, 8) and not mr.prefetches(1024, 8)
    assert mr.wave_slices(2081, 16)[8] == (64, 66) and mr.wave_slices(1000, 16)[7] == (28, 32) and mr.wave_slices(1000, 16)[8] == (32, 32)
    assert mr.sgemm_branch(7856, 16, 304, 0, True) == "splitk" and mr.sgemm_branch(1008, 16, 304, 0, True) == 1
    assert mr.sgemm_branch(4096, 64, 32, 0, True) == 4 and mr.sgemm_branch(300, 64, 64, 0, True) == 1
    assert mr.rows_bwd_lds_bytes(2, 128) == 69632 + 512 + 32 * 5 * 4 and mr.rows_bwd_max_R(2) == 6528


def test_lds_bytes_from_the_library():
    from mobgt_amd import _lib
    _lib.build()
    lib = _lib.lib()
    for ldm, R in ((2, 1), (2, 128), (2, 129), (32, 300), (2, 6528), (2, 6529), (1000, 77)):
        assert lib.mobgt_mask_rows_bwd_lds_bytes(ldm, R) == mr.rows_bwd_lds_bytes(ldm, R)
    assert lib.mobgt_mask_gemm_workspace_bytes(1000, 48) == 48 * 1024 * 2


# ------------------------------------------------------------------------------------------------ restatements against dense float64
def dense(c):
    """The entry's outputs as plain dense float64 expressions of modelGNN.py (GraphConvolution: adj @ (x W) + b, reassociated as
    _DistGcnFn's docstring states; LeakyReLU, dropout as keep / (1 - p')), from operands that are already bf16 values."""
    s, f = c["spec"], np.float64
    e = s["entry"]
    lk = lambda a: np.maximum(a, 0) + float(np.float32(c["slope"])) * np.minimum(a, 0)          # noqa: E731

    def drop(y, R, C):
        if not c.get("drop"):
            return y
        return y * mr.keep_mask(c["seed"] + (c["seed_dev"] or 0), c["salt"], R, C, c["p"]) * c["inv_keep"]
    if e == "mask_gemm":
        x = c["x"].astype(f) * (c["bscale"].astype(f)[:, None] if c["bscale"] is not None else 1.0)
        adj = c["bits"].astype(f) * (c["rscale"].astype(f)[:, None] if c["rscale"] is not None else 1.0)
        return dict(out=adj @ x + (c["bias"].astype(f) if c["bias"] is not None else 0.0))
    if e == "l1":
        adj = c["bits"].astype(f) * c["rscale"].astype(f)[:, None]
        t = adj @ c["y0"].astype(f)
        y = drop(lk(t @ c["w1"].astype(f) + c["b1"].astype(f)), s["M"], mr.GH)
        return dict(t=t, y=y, yt=y.T)
    if e == "rows_fwd":
        adj = (c["bits"].astype(f) * c["rscale"].astype(f)[:, None])[c["rows"]]
        u = adj @ c["y1"].astype(f)
        out = u @ c["w2"].astype(f) + (c["b2"].astype(f) if c["b2"] is not None else 0.0)
        return dict(u=u, total=out)
    if e == "rows_bwd":
        A = c["bits"].astype(f)
        onehot = np.zeros((s["R"], s["P"]))
        onehot[np.arange(s["R"]), c["rows"]] = 1
        dy1 = (onehot @ A).T @ c["gu"].astype(f)                                     # autograd of u = A[rows] y1: A^T (scatter of gu)
        pos, neg, zer = c["mask_vals"]
        y1 = c["y1"]
        m = pos * (y1 > 0) + neg * (y1 < 0) + zer * (y1 == 0)
        return dict(dy1=dy1, dtt=(((dy1 * m) @ c["w1"].astype(f).T) * c["bscale"].astype(f)[:, None]).T)
    if e == "sgemm":
        a = c["a"].astype(f)
        if c["a_mask"] is not None:
            pos, neg, zer = c["mask_vals"]
            am = c["a_mask"]
            a = a * (pos * (am > 0) + neg * (am < 0) + zer * (am == 0))
        kb = s["k_b"] or s["K"]
        b = c["b"].astype(f).T if s["b_is_nk"] else c["b"].astype(f)
        o = a[:, :kb] @ b[:kb] + (c["bias"].astype(f) if c["bias"] is not None else 0.0)
        if s["act"]:
            o = drop(lk(o), s["M"], s["N"])
        out = {} if s["ct"] == "only" else dict(c=o)
        if s["ct"]:
            out["ct"] = (o * (c["ct_scale"].astype(f)[:, None] if c["ct_scale"] is not None else 1.0)).T
        return out
    y = drop(lk(c["x"].astype(f) + (c["bias"].astype(f) if c["bias"] is not None else 0.0)), s["R"], s["C"])
    return dict(y=y, **(dict(y_t=y.T) if s["y_t"] else {}))


@pytest.mark.parametrize("entry", list(mr.APPLIES))
def test_restatement_equals_the_dense_expression(entry):
    """Exact family: every operand is a bf16 value and power-of-two scaling commutes with rounding, so the restatement (which rounds
    where the kernels round) must equal the unrounded dense expression exactly."""
    for s in of(entry, "exact"):
        c = case_of(s)
        ref, want = mr.restate(c), dense(c)
        for name, w in want.items():
            if name == "total":
                p = ref["parts"]["ref"]
                assert np.array_equal(p[0] + p[1] + p[2] + p[3], w), s["id"]
                q = 16
                assert np.array_equal(p[1], c["rscale"].astype(np.float64)[c["rows"]][:, None] *
                                      (c["bits"][c["rows"]].astype(np.float64) @ c["y1"].astype(np.float64))[:, q:2 * q] @ c["w2"].astype(np.float64)[q:2 * q])
            else:
                assert np.array_equal(ref[name]["ref"], w), (s["id"], name)
        if entry == "rows_fwd" and s["rs_rows"]:
            assert np.array_equal(ref["rs_rows"]["ref"], c["rscale"][c["rows"]].astype(np.float64))
        if entry == "mask_gemm":
            K = s["K"]
            assert np.array_equal(ref["work"]["ref"][:, :K], (c["x"].astype(np.float64) * (c["bscale"].astype(np.float64)[:, None] if c["bscale"] is not None else 1.0)).T)
            assert ref["work"]["ref"].shape == (s["N"], mr.roundup(K, 128)) and not ref["work"]["ref"][:, K:].any()


@pytest.mark.parametrize("entry", list(mr.APPLIES))
def test_rounding_restatement_is_close_to_dense_and_inside_its_own_bound(entry):
    """Rounding family: the restatement differs from the unrounded dense expression only by the operand roundings (relative 2^-8
    per term), and the emulation of a correct kernel (the restatement rounded to f32) passes its verdict."""
    for s in of(entry, "round"):
        c = case_of(s)
        ok, ratio = mr.verdict(c, mr.emulate(c))
        assert ok and ratio <= 1.0, (s["id"], ratio)
        ref, want = mr.restate(c), dense(c)
        for name, w in want.items():
            r = ref[name]["ref"] if name != "total" else ref["parts"]["ref"].sum(0)
            scale = max(1.0, float(np.abs(w).max()))
            assert float(np.abs(r - w).max()) <= 2.0 ** -6 * scale, (s["id"], name)


# ------------------------------------------------------------------------------------------------ planted defects
def rejects(mut, family):
    hits = []
    for s in SPECS:
        if s["family"] != family or mut not in mr.APPLIES[s["entry"]]:
            continue
        c = case_of(s)
        if not mr.verdict(c, mr.emulate(c, mut))[0]:
            hits.append(s["id"])
    return hits


def test_a_correct_kernel_passes():
    for s in SPECS:
        c = case_of(s)
        ok, ratio = mr.verdict(c, mr.emulate(c))
        assert ok and (ratio == 0.0 or s["family"] == "round"), (s["id"], ratio)


@pytest.mark.parametrize("mut", [m for m in mr.MUTANTS if m not in mr.ROUNDING_MUTANTS])
def test_exact_family_rejects(mut):
    """... on every entry point the defect can live in."""
    hits = rejects(mut, "exact")
    entries = {e for e, muts in mr.APPLIES.items() if mut in muts}
    assert entries and {h.split("-exact-")[0] for h in hits} == entries, (mut, entries, hits[:5])


@pytest.mark.parametrize("mut", mr.MUTANTS)
def test_rounding_family_rejects(mut):
    hits = rejects(mut, "round")
    entries = {e for e, muts in mr.APPLIES.items() if mut in muts}
    assert entries and {h.split("-round-")[0] for h in hits} == entries, (mut, entries, hits[:5])


def test_integers_cannot_see_a_scale_moved_across_the_rounding():
    """... which is one reason the rounding family exists: a power of two commutes with round-to-nearest-even.  (Truncation IS
    seen by the exact family wherever an output is not a bf16 value: l1's y and the small GEMM's results reach five digits.)"""
    assert not rejects("round_before_scale", "exact")
    assert rejects("truncate", "exact")


def test_every_listed_defect_is_planted_somewhere():
    assert set(m for muts in mr.APPLIES.values() for m in muts) == set(mr.MUTANTS) and len(mr.MUTANTS) == 12
