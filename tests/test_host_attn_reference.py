"""tests/attn_reference.py judged without a GPU: the float64 reference against independently written forms, and -- for every case
of the matrix tests/test_gpu_attn_matrix.py runs -- that the emulation of the kernels' rounding passes `compare` at the case's
tolerance, that the row floor hides at most 10 % of a tensor's rows, and that deliberately wrong references (mutants) do NOT pass.
The last is what shows the tolerances are tight enough to mean something."""
import math

import pytest
import torch
import torch.nn.functional as F

import attn_reference as ar

SPECS = ar.matrix_specs()


def _sdpa(case, q, k, v):
    qh, kh, vh = (ar._heads(t, case.H) for t in (q, k, v))
    return ar._merge(F.scaled_dot_product_attention(qh, kh, vh, attn_mask=case.bias, scale=case.scale))


@pytest.mark.parametrize("T,d,H", [(33, 16, 8), (70, 24, 4), (130, 32, 8)])
def test_reference_agrees_with_sdpa_float64(T, d, H):
    case = ar.make_case(T, d, H)
    ref = ar.case_reference(case)
    q, k, v = (t.clone().requires_grad_(True) for t in (case.q, case.k, case.v))
    b = case.bias.clone().requires_grad_(True)
    c2 = ar.SimpleNamespace(**vars(case))
    c2.bias = b
    out = _sdpa(c2, q, k, v)
    out.backward(case.gy)
    db = b.grad.clone()
    db[torch.isinf(case.bias)] = 0.0
    for name, got in (("out", out.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad), ("dbias", db)):
        err = float((got - ref[name]).abs().max())
        assert err <= 1e-12 * max(1.0, float(ref[name].abs().max())), (name, err)


def test_reference_dropout_is_softmax_times_keep_times_inv_keep():
    case = ar.make_case(65, 24, 4, p_drop=0.5)
    ref = ar.case_reference(case)
    assert abs(1.0 - float(case.keep.mean()) - 0.5) < 0.02 and case.inv_keep == 2.0
    q, k, v = (t.clone().requires_grad_(True) for t in (case.q, case.k, case.v))
    G, T, H, d = case.G, case.T, case.H, case.d
    out = torch.zeros(G, T, H * d, dtype=torch.float64)
    for g in range(G):                                       # the explicit expression, one (graph, head) at a time
        for h in range(H):
            sl = slice(h * d, (h + 1) * d)
            x = (q[g, :, sl] * case.scale) @ k[g, :, sl].t() + case.bias[g, h]
            e = torch.exp(x - x.max(dim=1, keepdim=True).values)
            p = e / e.sum(dim=1, keepdim=True) * case.keep[g, h] * case.inv_keep
            out[g, :, sl] = p @ v[g, :, sl]
    out.backward(case.gy)
    for name, got in (("out", out.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        err = float((got - ref[name]).abs().max())
        assert err <= 1e-12 * max(1.0, float(ref[name].abs().max())), (name, err)


@pytest.mark.parametrize("spec", SPECS, ids=ar.spec_id)
def test_emulation_passes_and_floor_cap_holds(spec):
    case = ar.spec_case(spec)
    tol = ar.spec_tolerances(spec, case)
    ref = ar.case_reference(case)
    emu = ar.case_emulation(case, ar.emu_form(spec["T"], spec["form"]), spec["form"] == "f32acc")
    ar.assert_padding_zero(emu, case)
    rep = ar.compare(emu, ref, tol, case)
    assert not rep["fail"], rep["fail"]                      # (fails where 2 x emulation is above a c5 ceiling and the emulation itself is too)
    for name in tol:
        assert rep[name]["floor_share"] <= ar.FLOOR_SHARE_CAP, (name, rep[name]["floor_share"])
    if case.family == "one_key" and not case.p_drop:
        v0 = ar._heads(case.v, case.H)[0, :, 0]               # graph 0 has ONE valid key: P = 1, out = v[0, 0] per head, exactly
        assert torch.equal(ar._heads(emu["out"], case.H)[0], v0.unsqueeze(1).expand(-1, case.T, -1))
        assert float(ref["dq"][0].abs().max()) == 0.0 and float(ref["dbias"][0].abs().max()) <= 1e-15


def _family_representatives():
    seen, reps = set(), []
    for s in SPECS:
        k = (s["family"], s["T"] > 64, s["form"], s["p_drop"] > 0)
        if s["T"] < 33 or k in seen:
            continue
        seen.add(k)
        reps.append(s)
    return reps


REPS = _family_representatives()


@pytest.mark.parametrize("spec", REPS, ids=ar.spec_id)
def test_mutants_fail(spec):
    """Every family, every backward form, with and without dropout, short (one chunk) and long: each applicable mutant is rejected
    at the tolerance the GPU test uses."""
    case = ar.spec_case(spec)
    tol = ar.spec_tolerances(spec, case)
    ref = ar.case_reference(case)
    n = 0
    for which in ar.MUTANTS:
        m = ar.mutant(case, which)
        if m is None:
            continue
        n += 1
        rep = ar.compare(m, ref, tol, case)
        print(ar.spec_id(spec), which, "worst measured / tolerance %.1f" % ar.worst_ratio(rep, tol))
        assert rep["fail"], which
    assert n >= 3
    assert (ar.mutant(case, "chunk_skipped") is not None) == (max(case.n_real) > (64 if case.T > 64 else 32))
    assert (ar.mutant(case, "keep_transposed") is not None) == (spec["p_drop"] > 0)
    assert (ar.mutant(case, "second_use_overwrites") is not None) == (spec["family"] == "two_use")


DELTA_SPECS = [s for s in SPECS if s["family"] == "common" or (s["family"] == "one_key" and s["p_drop"] > 0)]


@pytest.mark.parametrize("spec", DELTA_SPECS, ids=ar.spec_id)
def test_inconsistent_delta_fails_three_times_over(spec):
    """The two families built for it.  common: a is chosen so (choose_a).  one_key with dropout, two-pass forms: out = v / (1 - p)
    is not a bf16 value, so a delta from the rounded output leaves dS = dO . (O - bf16(O)) where the truth is exactly zero."""
    case = ar.spec_case(spec)
    tol = ar.spec_tolerances(spec, case)
    bad = ar.case_emulation(case, ar.emu_form(spec["T"], spec["form"]), spec["form"] == "f32acc", True)
    rep = ar.compare(bad, ar.case_reference(case), tol, case)
    ratio = ar.worst_ratio(rep, tol)
    print(ar.spec_id(spec), "a", case.key[8], "ratio %.1f" % ratio)
    assert ratio >= 3.0, ratio


def test_metric_sees_one_lost_key_where_whole_tensor_l2_does_not():
    case = ar.make_case(300, 32, 8)
    ref = ar.case_reference(case)
    m = ar.mutant(case, "key_dropped")
    whole = max(float((m[n] - ref[n]).norm() / ref[n].norm()) for n in ("out", "dq", "dv"))
    rows = max(ar.measure(m[n], ref[n], case, n)["row"] for n in ("out", "dq", "dv"))
    assert whole < 1e-2 < rows, (whole, rows)


def test_matrix_covers_what_the_issue_lists():
    ids = [ar.spec_id(s) for s in SPECS]
    assert len(set(ids)) == len(ids)
    plain = {(s["T"], s["d"], s["form"]) for s in SPECS if s["family"] == "plain" and not s["p_drop"]}
    assert plain == {(T, d, f) for T in ar.T_ALL for d in ar.D_ALL for f in ar.forms_for(T)}
    drop = [s for s in SPECS if s["family"] == "plain" and s["p_drop"]]
    pairs = lambda a, b: {(s[a], s[b]) for s in drop}                                    # noqa: E731
    forms = {f for T in ar.T_DROP for f in ar.forms_for(T)}
    assert pairs("T", "form") == {(T, f) for T in ar.T_DROP for f in ar.forms_for(T)}
    assert {(s["T"], s["form"], s["p_drop"]) for s in drop} == {(T, f, p) for T in ar.T_DROP for f in ar.forms_for(T) for p in (0.1, 0.5)}
    assert pairs("T", "d") == {(T, d) for T in ar.T_DROP for d in ar.D_ALL}
    assert pairs("d", "form") == {(d, f) for d in ar.D_ALL for f in forms}
    assert pairs("d", "p_drop") == {(d, p) for d in ar.D_ALL for p in (0.1, 0.5)}
    assert pairs("form", "seed_mode") == {(f, m) for f in forms for m in ("host", "split")}
    assert pairs("d", "seed_mode") == {(d, m) for d in ar.D_ALL for m in ("host", "split")}
    # DROP = true for NW = 1, 2, 4 at every d, both-kernel / one-pass / two-pass
    nw = lambda T: 1 if T <= 32 else (2 if T <= 64 else 4)                                 # noqa: E731
    assert {(nw(s["T"]), s["d"]) for s in drop} == {(n, d) for n in (1, 2, 4) for d in ar.D_ALL}
    assert {(s["d"], s["form"]) for s in drop if s["T"] > 64} == {(d, f) for d in ar.D_ALL for f in ar.forms_for(65)}
    assert {s["seed_mode"] for s in SPECS if s["p_drop"]} == {"host", "split"}
    assert {s["H"] for s in SPECS} == {4, 8} and {s["family"] for s in SPECS} == set(ar.FAMILIES)
    for T in ar.T_ALL:
        n = ar.default_n_real(T, 3)
        assert n[0] == T and (T < 129 or n[2] <= 64 * ((T + 63) // 64 - 1))
    assert math.isclose(ar.TOL_FLOOR, 2.0 ** -12)
