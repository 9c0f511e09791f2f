"""CPU checks of the one-launch GCN / CSR SpMM matrix's reference side (tests/gcn_reference.py): the restatements equal plain
float64 expressions written another way (torch autograd for the network, edge loops for the sparse products), the exact family
really is exact, the matrix reaches every staging form, and the verdicts the GPU test uses pass the unmutated reference and
reject every planted defect."""
import numpy as np
import pytest
import torch

import gcn_reference as gr

SPECS = gr.matrix_specs()
_CASES = {}


def case_of(spec):
    if spec["id"] not in _CASES:
        _CASES[spec["id"]] = gr.build_case(spec)
    return _CASES[spec["id"]]


def of(family, *entries):
    return [s for s in SPECS if s["entry"] in entries and s["family"] == family]


def test_ids_are_unique_and_the_matrix_reaches_every_form():
    ids = [s["id"] for s in SPECS]
    assert len(set(ids)) == len(ids)
    gr.check_coverage(SPECS)
    assert gr.fwd_form(300, 300) == "early" and gr.fwd_form(300, 400) == "restage" and gr.fwd_form(37, 609) == "restage"
    assert gr.fwd_form(305, 40) == "stream" and gr.chunks(305) == [(0, 304, 304), (304, 1, 16)] and len(gr.chunks(609)) == 3
    assert gr.kterms(17) == 32 + 4 and gr.kterms(609) == 304 + 304 + 16 + 12
    assert {(s["n"], s["K0"]) for s in of("round", "fwd")} == {(17, 303), (304, 304), (300, 300), (305, 40), (609, 320), (300, 400)}


def test_family_constants():
    assert gr.inv_keep(0.5) == 2.0 and gr.family_consts("exact")[1:] == (0.5, 0.5, 2.0)
    assert gr.family_consts("round")[3] == pytest.approx(1 / 0.9, rel=1e-4)


def test_exact_family_is_exact():
    """build_case asserts the 2^24 condition per output; here also: the references are f32 values, zeros and drops occur."""
    worst = 0.0
    for s in of("exact", "fwd", "bwd"):
        c = case_of(s)
        worst = max(worst, c["net"]["_exact_worst"])
        for k, x in c["v"][s["entry"]].items():
            if k != "_stages":
                assert np.array_equal(x[0].astype(np.float32).astype(np.float64), x[0]), (s["id"], k)
        a = c["net"]["a"]
        assert np.count_nonzero(a, axis=1).max() <= 4 and set(np.unique(a)) <= {0.0, 0.5, 1.0}
        assert s["n"] < 3 or not np.array_equal(a, a.T)
    print(f"gcn-exact-worst 2^{np.log2(worst):.1f}")
    assert 2.0 ** 16 < worst < 2.0 ** 24
    # the same sums in float32, in numpy's order, have the same bits
    c = case_of(next(s for s in of("exact", "fwd") if (s["n"], s["K0"], s["drop"]) == (609, 320, 1)))
    n = c["net"]
    h1 = gr.leaky(n["ax"] @ n["ws"][0] + n["ws"][1], np.float32(0.5)).astype(np.float32)
    t = n["a"] @ h1
    assert t.dtype == np.float32 and np.array_equal(t.astype(np.float64), c["v"]["fwd"]["t"][0])


@pytest.mark.parametrize("family", ["exact", "round"])
@pytest.mark.parametrize("shape", [(300, 400), (305, 40), (17, 303)])
@pytest.mark.parametrize("drop", [0, 2])
def test_network_restatement_is_torch_autograd_in_float64(family, shape, drop):
    """graphormer/modelGNN.py:53-74 in torch float64 with the same keep mask: values, and the gradients accumulated onto the
    initial buffers (the rounding family's saved activations are f32 roundings of the float64 ones: a relative 2^-24 apart)."""
    c = case_of(next(s for s in of(family, "bwd") if (s["n"], s["K0"]) == shape and s["drop"] == drop))
    n, v = c["net"], c["v"]
    tt = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))                       # noqa: E731
    ws = [tt(w).requires_grad_(True) for w in n["ws"]]
    ax, a = tt(n["ax"]), tt(n["a"])
    lk = lambda x: torch.nn.functional.leaky_relu(x, float(np.float32(n["slope"])))        # noqa: E731
    h1 = lk(ax @ ws[0] + ws[1])
    h2 = lk(a @ h1 @ ws[2] + ws[3])
    if drop:
        h2 = h2 * tt(v["keep"]) * v["ik"]
    out = a @ h2 @ ws[4] + ws[5]
    out.backward(tt(n["g"]))
    tol = dict(rtol=0, atol=0) if family == "exact" else dict(rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(v["fwd"]["out"][0], out.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(v["fwd"]["h2"][0], h2.detach().numpy(), rtol=1e-12, atol=1e-12)
    for name, w in zip(gr.GRADS, ws):
        scale = float(w.grad.abs().max()) + 1.0
        np.testing.assert_allclose(v["bwd"][name][0], n["init"][name] + w.grad.numpy(), rtol=tol["rtol"], atol=tol["atol"] * scale,
                                   err_msg=name)


def test_keep_mask_is_the_bias_act_sites_host_replay():
    from mobgt_amd import ops
    c = case_of(next(s for s in of("exact", "fwd") if s["n"] == 300 and s["K0"] == 400 and s["drop"] == 2))
    n, v = c["net"], c["v"]
    want = ops.dropout_site_mask(n["seed"] + gr.SEED_DEV, n["salt"], 300, 64, 0.5)
    assert np.array_equal(v["keep"], want) and 0.4 < want.mean() < 0.6
    assert not np.array_equal(want, ops.dropout_site_mask(n["seed"], n["salt"], 300, 64, 0.5))
    assert np.array_equal(v["fwd"]["h2"][0] != 0, want & (v["fwd"]["h2"][0] != 0)) and (v["fwd"]["h2"][0][~want] == 0).all()


@pytest.mark.parametrize("family", ["exact", "round"])
def test_sparse_restatements_are_the_edge_loops(family):
    f = np.float64
    for s in of(family, "csr", "t_rows", "gather"):
        if s["C"] not in (60, 128, 260):
            continue
        c = case_of(s)
        g, C = c["graph"], s["C"]
        ref = gr.restate_spmm(c)
        if s["entry"] == "gather":
            want = np.zeros((c["P"], C))
            for j in range(c["P"]):
                for e in range(g["rowptr"][j], g["rowptr"][j + 1]):
                    for k in range(c["R"]):
                        if c["rows"][k] == g["col"][e]:
                            want[j] += f(g["val"][e]) * c["g"][k].astype(f)
            np.testing.assert_allclose(ref["db"][0], want, rtol=1e-12, atol=1e-12)
            assert (ref["head"][0] == -1).all()
            continue
        rows = c["rows"] if c["rows"] is not None else np.arange(gr.CSR_ROWS)
        if s["entry"] == "csr":
            want = np.zeros((rows.size, C)) + (c["bias"].astype(f) if c["bias"] is not None else 0.0)
            for i, r in enumerate(rows):
                for e in range(g["rowptr"][r], g["rowptr"][r + 1]):
                    want[i] += f(g["val"][e]) * c["b"][g["col"][e]].astype(f)
            np.testing.assert_allclose(ref["out"][0], want, rtol=1e-12, atol=1e-12)
        else:
            want = c["init"].astype(f)
            for i, r in enumerate(rows):
                for e in range(g["rowptr"][r], g["rowptr"][r + 1]):
                    want[g["col"][e]] += f(g["val"][e]) * c["g"][i].astype(f)
            np.testing.assert_allclose(ref["db"][0], want, rtol=1e-12, atol=1e-12)
        assert (g["col"] == gr.CSR_COLS - 1).any() and sorted(set(g["degs"])) == sorted(gr.CSR_DEGS)
    gd = case_of(of(family, "gather")[0])["graph"]["degs"]
    assert list(gd[:6]) == list(gr.GATHER_DEGS)


def test_unmutated_reference_passes_every_verdict():
    for s in SPECS:
        c = case_of(s)
        ok, ratio = gr.verdict(c, gr.emulate(c))
        assert ok and ratio <= 1.0, (s["id"], ratio)


@pytest.mark.parametrize("mut", gr.GCN_MUTANTS + gr.SPMM_MUTANTS)
def test_every_defect_is_rejected(mut):
    """Wherever a defect can show (gr.applies), the verdict of that spec rejects it -- in both families."""
    hit = {"exact": 0, "round": 0}
    for s in SPECS:
        if not gr.applies(s, mut):
            continue
        if s["entry"] in ("fwd", "bwd") and s["n"] > 320 and s["drop"] != 1:
            continue                                    # (the large shapes once: the defects do not depend on the drop variant)
        c = case_of(s)
        ok, _ = gr.verdict(c, gr.emulate(c, mut))
        assert not ok, (s["id"], mut)
        hit[s["family"]] += 1
    assert hit["exact"] and hit["round"], (mut, hit)


def test_the_suspected_defect_shows_only_where_layer_one_streams_through_the_L_area():
    for s in of("exact", "fwd"):
        c = case_of(s)
        same = gr.verdict(c, gr.emulate(c, "stale_L_after_layer1"))[0]
        assert same == (gr.fwd_form(s["n"], s["K0"]) != "restage"), s["id"]
