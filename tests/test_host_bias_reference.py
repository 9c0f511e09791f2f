"""tests/bias_reference.py on the host: its two statements of the operation agree, its EXACT builders satisfy their own condition for
every case of the GPU matrix, it agrees with the model oracle (oracle/model_oracle.py: assemble_bias and its autograd), and its
verdicts reject every planted defect while passing the unmutated emulation."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bias_reference as br                                             # noqa: E402
from oracle import model_oracle as mo                                   # noqa: E402

F64 = torch.float64
SMALL = [br.spec(N=9, G=2, D=3, D_in=4, F=2, hop="random", n_edge=40, ragged=True, db="bf16", L=3),
         br.spec(N=33, G=3, D=20, D_in=21, n_rel=600, n_poi=1500, n_edge=40, big_ids=True, ragged=True),
         br.spec(N=12, G=2, D=0, D_in=4, n_poi=0), br.spec(N=12, G=2, H=4, D=21, D_in=21, F=3, hop="random", idx="i64", edge="i64")]
_INPUTS = {}


def inputs(s, family):
    key = br.input_key(s, family)
    if key not in _INPUTS:
        _INPUTS[key] = br.build_inputs(s, family)
    return _INPUTS[key]


def max_db(x):
    return float(torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).max())


@pytest.mark.parametrize("k", range(len(SMALL)))
@pytest.mark.parametrize("family", ["exact", "round"])
def test_numpy_and_index_add_statements_agree(k, family):
    s = br.for_family(SMALL[k], family)
    inp, init = inputs(s, family), br.init_tables(s)
    x, _, _ = br.build_grad(s, inp, family)
    f_t, _ = br.forward(inp, s["D"])
    f_n = br.forward_np(inp, s["D"])
    fin = np.isfinite(f_n)
    assert np.array_equal(fin, torch.isfinite(f_t).numpy())
    np.testing.assert_allclose(f_t.numpy()[fin], f_n[fin], rtol=1e-13, atol=1e-13)
    b_t, b_n = br.backward(inp, x, s["D"], init), br.backward_np(inp, x, s["D"], init)
    for name in ("d_rel", "d_poi", "d_hop", "d_vdist"):
        assert (b_t[name] is None) == (b_n[name] is None), name
        if b_t[name] is not None:
            np.testing.assert_allclose(b_t[name].numpy(), b_n[name], rtol=1e-12, atol=1e-12, err_msg=name)


def test_exact_builders_satisfy_their_condition_for_every_case_of_the_matrix():
    """Forward: asserted inside build_inputs.  Backward: pick_K finds a K whose upper bound on sum |addend| / granule is below 2^24
    in every table -- a case that cannot is a builder bug (an AssertionError here), never a skip."""
    seen = {}
    for cus in (256, 64):
        specs = br.matrix_specs(cus)
        assert len({s["id"] for s in specs}) == len(specs)
        for s0 in specs:
            s = br.for_family(s0, "exact")
            key = br.input_key(s, "exact") + (s["L"], s["special"] == "outlier", s["dir"])
            if key in seen:
                continue
            inp = br.build_inputs(s, "exact")
            if s["dir"] == "bwd":
                K, worst = br.pick_K(s, inp, 2.0 ** 13 * s["L"] / 8 if s["special"] == "outlier" else 0.0)
                assert K >= 1 and all(v < 2 ** 24 for v in worst.values()), (s["id"], K, worst)
                if s["special"] and br.pairs(s) < 2 ** 16:
                    assert br.build_grad(s, inp, "exact")[2] is not None
            seen[key] = True
    forms = {br.form_of(s) for s in br.matrix_specs(256)}
    assert forms == {"fwd/short8", "fwd/short4", "fwd/long", "bwd/mfma8", "bwd/mfma4", "bwd/plain8", "bwd/plain4"}


def _oracle_case(variant, seed):
    rs = np.random.RandomState(seed)
    G, N, H, D, D_in, n_edge, n_rel, n_poi = 3, 11, 8, 3, 5, 12, 30, 17
    T = N + 1
    b = SimpleNamespace()
    ab = np.zeros((G, T, T))
    ab[1, :, 9:] = -np.inf
    ab[2, 4, 5] = -np.inf
    b.attn_bias = torch.from_numpy(ab)
    b.rel_pos = torch.from_numpy(rs.randint(0, n_rel, size=(G, N, N)))
    b.poi_pos = torch.from_numpy(rs.randint(0, n_poi, size=(G, N, N)))
    b.edge_input = torch.from_numpy(rs.randint(0, n_edge, size=(G, N, N, D_in, 2)))
    sd = {"rel_pos_encoder.weight": torch.from_numpy(rs.standard_normal((n_rel, H))),
          "edge_encoder.weight": torch.from_numpy(rs.standard_normal((n_edge, H))),
          "edge_dis_encoder.weight": torch.from_numpy(rs.standard_normal((8 * H * H, 1)) * 0.3),
          "graph_token_virtual_distance.weight": torch.from_numpy(rs.standard_normal((1, H)))}
    if variant == "fq":
        sd["poi_pos_encoder.weight"] = torch.from_numpy(rs.standard_normal((n_poi, H)))
    gb = torch.from_numpy(rs.standard_normal((G, H, T, T)))
    return b, sd, gb, (G, N, H, D, D_in, n_edge)


def _as_inputs(b, sd, hop, poi):
    return dict(attn_bias=b.attn_bias, rel_pos=b.rel_pos, poi_pos=b.poi_pos if poi else None, edge_input=b.edge_input,
                rel_table=sd["rel_pos_encoder.weight"], poi_table=sd["poi_pos_encoder.weight"] if poi else None, hop_table=hop,
                vdist=sd["graph_token_virtual_distance.weight"].reshape(-1))


def test_anchor_to_the_model_oracle_stock():
    """The reference forward equals assemble_bias(..., 'stock') with the hop table built in float64 from edge_encoder and
    edge_dis_encoder; with the chain rule applied to d_hop in float64 its four gradients equal the oracle's autograd gradients
    (padding rows as in test_build_bias_fwd_bwd: row 0 of the index tables receives no gradient)."""
    b, sd, gb, (G, N, H, D, D_in, n_edge) = _oracle_case("stock", 7)
    for t in sd.values():
        t.requires_grad_(True)
    want = mo.assemble_bias(sd, b, H, D, "stock")
    (torch.where(torch.isfinite(want), want, torch.zeros_like(want)) * gb).sum().backward()
    enc, dis = sd["edge_encoder.weight"].detach(), sd["edge_dis_encoder.weight"].detach().reshape(-1, H, H)[:D_in]
    hop = torch.einsum("ek,dkh->deh", enc, dis)                                   # [D_in, n_edge, H]
    inp = _as_inputs(b, {k: v.detach() for k, v in sd.items()}, hop, False)
    s = br.spec(G=G, N=N, H=H, D=D, D_in=D_in, F=2)
    got, mag = br.forward(inp, D)
    ok, worst = br.within(got, want.detach(), br.forward_bound(s, got, mag))
    assert ok, worst
    init = dict(d_rel=torch.zeros(30, H, dtype=F64), d_poi=None, d_hop=torch.zeros(D, n_edge, H, dtype=F64), d_vdist=torch.zeros(H, dtype=F64))
    r = br.backward(inp, gb[None], D, init)
    d_enc = torch.einsum("deh,dkh->ek", r["d_hop"], dis[:D])
    d_enc[0] = 0
    d_dis = torch.einsum("ek,deh->dkh", enc, r["d_hop"])
    w_rel, w_enc = sd["rel_pos_encoder.weight"].grad.clone(), sd["edge_encoder.weight"].grad.clone()
    w_rel[0], w_enc[0] = 0, 0
    w_dis = sd["edge_dis_encoder.weight"].grad.reshape(-1, H, H)
    for name, have, ref in (("rel", r["d_rel"], w_rel), ("edge", d_enc, w_enc), ("dis", d_dis, w_dis[:D]),
                            ("vdist", r["d_vdist"], sd["graph_token_virtual_distance.weight"].grad.reshape(-1))):
        np.testing.assert_allclose(have.numpy(), ref.numpy(), rtol=1e-11, atol=1e-11, err_msg=name)
    assert not bool(w_dis[D:].any())


def test_anchor_to_the_model_oracle_fq_poi_pos():
    """fq variant: its edge term carries fp16 rounding points this kernel never sees (the hop table arrives as f32), so only what
    poi_pos adds is compared: the forward difference between a model with and without the poi table, and d_poi."""
    b, sd, gb, (G, N, H, D, D_in, n_edge) = _oracle_case("fq", 8)
    sd["poi_pos_encoder.weight"].requires_grad_(True)
    with_poi = mo.assemble_bias(sd, b, H, D, "fq")
    (torch.where(torch.isfinite(with_poi), with_poi, torch.zeros_like(with_poi)) * gb).sum().backward()
    zero = dict(sd)
    zero["poi_pos_encoder.weight"] = torch.zeros_like(sd["poi_pos_encoder.weight"])
    without = mo.assemble_bias(zero, b, H, D, "fq")
    hop = torch.zeros(D_in, n_edge, H, dtype=F64)
    det = {k: v.detach() for k, v in sd.items()}
    a, _ = br.forward(_as_inputs(b, det, hop, True), D)
    c, _ = br.forward(_as_inputs(b, det, hop, False), D)
    fin = torch.isfinite(a)
    assert torch.equal(fin, torch.isfinite(with_poi))
    np.testing.assert_allclose((a - c)[fin].numpy(), (with_poi - without).detach()[fin].numpy(), rtol=0, atol=1e-12)
    init = dict(d_rel=torch.zeros(30, H, dtype=F64), d_poi=torch.zeros(17, H, dtype=F64), d_hop=torch.zeros(D, n_edge, H, dtype=F64),
                d_vdist=torch.zeros(H, dtype=F64))
    r = br.backward(_as_inputs(b, det, hop, True), gb[None], D, init)
    want = sd["poi_pos_encoder.weight"].grad.clone()
    want[0] = 0
    np.testing.assert_allclose(r["d_poi"].numpy(), want.numpy(), rtol=1e-11, atol=1e-11)


# ------------------------------------------------------------------------------------------------ mutants
M_BWD = br.spec(N=33, G=3, D=4, D_in=8, F=2, hop="random", n_rel=600, n_poi=1500, n_edge=40, db="bf16", L=13, ragged=True)
M_FWD = dict(br.spec(N=33, G=3, D=4, D_in=8, F=2, hop="random", n_rel=600, n_poi=1500, n_edge=40, out="bf16", ragged=True), dir="fwd")
LARGEST = br.spec(G=16, N=255, D=3, D_in=4, db="bf16", L=2, n_rel=600, n_poi=1500, n_edge=40, big_ids=True, ragged=True, max_div=4)
_BWD = {}


def bwd_case(s, family):
    key = (br.input_key(s, family), s["L"])
    if key not in _BWD:
        inp, init = inputs(s, family), br.init_tables(s)
        x, K, _ = br.build_grad(s, inp, family, poison=False)
        ref = br.backward(inp, x, s["D"], init, stats=family == "round")
        _BWD[key] = (inp, init, x, ref)
    return _BWD[key]


def families(name):
    meant = br.MUTANTS[name][1]
    return ("exact", "round") if meant == "both" else (meant,)


def test_every_named_defect_has_a_mutant():
    assert len(br.MUTANTS) >= 20 and all(m[0] in ("fwd", "bwd", "both") and m[1] in ("exact", "round", "both") and m[2]
                                          for m in br.MUTANTS.values())


@pytest.mark.parametrize("family", ["exact", "round"])
def test_the_unmutated_emulation_passes(family):
    inp, init, x, ref = bwd_case(M_BWD, family)
    ok, worst, why = br.backward_verdict(M_BWD, family, br.emulate_backward(M_BWD, inp, x, init), ref, init, max_db(x))
    assert ok, (why, worst)
    f_ref, mag = br.forward(inp, M_FWD["D"])
    for out in ("f32", "bf16"):
        s = dict(M_FWD, out=out)
        ok, worst, why = br.forward_verdict(s, family, *br.emulate_forward(s, inp), f_ref, mag)
        assert ok, (out, why, worst)


@pytest.mark.parametrize("name", [n for n, m in br.MUTANTS.items() if m[0] in ("fwd", "both")])
def test_forward_mutants_are_rejected(name):
    for family in families(name):
        inp = inputs(M_FWD, family)
        f_ref, mag = br.forward(inp, M_FWD["D"])
        for out in ("f32", "bf16"):
            s = dict(M_FWD, out=out)
            ok, _, _ = br.forward_verdict(s, family, *br.mutant(name, s, inp), f_ref, mag)
            assert not ok, (name, family, out)


@pytest.mark.parametrize("name", [n for n, m in br.MUTANTS.items() if m[0] in ("bwd", "both")])
def test_backward_mutants_are_rejected(name):
    for family in families(name):
        inp, init, x, ref = bwd_case(M_BWD, family)
        ok, _, _ = br.backward_verdict(M_BWD, family, br.mutant(name, M_BWD, inp, x, init), ref, init, max_db(x))
        assert not ok, (name, family)


@pytest.mark.parametrize("name", ["one pair's contribution lost", "one pair counted twice", "zero tail (hop row 0) dropped",
                                  "a key >= the LDS cap dropped"])
def test_mutants_of_the_largest_case_are_rejected_in_the_exact_family(name):
    """2^20 pairs: the heavy rows (padding, hop row 0) sum ~10^5 - 10^6 addends, where a relative gate lets one pair through; the
    EXACT family's bit comparison does not."""
    inp, init, x, ref = bwd_case(LARGEST, "exact")
    ok, _, _ = br.backward_verdict(LARGEST, "exact", br.emulate_backward(LARGEST, inp, x, init), ref)
    assert ok
    ok, _, _ = br.backward_verdict(LARGEST, "exact", br.mutant(name, LARGEST, inp, x, init), ref)
    assert not ok, name
