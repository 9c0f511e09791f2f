"""mobgt_amd/layer_plan.py: which launches a fused encoder layer takes, enumerated over the whole grid of variants, dtypes, row
counts, widths, supplied operands and forms -- no GPU, no tensors.  The rules are restated here from the description of the layer
(own GEMMs, the two chain bodies, the norm inside the QKV GEMM, the backward chain's entry points, what leaves the layer), not
read back from the functions under test."""
import itertools

import pytest

from mobgt_amd import forms
from mobgt_amd.layer_plan import (BACKWARD_FORMS, FORWARD_FORMS, BackwardPlan, Given, LayerPlan, Operands, Tail, plan_backward,
                                  plan_forward)

ROWS = (16, 608, 4096, 4097, 12560)
WIDTHS = ((128, 1024), (192, 1024), (256, 1024), (160, 1024), (192, 512))
CHAIN_WIDTHS = WIDTHS[:3]
FLIPS = ("chain", "chain_big", "chain_bwd", "ln_gemm", "ln_gemm_bwd", "own_gemm", "tail", "defer_tail", "wgrad_big", "stock_ln_qkv")
DEFAULTS = {row.name: row.default for row in forms.table() if row.name in FLIPS}
FORM_SETS = [dict(DEFAULTS)] + [dict(DEFAULTS, **{name: not DEFAULTS[name]}) for name in FLIPS]


def operands(bf16, R, C, F):
    """Aligned, contiguous operands: ops.layer_gemm_ok takes bf16 up to 4 096 rows; csrc/wgrad.hip takes bf16 gradients of up
    to 131 072 outputs, or any at up to 4 096 rows."""
    gemm = bf16 and R <= 4096
    return Operands(gemm_qkv=gemm, gemm_w1=gemm, chain=True, ln_qkv=True, ln_ffn=True, packed_t=True,
                    wgrad_hip=bf16 and (C * F <= 131072 or R <= 4096))


def forward_grid():
    for variant, bf16, R, (C, F), packed, n_t, need_bwd, from_layer, qkv_pre, on in itertools.product(
            ("fq", "stock"), (False, True), ROWS, WIDTHS, (True, False), (0, 3, 4), (True, False), (True, False), (True, False), FORM_SETS):
        given = Given(xa_pre=qkv_pre, qkv_pre=qkv_pre, nx=True, packed=packed, n_packed_t=n_t, next_qkv=True, next_norm=True,
                      from_layer=from_layer)
        yield variant, bf16, R, C, F, need_bwd, given, operands(bf16, R, C, F), on


def run_forward(case):
    variant, bf16, R, C, F, need_bwd, given, ok, on = case
    return plan_forward(variant, bf16, R, C, F, need_bwd, given, ok, {k: on[k] for k in FORWARD_FORMS})


def test_the_forward_rules_over_the_whole_grid():
    n = 0
    bodies = set()
    for case in forward_grid():
        variant, bf16, R, C, F, need_bwd, given, ok, on = case
        plan = run_forward(case)
        n += 1
        bodies.add((variant, plan.body))
        stock = variant == "stock"
        own = on["own_gemm"] and ok.gemm_qkv and ok.gemm_w1 and C % 32 == 0 and F % 32 == 0
        chain_ok = on["chain"] and (C, F) in CHAIN_WIDTHS
        assert plan.own == own, case
        # the bodies
        fq_chain = not stock and bf16 and given.packed and (own or (R > 4096 and on["chain_big"])) and chain_ok
        preln = (stock and bf16 and own and given.packed and (not need_bwd or (on["chain_bwd"] and given.n_packed_t == 4)) and ok.wgrad_hip
                 and chain_ok)
        assert plan.body == ("chain" if fq_chain else "preln_chain" if preln else "launches"), case
        if plan.body != "launches":
            assert bf16 and (C, F) in CHAIN_WIDTHS and on["chain"]
        assert not (stock and plan.body == "chain") and not (not stock and plan.body == "preln_chain")
        # the backward chain and hosting
        chain_bwd = fq_chain and on["chain_bwd"] and given.n_packed_t >= 3 and (R <= 4096 or on["chain_big"])
        assert plan.chain_bwd == bool(chain_bwd), case
        assert plan.below_hosts == bool(given.from_layer and given.qkv_pre and chain_bwd and given.n_packed_t == 4), case
        assert not plan.chain_bwd or plan.body == "chain"
        assert not plan.below_hosts or plan.chain_bwd
        # where qkv comes from, and the input norm
        norm_in_gemm = (stock and bf16 and not given.qkv_pre and on["own_gemm"] and ok.gemm_qkv and on["ln_gemm"] and C % 32 == 0
                        and C <= 256 and on["stock_ln_qkv"])
        want = "pre" if (given.qkv_pre and not stock) else "ln_gemm" if norm_in_gemm else "own" if own else "torch"
        assert plan.qkv == want, case
        assert plan.norm_launch == (stock and not norm_in_gemm), case
        assert plan.ln_gemm == bool(plan.body == "launches" and own and on["ln_gemm"] and C % 32 == 0 and C <= 256), case
        assert plan.chain_next == (plan.body != "launches") and not plan.chained_in
        assert plan.db1_in_wgrad == ok.wgrad_hip
        # a plan holds no tensor
        assert isinstance(plan, LayerPlan) and all(type(v) in (str, bool, int) for v in plan), plan
    assert n == 2 * 2 * 5 * 5 * 2 * 3 * 2 * 2 * 2 * 11
    assert bodies == {("fq", "chain"), ("fq", "launches"), ("stock", "preln_chain"), ("stock", "launches")}


def _plan(variant="fq", bf16=True, R=608, C=192, F=1024, need_bwd=True, on=None, **given):
    g = dict(xa_pre=True, qkv_pre=True, nx=True, packed=True, n_packed_t=4, next_qkv=True, next_norm=True, from_layer=True)
    g.update(given)
    return plan_forward(variant, bf16, R, C, F, need_bwd, Given(**g), operands(bf16, R, C, F), dict(DEFAULTS, **(on or {})))


def test_a_chained_input_that_cannot_be_run_raises():
    chained = _plan("stock", C=128, nx=False)
    assert chained.chained_in and chained.body == "preln_chain" and chained.qkv == "pre" and not chained.norm_launch
    for missing in (dict(xa_pre=False), dict(qkv_pre=False)):
        with pytest.raises(RuntimeError, match="a chained input without its normed copy / qkv"):
            _plan("stock", C=128, nx=False, **missing)
    for cannot in (dict(on=dict(chain=False)), dict(bf16=False), dict(C=160), dict(packed=False), dict(n_packed_t=3), dict(R=4097)):
        with pytest.raises(RuntimeError, match="cannot run its chain kernels"):
            _plan("stock", **dict(dict(C=128, nx=False), **cannot))
    assert _plan("stock", C=128, nx=False, n_packed_t=0, need_bwd=False).body == "preln_chain"      # (no backward: no packs needed)
    assert not _plan("stock", C=128, next_norm=False).chain_next and not _plan("fq", next_qkv=False).chain_next


def backward_grid(plan):
    R = plan.R
    tails = (None, Tail("layer", R, True), Tail("layer", R + 16, True), Tail("big", R, False), Tail("preln", R, False))
    for wgrad_on, tail, sinks, small, name in itertools.product((False, True), tails, (True, False), (True, False), (None,) + BACKWARD_FORMS):
        on = {k: DEFAULTS[k] for k in BACKWARD_FORMS}
        if name is not None:
            on[name] = not on[name]
        n_hip = sum(plan.bf16 and (m * n <= 131072 or R <= 4096) for m, n in ((plan.C, plan.F), (plan.F, plan.C), (plan.C, plan.C),
                                                                                (3 * plan.C, plan.C)))
        yield on, wgrad_on, tail, n_hip, sinks, small


def test_the_backward_rules_over_the_whole_grid():
    plans = {run_forward(case) for case in forward_grid()} | {_plan("stock", C=128, nx=False), _plan("stock", C=128, nx=False, next_qkv=False)}
    seen, n = set(), 0
    for plan in plans:
        stock = plan.variant == "stock"
        for on, wgrad_on, tail, n_hip, sinks, small in backward_grid(plan):
            bp = plan_backward(plan, on, wgrad_on, tail, n_hip, sinks, small, True)
            n += 1
            seen.add((bp.entry, bp.wgrads, bp.dx))
            R = plan.R
            assert isinstance(bp, BackwardPlan) and all(v is None or type(v) in (str, bool) for v in bp), bp
            step = stock and wgrad_on and n_hip > 0 and R <= 4096 and sinks
            if plan.body == "preln_chain":
                assert bp.entry == "preln" and not bp.host_items and not bp.db1_colsum and not bp.ln_gemm_bwd
                assert bp.host == (tail is not None and tail.kind == "preln" and tail.R == R and plan.chain_next)
                assert bp.wgrads == ("step" if step else "own") and bp.dx == ("below" if plan.chained_in else "norm")
                continue
            # the fq chain runs when chain_bwd holds and (db1 rides in the weight gradient or R > 4096)
            chain = plan.chain_bwd and (plan.db1_in_wgrad or R > 4096)
            assert (bp.entry is not None) == chain and bp.entry != "preln"
            # a parked tail is hosted only by a layer of the same kind and the same R
            assert bp.host == bool(chain and tail is not None and tail.kind != "preln" and tail.R == R)
            assert bp.host_items == (bp.host and tail.items)
            # the 64-row entry only past 4 096 rows and without hosted items; else 16 rows, + a column sum for db1 outside the wgrad
            if chain:
                assert bp.entry == ("chain64" if R > 4096 and not bp.host_items else "chain16")
            assert bp.db1_colsum == (bp.entry == "chain16" and not plan.db1_in_wgrad)
            assert bp.ln_gemm_bwd == bool(not chain and on["ln_gemm_bwd"] and (plan.ln_gemm if plan.body == "launches" else plan.own))
            big = chain and R > 4096 and on["wgrad_big"] and plan.bf16 and not plan.db1_in_wgrad
            n_batch = 0 if big else n_hip
            may = on["defer_tail"] and plan.below_hosts and not stock and on["tail"]
            defer = may and plan.own and n_batch == 4 and R <= 4096 and small and sinks
            big_defer = may and not defer and R > 4096
            # precedence of what leaves the layer: big_defer, defer, the step's grouped launch (stock), the own launch with the tail
            if big_defer:
                assert bp.dx == "below" and bp.wgrads == ("big" if big else "own")
            elif defer:
                assert (bp.wgrads, bp.dx) == ("below", "below")
            elif step:
                assert (bp.wgrads, bp.dx) == ("step", "norm")
            else:
                assert bp.wgrads == ("big" if big else "own")
                rides = plan.own and not stock and on["tail"] and n_batch > 0 and R <= 1024
                assert bp.dx == ("tail" if rides else "norm" if stock else "addmm_out" if not plan.bf16 else "own_gemm" if plan.own
                                 else "addmm_f32")
    assert n > 10000
    for want in (("chain16", "below", "below"), ("chain64", "big", "below"), ("chain16", "own", "tail"), (None, "step", "norm"),
                 ("preln", "step", "below"), ("preln", "own", "norm"), (None, "own", "addmm_out"), ("chain64", "own", "addmm_f32"),
                 (None, "own", "own_gemm")):
        assert want in seen, want


def test_a_form_read_at_backward_time_changes_only_the_backward_plan():
    plan = _plan("fq", R=608)
    on = {k: DEFAULTS[k] for k in BACKWARD_FORMS}
    args = (False, None, 4, True, True, True)
    assert plan_backward(plan, on, *args) == BackwardPlan("chain16", False, False, False, False, "below", "below")
    assert plan_backward(plan, dict(on, defer_tail=False), *args).dx == "tail"
    assert plan_backward(plan, dict(on, tail=False), *args).dx == "own_gemm"
    forward_only = _plan("fq", R=608, on=dict(chain_bwd=False))
    assert forward_only.body == "chain" and not forward_only.chain_bwd
    assert plan_backward(forward_only, dict(on, ln_gemm_bwd=True), *args) == BackwardPlan(None, False, False, False, True, "own", "tail")
    big = _plan("fq", R=12560, C=256)
    assert big.body == "chain" and not big.own and big.chain_bwd and not big.db1_in_wgrad
    assert plan_backward(big, on, False, Tail("big", 12560, False), 1, False, False, True) == \
        BackwardPlan("chain64", True, False, False, False, "big", "below")
    assert plan_backward(big, dict(on, wgrad_big=False), False, None, 1, False, False, True).wgrads == "own"
    assert plan_backward(big, on, False, None, 1, False, False, False).wgrads == "own"            # (operands past 2 GiB)
