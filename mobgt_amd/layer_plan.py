"""Which launches one fused encoder layer takes (fused_layer.py runs them): decided in two pure functions from plain values, so
that every combination can be enumerated without a GPU (tests/test_host_layer_plan.py).  `plan_forward` is filled at the top of the
layer's forward, `plan_backward` at the top of its backward; a form is read -- by the caller, into `on` -- at the moment the pass
that uses it starts, so switching forms between a forward and its backward acts as it always did.
Of the package it imports only _lib and _tokhost, for the constants of the libraries' headers: like forms.py it needs no torch, and no built
library."""
from collections import namedtuple

from . import _lib, _tokhost

CHAIN_SHAPES = ((128, 1024), (192, 1024), (256, 1024))     # (C, F) the chain kernels are instantiated for (csrc/chain.hip)
BIG_R = _lib.CONSTANTS["MOBGT_CHAIN_BIG_ROWS"]     # rows past which the library's tiles / the 64-row chain kernels take a layer's products
TAIL_MAX_R = 1024        # rows up to which the tail GEMM of mobgt_layer_backward_tail is sized
DEFER_MAX_R = 4096       # S-GOW: 1024 / 2048 / 4096 / 16384 -> 18.96 / 19.33 / 19.65 / 19.5 k check-ins/s
# rows up to which the encoder input's backward launch hosts the FIRST layer's tail (forms "l0_token_host"; model.fused_layer_forward
# then names that launch as the layer's host through Given.from_layer, and the rules below are those of any hosted layer)
TOKEN_HOST_MAX_R = _tokhost.MAX_ROWS

FORWARD_FORMS = ("own_gemm", "ln_gemm", "stock_ln_qkv", "chain", "chain_big", "chain_bwd")
BACKWARD_FORMS = ("ln_gemm_bwd", "wgrad_big", "defer_tail", "tail")

# what the caller handed to the layer, as booleans (`n_packed_t`: entries of cfg.packed_t, 0 without one)
#   xa_pre / qkv_pre: usable (dtype and size fit);  nx: the variant's other norm is the layer's own (stock: None = chained input)
#   next_qkv / next_norm: the next layer's packed projection / its norm are valid operands of this layer's chain launch
Given = namedtuple("Given", "xa_pre qkv_pre nx packed n_packed_t next_qkv next_norm from_layer")
# what the kernels ask of their operands (fused_layer._operands looks at the tensors)
#   gemm_qkv / gemm_w1: ops.layer_gemm_ok of the activation with Wqkv / W1;  chain, ln_qkv, ln_ffn, packed_t: the operand groups of
#   the chain launch, the norm + QKV launch, the norm + FFN-1 launch and the backward chain are contiguous and 16-byte aligned
#   wgrad_hip: dW1 goes to csrc/wgrad.hip (then b1's gradient rides on that kernel)
Operands = namedtuple("Operands", "gemm_qkv gemm_w1 chain ln_qkv ln_ffn packed_t wgrad_hip")

# qkv: "pre" (the layer below computed it) | "ln_gemm" (norm + projection in one launch) | "own" | "torch"
# norm_launch: the input norm is a launch of its own;  own: the layer's GEMMs run on csrc/gemm.hip
# body: "chain" (fq) | "preln_chain" (stock) | "launches";  ln_gemm: the separate-launch body fuses norm 1 into the FFN-1 GEMM
# chain_next: the chain launch also projects (stock: norms and projects) the next layer's input
# chain_bwd: the fq backward chain may run;  below_hosts: the layer below can host this layer's tail;  chained_in: stock, no own norm
LayerPlan = namedtuple("LayerPlan", "variant bf16 R C F qkv norm_launch own body ln_gemm chain_next chain_bwd below_hosts chained_in "
                                    "db1_in_wgrad")
# a parked tail found under the incoming gradient: kind "layer" | "big" | "preln", its rows, whether it carries weight-gradient items
Tail = namedtuple("Tail", "kind R items")
# entry: "chain16" | "chain64" | "preln" | None (separate launches);  host / host_items: the parked tail rides in the chain launch,
# with its weight-gradient items;  db1_colsum: b1's gradient is a column-sum launch behind the 16-row chain
# ln_gemm_bwd: the separate launches fuse the norms' backward into the GEMMs behind them
# wgrads: "big" (one mobgt_layer_wgrad_big launch) | "below" (parked for the layer below) | "step" (the step's grouped launch) | "own"
# dx: "below" (parked) | "tail" (rides in the own grouped launch) | "norm" (stock: back through self_attention_norm)
#     | "addmm_out" (f32) | "own_gemm" | "addmm_f32"
BackwardPlan = namedtuple("BackwardPlan", "entry host host_items db1_colsum ln_gemm_bwd wgrads dx")


def plan_forward(variant, bf16, R, C, F, need_bwd, given, ok, on):
    """-> LayerPlan.  `on`: {form: bool} over FORWARD_FORMS.  Raises for a chained input (stock, no own norm) that cannot be run."""
    stock = variant == "stock"
    # pre-LN, input normed and projected by the chain launch of the layer below (model.fused_layer_forward: no own norm)
    chained_in = stock and not given.nx
    if chained_in and not (given.xa_pre and given.qkv_pre):
        raise RuntimeError("mobgt fused layer (pre-LN): a chained input without its normed copy / qkv")
    # bf16 configuration at MobGT's sizes: the split-K MFMA kernel of csrc/gemm.hip (GELU fused after FFN layer 1); otherwise the library
    own = bool(on["own_gemm"] and ok.gemm_qkv and ok.gemm_w1 and C % 32 == 0 and F % 32 == 0)
    ln_fits = on["ln_gemm"] and C % 32 == 0 and C <= 256          # csrc/lngemm.hip: model width a multiple of 32 up to 256
    if given.qkv_pre and (not stock or chained_in):
        qkv = "pre"
    elif (stock and bf16 and not given.qkv_pre and on["own_gemm"] and ok.gemm_qkv and ln_fits and ok.ln_qkv and on["stock_ln_qkv"]):
        qkv = "ln_gemm"       # (the first layer of a stack: norm + QKV projection as one launch when the own-GEMM path takes the layer)
    else:
        qkv = "own" if own else "torch"
    chain_fits = bool(bf16 and given.packed and on["chain"] and (C, F) in CHAIN_SHAPES and ok.chain)
    if stock:
        # pre-LN chain: its backward is the chain's too, so a forward that needs one needs the four transposed packs
        bwd_ok = on["chain_bwd"] and given.n_packed_t > 3 and ok.packed_t
        body = "preln_chain" if (own and chain_fits and (bwd_ok or not need_bwd) and ok.wgrad_hip) else "launches"
        chain_bwd = False
    else:
        # (past 4 096 rows `own` is off -- the library's GEMMs take the layer's products -- but the forward chain has its 64-row
        #  form there: csrc/chain.hip, layer_chain_fwd_big_kernel; both chains are the 64-row kernels then, and the backward hosts the
        #  upper layer's tail only)
        body = "chain" if ((own or (R > BIG_R and on["chain_big"])) and chain_fits) else "launches"
        chain_bwd = bool(body == "chain" and on["chain_bwd"] and given.n_packed_t >= 3 and ok.packed_t and (R <= BIG_R or on["chain_big"]))
    if chained_in and body != "preln_chain":
        raise RuntimeError("mobgt fused layer (pre-LN): the layer below chained into this one, which cannot run its chain kernels")
    return LayerPlan(
        variant=variant, bf16=bool(bf16), R=R, C=C, F=F, qkv=qkv, norm_launch=stock and not chained_in and qkv != "ln_gemm", own=own,
        body=body, ln_gemm=bool(body == "launches" and own and bf16 and ln_fits and ok.ln_ffn),
        chain_next=bool(given.next_qkv and (body == "chain" or (body == "preln_chain" and given.next_norm))), chain_bwd=chain_bwd,
        # the layer below produced this layer's qkv in ITS chain launch and will run chain_bwd: it can host what this layer's
        # backward leaves undone (STEP.layer_tails)
        below_hosts=bool(given.from_layer and given.qkv_pre and chain_bwd and given.n_packed_t > 3),
        chained_in=chained_in, db1_in_wgrad=bool(ok.wgrad_hip))


def plan_backward(plan, on, wgrad_on, tail, n_hip, sinks, small_sink, big_fits):
    """-> BackwardPlan.  `on`: {form: bool} over BACKWARD_FORMS;  `wgrad_on`: a train step records weight gradients (STEP.wgrad_on);
    `tail`: the Tail parked under the incoming gradient, or None;  `n_hip`: how many of the layer's four weight gradients go to
    csrc/wgrad.hip;  `sinks` / `small_sink`: the trainer registered destinations for all four weight gradients / for the block of
    small ones;  `big_fits`: the operands of mobgt_layer_wgrad_big stay below 2 GiB."""
    R, stock = plan.R, plan.variant == "stock"
    # inside a train step nothing downstream reads a weight gradient and all four land in their sinks: they join the step's ONE
    # grouped launch (ops.flush_deferred_wgrads) instead of one 7 us launch per layer
    step = bool(stock and wgrad_on and R <= DEFER_MAX_R and sinks)
    if plan.body == "preln_chain":
        host = bool(tail is not None and tail.kind == "preln" and plan.chain_next and tail.R == R)
        return BackwardPlan("preln", host, False, False, False, "step" if step and n_hip else "own", "below" if plan.chained_in else "norm")
    # (the 64-row backward chain, R > 4096: b1's gradient is a column sum of du behind it -- the weight gradients are the library's)
    chain = plan.chain_bwd and (plan.db1_in_wgrad or R > BIG_R)
    host = bool(chain and tail is not None and tail.kind != "preln" and tail.R == R)
    host_items = bool(host and tail.items)
    entry = None if not chain else "chain64" if (R > BIG_R and not host_items) else "chain16"
    # past 4 096 rows: all four weight gradients of the layer (and dbqkv) as ONE launch behind the attention backward
    big = bool(chain and R > BIG_R and on["wgrad_big"] and plan.bf16 and not plan.db1_in_wgrad and big_fits)
    n_batch = 0 if big else n_hip                       # problems in the layer's own grouped launch
    may_defer = on["defer_tail"] and plan.below_hosts and not stock and on["tail"]
    defer = bool(may_defer and plan.own and n_batch == 4 and R <= DEFER_MAX_R and small_sink and sinks)
    big_defer = bool(not defer and may_defer and R > BIG_R)
    wgrads = "big" if big else "below" if defer else "step" if step and n_batch else "own"
    if defer or big_defer:
        dx = "below"
    elif wgrads == "own" and plan.own and not stock and on["tail"] and n_batch and R <= TAIL_MAX_R:
        dx = "tail"               # fq variant, own GEMMs: dx = dx1 + dqkv Wqkv rides in the weight-gradient launch
    else:
        dx = "norm" if stock else "addmm_out" if not plan.bf16 else "own_gemm" if plan.own else "addmm_f32"
    return BackwardPlan(entry, host, host_items, entry == "chain16" and not plan.db1_in_wgrad,
                        bool(entry is None and on["ln_gemm_bwd"] and (plan.ln_gemm if plan.body == "launches" else plan.own)), wgrads, dx)
