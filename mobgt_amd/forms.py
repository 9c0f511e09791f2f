"""Which form of a kernel path runs: the one place that decides it.

Every fused path keeps its separate-launch form (the parity tests compare the two; TrainStep.guarded_step falls back to the
wait-free forms after a peer-wait fault).  One row per form below; `on(name)` answers from, in this order, a programmatic
override (`set` / `using`), the row's environment variable read AT CALL TIME, the row's default.  A variable that is set
selects the form's non-default state, so `MOBGT_NO_X=1` turns `x` off and `MOBGT_SAFE_FORMS=1` turns `safe_forms` on.
Unset, "" and "0" mean not set, "1" means set, anything else is an error.

Imports nothing from the package and needs no torch.
"""
import contextlib
import os
from collections import namedtuple

Form = namedtuple("Form", "name env default doc")

_ROWS = (
    Form("safe_forms", "MOBGT_SAFE_FORMS", False, "no launch waits for peer workgroups: one workgroup per row block, the head as "
         "three launches, the GCN layer by layer (what TrainStep.guarded_step switches to before it re-runs a faulted step)"),
    # ---- encoder layer (fused_layer.py; csrc/chain.hip, lngemm.hip, wgradbig.hip)
    Form("chain", "MOBGT_NO_CHAIN", True, "out-proj -> LN -> FFN -> LN -> the next layer's QKV in one launch (off: separate launches)"),
    Form("chain_big", "MOBGT_NO_CHAIN_BIG", True, "past 4 096 rows: the 64-row forward chain (off: the library's GEMMs)"),
    Form("chain_bwd", None, True, "the same chain backwards, d(out) -> d(attention out)"),
    Form("ln_gemm", None, True, "dropout+residual+LN as the prologue of the GEMM that consumes it (off: the two-launch form)"),
    Form("ln_gemm_bwd", "MOBGT_LN_GEMM_BWD", False, "the LayerNorm-prologue GEMMs in the backward as well"),
    Form("own_gemm", None, True, "the layer's GEMMs on csrc/gemm.hip (off: through torch)"),
    Form("tail", None, True, "a layer's input-gradient GEMM rides in its grouped weight-gradient launch"),
    Form("defer_tail", "MOBGT_NO_DEFER_TAIL", True, "a layer leaves dx and its weight gradients to the chain_bwd launch of the layer "
         "below (off: it finishes its own backward)"),
    Form("wgrad_big", None, True, "past 4 096 rows: the layer's weight gradients as one launch"),
    # ---- classifier, encoder input
    Form("skinny_all", "MOBGT_SKINNY_ALL", False, "all three classifier products on csrc/skinny.hip (off: dW / db only)"),
    Form("token_fwd_chain", "MOBGT_NO_TOKEN_FWD_CHAIN", True, "the encoder input's forward as one launch (off: four)"),
    Form("token_bwd_chain", "MOBGT_NO_TOKEN_BWD_CHAIN", True, "the encoder input's backward as one launch, csrc/tokbwd.hip (off: three)"),
    Form("l0_token_host", "MOBGT_NO_L0_TOKEN_HOST", True, "the first encoder layer leaves dx and its weight gradients to the encoder "
         "input's one-launch backward (off: it finishes its own backward); no workgroup waits for another, so safe_forms keeps it"),
    Form("l0_token_host_eager", "MOBGT_L0_TOKEN_HOST_EAGER", False, "l0_token_host outside a graph capture as well (off: only a step "
         "that is being captured defers; an eager step is bound by the host, gains nothing and keeps its launch list)"),
    Form("scatter_burst", "MOBGT_NO_SCATTER_BURST", True, "short batches, fused distance GCN: the encoder input's gradients are scattered "
         "in one burst per position, the distance GCN's compact table written instead of scattered (off: job after job); no workgroup "
         "waits for another, so safe_forms keeps it"),
    Form("scatter_burst_eager", "MOBGT_SCATTER_BURST_EAGER", False, "scatter_burst outside a graph capture as well (off: only a step "
         "that is being captured takes it; an eager step keeps its launch list)"),
    # ---- jobs that ride in another launch (off: a launch of their own)
    Form("dist_gu_ride", "MOBGT_NO_DIST_GU_RIDE", True, "the distance GCN's backward product gu, in the burst scatter's launch (needs "
         "scatter_burst); no workgroup waits for another, so safe_forms keeps it"),
    Form("dist_gu_ride_eager", "MOBGT_DIST_GU_RIDE_EAGER", False, "dist_gu_ride outside a graph capture as well (with scatter_burst_eager)"),
    Form("pack_passenger", "MOBGT_NO_PACK_PASSENGER", True, "the layers' weight pack, in the next front launch"),
    Form("front_passengers", "MOBGT_NO_FRONT_PASSENGERS", True, "hop table forward and node-feature indices, in the category GCN's forward"),
    Form("bias_bwd_passenger", "MOBGT_NO_BIAS_BWD_PASSENGER", True, "short batches: the bias tables' backward, in the category GCN's backward"),
    Form("bias_bwd_beside", None, True, "long batches: the bias tables' backward on a side stream (off: where autograd reaches it)"),
    Form("l0_ride", "MOBGT_NO_L0_RIDE", True, "the distance GCN's first product, in the bias assembly's launch"),
    Form("psum_defer", "MOBGT_NO_PSUM_DEFER", True, "split-K partial sums, in the step's one reduction launch into the gradient sinks"),
    # ---- GCNs (modelGNN.py)
    Form("small_gcn", "MOBGT_NO_SMALL_GCN", True, "the three-layer category GCN as one launch each way (off: layer by layer)"),
    Form("conv_act", "MOBGT_NO_CONV_ACT", True, "bias + LeakyReLU + dropout in the small GEMM's epilogue (off: launch per product)"),
    Form("dist_gcn_fused", "MOBGT_NO_DIST_GCN_FUSED", True, "the distance GCN on the masked-GEMM launches"),
    Form("sp_gather", None, True, "sparse adjacency, transposed product as a gather (off: the atomic scatter)"),
    # ---- stock variant
    Form("stock_front", "MOBGT_NO_STOCK_FRONT", True, "hop table, weight pack and encoder input as one front launch"),
    Form("stock_tail", "MOBGT_NO_STOCK_TAIL", True, "the encoder input's and the wide hop table's backward share one grid at the flush"),
    Form("stock_ln_qkv", "MOBGT_NO_STOCK_LN_QKV", True, "the first layer's norm inside its QKV GEMM"),
    # ---- attention
    Form("attn_one_pass", "MOBGT_ATTN_TWO_PASS", True, "T > 64, bf16: one-pass backward (off: the two deterministic passes)"),
    # ---- data parallel (train.TrainStep)
    Form("ddp_overlap", "MOBGT_DDP_OVERLAP", False, "the backward split into graphs, finished gradient slices all-reduced beside the next"),
    Form("ddp_host_exchange", "MOBGT_DDP_HOST_EXCHANGE", False, "all-reduce issued by the host between backward and optimizer graph"),
    Form("force_comm", "MOBGT_FORCE_COMM", False, "a process group of one rank takes the data-parallel path (tests)"),
)
_BY_NAME = {row.name: row for row in _ROWS}
_OVERRIDES = {}


def _env_set(var):
    v = os.environ.get(var, "")
    if v in ("", "0"):
        return False
    if v == "1":
        return True
    raise ValueError(f"{var}={v!r}: expected unset, '', '0' or '1'")


def on(name):
    row = _BY_NAME[name]
    if name in _OVERRIDES:
        return _OVERRIDES[name]
    if row.env is not None and _env_set(row.env):
        return not row.default
    return row.default


def set(name, value):
    """Override what the environment and the default say; `value=None` removes the override."""
    _BY_NAME[name]
    if value is None:
        _OVERRIDES.pop(name, None)
    else:
        _OVERRIDES[name] = bool(value)


@contextlib.contextmanager
def using(**names):
    """`with forms.using(chain=False, ...)`: overrides for the body; the previous overrides come back on exit."""
    saved = dict(_OVERRIDES)
    try:
        for name, value in names.items():
            set(name, value)
        yield
    finally:
        _OVERRIDES.clear()
        _OVERRIDES.update(saved)


def table():
    return _ROWS
