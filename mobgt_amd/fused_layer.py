"""One autograd node per EncoderLayer (graphormer/model.py:479-489, model_fqandtoyo.py:1731-1743).

The reference's layer is ~25 eager kernel launches forward and ~70 backward, almost all
of them tiny at MobGT's sizes (G*T = a few hundred rows).  Here the forward is
    [LN] -> QKV GEMM -> attention -> out GEMM -> dropout+residual+LN -> FFN GEMM -> GELU -> FFN GEMM ->
    dropout+residual[+LN]
i.e. 4 library GEMMs (bias in the epilogue), the HIP attention kernel and 3-4 fused HIP elementwise kernels
(`csrc/layer.hip`); the backward mirrors it with 8 GEMMs, 2 attention kernels and 4-5 fused kernels that also
produce every bias / LayerNorm gradient (column sums accumulated in registers), so no separate reduce,
dropout-mask, cast or accumulate kernels remain.  The residual stream and all statistics are fp32; the
GEMM-facing activations are fp32 or bf16 (`act_dtype`).

WHICH form of each stage runs is decided in layer_plan.py (plan_forward at the top of the forward, plan_backward at the top of
the backward); the functions here allocate what the plan names and launch it.
"""
import ctypes
from collections import namedtuple

import torch

from . import _lib, forms, ops
from .layer_plan import (BACKWARD_FORMS, BIG_R, FORWARD_FORMS, TAIL_MAX_R, Given, Operands, Tail, plan_backward, plan_forward)
from .ops import _p, _stream, _DT
from .step_state import STEP

_M32 = 0xFFFFFFFF
_TAKES_OUT_DTYPE = {}


def _takes_out_dtype(gemm, *operands):
    """Does this torch GEMM (mm / bmm / addmm) take `out_dtype`?  Tried once per function, on the first caller's operands."""
    if gemm not in _TAKES_OUT_DTYPE:
        try:
            gemm(*operands, out_dtype=torch.float32)
            _TAKES_OUT_DTYPE[gemm] = True
        except Exception:
            _TAKES_OUT_DTYPE[gemm] = False
    return _TAKES_OUT_DTYPE[gemm]


def _split_factor(R, tiles):
    """Divisor s of R so that s * tiles fills the chip (>= ~512 workgroups) while each slice keeps K >= 32."""
    want = max(1, (512 + tiles - 1) // tiles)
    best = 1
    for s in range(1, 257):
        if R % s == 0 and R // s >= 32:
            best = s
            if s >= want:
                break
    return best


def _wgrad_hip(dtype, M, N, R):
    """True when the weight gradient of an [M,N] Linear over R rows goes to csrc/wgrad.hip.  Its 32x32 output
    tiles re-read g / x once per tile column / row: with many rows AND more than ~128 k outputs (c5's 768x256
    and 256x1024 at R = 12 560: 48 / 50 us vs 29 us) the library's split-K GEMM with its 64x64+ tiles is the
    faster one; at R <= 4096 the kernel is on par or ahead for the 1024x192 FFN shapes as well (9 vs 10.6 us at
    R = 800, 16.6 vs 17.9 at R = 2432) and saves the reduce launch."""
    return dtype == torch.bfloat16 and M % 2 == 0 and N % 2 == 0 and (M * N <= _WGRAD_HIP_MN or R <= BIG_R)


_WGRAD_HIP_MN = 131072      # outputs up to which long batches stay on csrc/wgrad.hip


def _wgrad_arrays(items):
    """[(g, x, dw, db or None)] -> (n, g, ldg, x, ldx, dw, ldw, db, M, N) as the grouped weight-gradient launches take them."""
    n = len(items)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    return (n, (vp * n)(*[t[0].data_ptr() for t in items]), (i64 * n)(*[t[0].stride(0) for t in items]),
            (vp * n)(*[t[1].data_ptr() for t in items]), (i64 * n)(*[t[1].stride(0) for t in items]),
            (vp * n)(*[t[2].data_ptr() for t in items]), (i64 * n)(*[t[2].shape[1] for t in items]),
            (vp * n)(*[(t[3].data_ptr() if t[3] is not None else None) for t in items]),
            (ci * n)(*[t[0].shape[1] for t in items]), (ci * n)(*[t[1].shape[1] for t in items]))


class _WgradBatch:
    """Collects the weight-gradient problems of one layer's backward and issues those that go to csrc/wgrad.hip as
    ONE grouped launch at the end of that backward (nothing downstream depends on a weight gradient).  Deferring
    further -- one launch for all layers when the autograd engine finishes the pass -- was tried and dropped: the
    engine's AccumulateGrad clones a gradient that anything else still references (here: the pending list), i.e.
    it would copy the buffers before they are filled."""

    def __init__(self):
        self.items = []

    def add(self, g, x, db=None, sink=None):
        """-> the dW tensor (filled when `flush` runs), or an immediately computed one for the library path.
        `sink`: a zero-initialised [M,N] f32 destination (the trainer's flat gradient slice) to accumulate into."""
        if not _wgrad_hip(g.dtype, g.shape[1], x.shape[1], g.shape[0]):
            return _wgrad(g, x, db, sink=sink)
        dw = sink[:] if sink is not None else ops.zeros_f32((g.shape[1], x.shape[1]), g.device)
        self.items.append((g, x, dw, db))
        return dw

    def flush(self, tail=None):
        """One launch for all queued weight gradients; `tail` = (a [M,K] bf16, w [K,N] bf16, c [M,N] f32): c += a @ w rides
        in the same launch (mobgt_layer_backward_tail).  Returns True if the tail was taken along."""
        it = self.items
        if not it:
            return False
        R = it[0][0].shape[0]
        arr = _wgrad_arrays(it)
        group = arr[:8] + (R,) + arr[8:] + (_DT[it[0][0].dtype],)
        self.items = []
        if tail is not None and R <= TAIL_MAX_R:     # (the tail GEMM of mobgt_layer_backward_tail is sized for <= 1024 rows)
            a, w, c = tail
            if (a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and c.dtype == torch.float32 and a.shape[1] % 32 == 0
                    and w.shape[1] % 8 == 0 and a.is_contiguous() and w.is_contiguous() and c.is_contiguous()):
                _lib.call("mobgt_layer_backward_tail", *group, _p(a), a.stride(0), _p(w), w.stride(0), _p(c), c.stride(0),
                          a.shape[0], w.shape[1], a.shape[1], _stream())
                return True
        _lib.call("mobgt_linear_wgrad_group", *group, _stream())
        return False


def _join_step_wgrads(wb):
    """The queued problems join the train step's ONE grouped launch (ops.flush_deferred_wgrads) -- parked as FRESH views of the
    gradient buffers: autograd's AccumulateGrad clones a returned gradient that anything else still references, and the clone --
    taken before the buffers are filled -- would later be copied over them."""
    for g, x, dw, db in wb.items:
        STEP.wgrad_items.append((g, x, None, None, (1.0, 1.0, 1.0), dw[:], db[:] if db is not None else None, False))
    wb.items = []


def _wgrad(g, x, db=None, sink=None):
    """Weight gradient g^T @ x (fp32) of a Linear layer; bf16 operands go to the split-K MFMA kernel
    (csrc/wgrad.hip), which also accumulates the bias gradient g.sum(0) into `db` when given.  `sink` (library path): the
    gradient's destination in the trainer's flat buffer -- the sum over the split-K partial products may be parked for it."""
    if _wgrad_hip(g.dtype, g.shape[1], x.shape[1], g.shape[0]):
        return ops.linear_wgrad(g, x, db=db)[0]
    if db is not None:
        _lib.call("mobgt_colsum", _p(g), _p(db), g.shape[0], g.shape[1], _DT[g.dtype], _stream())
    return _mm_tn_f32(g, x, sink=sink)


def _mm_tn_f32(g, x, sink=None):
    """g^T @ x for row-major g [R,M], x [R,N] with an fp32 result (library path: fp32 operands).
    The output is small and K = R is long, so K is split over a batch axis (strided views, no copies):
    a plain GEMM call maps a 192x192 output onto ONE workgroup and leaves the other 255 CUs idle."""
    R, M = g.shape
    N = x.shape[1]
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    # split only where a plain GEMM call is starved: <= 12 output tiles, or a very long K
    s = _split_factor(R, tiles) if (tiles <= 12 or (R >= 4096 and tiles < 256)) else 1
    if s > 1:
        ga, xa = g.view(s, R // s, M).transpose(1, 2), x.view(s, R // s, N)
        if g.dtype != torch.float32 and _takes_out_dtype(torch.bmm, ga[:1], xa[:1]):
            part = torch.bmm(ga, xa, out_dtype=torch.float32)           # f32 partial sums: no cast launch, no bf16 rounding
            # round 4: inside a train step the sum waits for the end of the backward pass, where all of the step's run as ONE
            # launch into the gradients' sinks (36 `.sum(0)` launches of 5.5 us per S-BIG step)
            parked = ops.defer_partial_sum(part, sink) if sink is not None else None
            return parked if parked is not None else part.sum(0)
        part = torch.bmm(ga, xa)
        return part.float().sum(0) if part.dtype != torch.float32 else part.sum(0)
    if g.dtype == torch.float32:
        return g.t() @ x
    if _takes_out_dtype(torch.mm, g.t(), x):
        return torch.mm(g.t(), x, out_dtype=torch.float32)      # bf16 operands, fp32 accumulate AND fp32 result
    return (g.t() @ x).float()


# (forms "chain_big"; round 4 measured and round 5 removed: the 16-row chain kernels also past 4 096 rows -- S-BIG 9.53 -> 10.93 ms: a 16-row
#  workgroup re-streams the layer's weights from L2 785 times and loses against the library's tiles there)


def _addmm_f32(c, a, b, inplace=False):
    """c (fp32) + a @ b (bf16 operands) with an fp32 result.  `inplace`: c is a scratch buffer of the caller and
    receives the result (beta = 1 GEMM straight onto it; out-of-place, addmm first copies c into a new tensor)."""
    if _takes_out_dtype(torch.addmm, c, a, b):
        if inplace:
            return torch.ops.aten.addmm.dtype_out(c, a, b, torch.float32, out=c)
        return torch.addmm(c, a, b, out_dtype=torch.float32)
    return c + (a @ b).float()


def _k1_fwd(x, y, x1, w, b, z, z32, mean, rstd, R, C, p, seed, seed_dev, salt, act):
    _lib.call("mobgt_dropout_add_ln_fwd", _p(x), _p(y), _p(x1), _p(w), _p(b), _p(z), _p(z32), _p(mean), _p(rstd), R, C,
              p, seed, _p(seed_dev), salt, act, _stream())


# forms "ln_gemm" / "ln_gemm_bwd" (csrc/lngemm.hip).  Measured on the S-FSQ step (608 rows, C = 192), kernel durations inside the replayed graph:
#   forward   dropout_add_ln 4.8 us + FFN-1 GEMM 5.2 us  ->  fused 9.1 us
#   backward  dropout_add_ln' 5.7 us + GEMM 5.7 us       ->  fused 12.9 - 14.4 us (the first column tile of every row block
#             also reduces dgamma / dbeta / dbias and is the last workgroup to finish)
# i.e. the gaps between dependent launches of a replayed graph are ~0.1 us; what a stage costs is its own ramp-up + one
# memory round trip, and fusing two stages saves only the intermediate's round trip.  The forward fusion is on by
# default, the two backward ones only with MOBGT_LN_GEMM_BWD=1 (kept: parity-tested, and the better trade at other sizes).


# ---- what a layer's backward may leave to the backward of the layer BELOW it --------------------------------------------------
# After its attention backward a layer still owes (a) its input gradient dx = dx1 + dqkv Wqkv and (b) four weight gradients: one
# launch of ~9 us that keeps ~530 workgroups busy for a moment.  The next thing on the device is the lower layer's chain_bwd
# launch: 38 workgroups on 38 of 256 compute units for 16 us.  So, when the layer below is a fused layer that will run
# chain_bwd (its forward produced this layer's qkv), this layer returns dx1 as its input gradient, parks (dqkv, Wqkv^T, the
# four problems) under that tensor's address, and the lower layer's chain launch finishes dx per row block in front of its
# first norm and runs the weight gradients as extra workgroups (csrc/chain.hip).  A parked entry that no layer picks up is
# an error, raised when the backward pass ends -- never a silently incomplete gradient.  (forms "defer_tail"; up to
# layer_plan.DEFER_MAX_R rows)
# (STEP.layer_tails, keyed by _pending_key; STEP.tail_check_task; tails of a backward pass that died: STEP.drop_stale_tails)


def _pending_key(t):
    return (ops.graph_task_id(), t.device.index, t.data_ptr())


def _park_tail(dx1, **work):
    """`kind`: "layer" (dx and the four weight gradients), "big" (past 4 096 rows: dx only) or "preln" (dx through the host's norm)."""
    STEP.layer_tails[_pending_key(dx1)] = dict(dx1=dx1[:], **work)
    if STEP.tail_check_task != ops.graph_task_id():
        STEP.tail_check_task = ops.graph_task_id()
        torch.autograd.Variable._execution_engine.queue_callback(_pending_check)


def _take_tail(dout):
    """What the layer above parked under this layer's incoming gradient, or None."""
    if STEP.layer_tails or STEP.tail_check_task is not None:
        STEP.drop_stale_tails(ops.graph_task_id())
    return STEP.layer_tails.pop(_pending_key(dout), None) if STEP.layer_tails else None


def _complete_pending(pend):
    """The parked work as its own launch (what the layer would have issued itself): dx1 += dqkv Wqkv and the four dW."""
    if pend["kind"] == "preln":
        # (a pre-LN layer's tail goes back through a norm whose parameters and statistics only its host holds)
        raise RuntimeError("mobgt fused layer (pre-LN): the parked input gradient of a chained layer found no host "
                           "(was the layer's input used by something else as well?); set MOBGT_NO_DEFER_TAIL=1")
    if pend["kind"] == "big":                             # (past 4 096 rows: the library's GEMM, onto dx1 in place)
        _addmm_f32(pend["dx1"], pend["dqkv"], pend["wqkv"], inplace=True)
        return
    wb = _WgradBatch()
    wb.items = pend["items"]
    if not wb.flush(tail=(pend["dqkv"], pend["wqkv"], pend["dx1"])):
        ops.layer_gemm(pend["dqkv"], pend["wqkv"], None, True, ops.GEMM_ADD, aux_in=pend["dx1"])


def _pending_check():
    """End of a backward pass (autograd engine callback): nothing may still be parked.  If the lower layer's output had a
    second consumer whose gradient reached the engine's input buffer FIRST, the buffer's sum is a new tensor, no layer
    recognises it and the entry is still here: the weight gradients are completed, the input gradient cannot be repaired
    (the sum was taken without dqkv Wqkv) -- hence the error, never a silent result.  (Had dx1 arrived first, the engine
    accumulates in place into it and the hosted product lands on top: correct.)"""
    tid = ops.graph_task_id()
    STEP.tail_check_task = None
    mine = [k for k in STEP.layer_tails if k[0] == tid or tid == -1]
    if mine:
        left = [STEP.layer_tails.pop(k) for k in mine]
        try:
            for pend in left:                    # finish the arithmetic, then say that the protocol was broken
                _complete_pending(pend)
        finally:
            STEP.layer_tails.clear()
        raise RuntimeError("mobgt fused layer: a deferred input gradient was not consumed by the layer below "
                           "(was the layer's input used by something else as well?); set MOBGT_NO_DEFER_TAIL=1")


_CHAIN_WS = {}              # (device index, C, cluster size) -> workspace of the chain kernels' cluster form
_CHAIN_NCL = {}             # (device index, rows) -> the library's cluster size for them: asked once, not per launch


def chain_workspace(dev, C=192, R=None):
    """Hand-over counters + exchange buffers of the cluster form of the chain kernels (include/mobgt_hip.h:
    mobgt_chain_ws_bytes): zeroed once, for ONE stream at a time (the step's compute stream).  One per device AND per launch
    geometry (model width C and the cluster size the library picks for R rows, mobgt_chain_cluster_size): a row block's
    exchange area is addressed as block x members x 16 x C, so launches of different geometry on one workspace would poll
    words another block wrote, and a stale packet whose generation happens to match would be accepted.  Must exist
    before a graph capture starts (an eager warm-up step creates it).  forms "safe_forms" -> None (one-workgroup form)."""
    if forms.on("safe_forms"):
        return None
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    R = 16 if R is None else int(R)                       # (no R: one row block)
    ncl = _CHAIN_NCL.get((idx, R))
    if ncl is None:
        ncl = _CHAIN_NCL[idx, R] = _lib.lib().mobgt_chain_cluster_size(R)
    key = (idx, int(C), ncl)
    ws = _CHAIN_WS.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the chain kernels' workspace must be allocated before graph capture: run one eager step first")
        ws = _CHAIN_WS[key] = torch.zeros(int(_lib.lib().mobgt_chain_ws_bytes()), dtype=torch.uint8, device=dev)
    return ws


def _ln_gemm_fwd(x, y, x1, w, b, z, mean, rstd, R, C, p, seed, seed_dev, salt, weight, bias, epilogue):
    """x1 = x + dropout(y); z = LayerNorm(x1); out = z @ weight.T + bias [-> GELU] in ONE launch (mobgt_ln_gemm_fwd)."""
    N = weight.shape[0]
    out = torch.empty(R, N, dtype=torch.bfloat16, device=x.device)
    aux = torch.empty(R, N, dtype=torch.bfloat16, device=x.device) if epilogue == ops.GEMM_GELU else None
    _lib.call("mobgt_ln_gemm_fwd", _p(x), _p(y), _p(x1), _p(w), _p(b), _p(z), _p(mean), _p(rstd), R, C, p, seed,
              _p(seed_dev), salt, _p(weight), weight.stride(0), _p(bias), _p(out), N, epilogue,
              _p(aux), N, _stream())
    return (out, aux) if aux is not None else out


def _ln_gemm_bwd(dz, dz32, dres, x1, mean, rstd, w, dx1, dy, dgamma, dbeta, dbias, R, C, p, seed, seed_dev, salt, weight_kn,
                 epilogue, aux_in):
    """dx1 = dres + LayerNorm'(dz + dz32); dy = dropout'(dx1); out = dy @ weight_kn [* gelu'(aux_in)] in ONE launch."""
    N = weight_kn.shape[1]
    out = torch.empty(R, N, dtype=torch.bfloat16, device=x1.device)
    _lib.call("mobgt_ln_gemm_bwd", _p(dz), _p(dz32), _p(dres), _p(x1), _p(mean), _p(rstd), _p(w), _p(dx1), _p(dy),
              _p(dgamma), _p(dbeta), _p(dbias), R, C, p, seed, _p(seed_dev), salt, _p(weight_kn),
              weight_kn.stride(0), _p(out), N, epilogue, _p(aux_in), N, _stream())
    return out


def _k1_bwd(dz, dz32, dres, x1, mean, rstd, w, dx1, dy, dgamma, dbeta, dbias, R, C, p, seed, seed_dev, salt, act):
    _lib.call("mobgt_dropout_add_ln_bwd", _p(dz), _p(dz32), _p(dres), _p(x1), _p(mean), _p(rstd), _p(w), _p(dx1), _p(dy),
              _p(dgamma), _p(dbeta), _p(dbias), R, C, p, seed, _p(seed_dev), salt, act,
              _stream())


def _chain_fwd(a, x, packed, sh, n1, norm, nq, outs, stats, plan, cfg):
    """mobgt_layer_chain_fwd, both variants: `norm` = (weight, bias) behind the second residual add (fq: ffn_norm2; pre-LN: the NEXT
    layer's self_attention_norm, or nulls), `nq` = the next layer's (packed Wqkv, bqkv) or nulls, `outs` = (x1, z, u, h, x2, out,
    out_a, qkv_next) with None for what the variant does not produce."""
    p_wo, p_w1, p_w2 = packed
    _lib.call("mobgt_layer_chain_fwd", _p(a), _p(x), _p(p_wo), _p(sh.bo), _p(n1[0]), _p(n1[1]), _p(p_w1), _p(sh.b1), _p(p_w2),
              _p(sh.b2), _p(norm[0]), _p(norm[1]), _p(nq[0]), _p(nq[1]), *[_p(t) for t in outs], _p(stats[2]), _p(stats[3]),
              _p(stats[4]), _p(stats[5]), plan.R, plan.C, plan.F, cfg.p, cfg.seed, _p(cfg.seed_dev), (cfg.salt + 1) & _M32,
              (cfg.salt + 2) & _M32, _p(chain_workspace(x.device, plan.C, plan.R)), _stream())


def _chain_bwd(entry, plan, cfg, sv, dout, norm, sm, pend):
    """One backward chain launch: d(out) -> [norm'] -> dropout' -> (W2, gelu') -> W1 -> ffn_norm' + residual -> dropout' -> Wo.
    `entry`: "chain16" (mobgt_layer_chain_bwd), "chain64" (..._big, past 4 096 rows) or "preln" (..._preln); the three share their
    first 32 arguments.  `norm` = (weight, dweight, dbias) of the norm in front (fq: ffn_norm2; pre-LN: the hosted layer's
    self_attention_norm, or nulls).  `pend`: the tail hosted for the layer above (`dout` holds its dx1): dx1 + dqkv Wqkv is
    finished in front of the first norm and -- 16-row entry -- its weight gradients run as extra workgroups.
    -> (df, du, dy, da, dx1)"""
    R, C, F = plan.R, plan.C, plan.F
    bf = dict(dtype=cfg.act_dtype, device=dout.device)
    df, dy, da = torch.empty(R, C, **bf), torch.empty(R, C, **bf), torch.empty(R, C, **bf)
    du = torch.empty(R, F, **bf)
    dx1 = torch.empty(R, C, dtype=torch.float32, device=dout.device)
    w2t, w1t, wot = cfg.packed_t[:3]
    st = sv.stats
    ptrs = [_p(t) for t in (dout, sv.x2, sv.x1, sv.u, st[2], st[3], st[4], st[5], sv.n1w, norm[0], w2t, w1t, wot, df, du, dy, da, dx1,
                            norm[1], norm[2], sm.db2, sm.dn1w, sm.dn1b, sm.dbo)]
    dims = (R, C, F, cfg.p, cfg.seed, _p(cfg.seed_dev), (cfg.salt + 1) & _M32, (cfg.salt + 2) & _M32)
    tail = (_p(pend["dqkv"]), _p(pend["wqt"])) if pend is not None else (None, None)
    if entry == "chain64":      # b1's gradient is summed inside (db1 is zero-filled); the hosted tail comes without weight gradients
        _lib.call("mobgt_layer_chain_bwd_big", *ptrs, _p(None if plan.db1_in_wgrad else sm.db1), *dims, *tail, _stream())
    else:
        extra = _wgrad_arrays(pend["items"]) if pend is not None and pend["items"] else (0,) + (None,) * 9
        _lib.call("mobgt_layer_chain_bwd_preln" if entry == "preln" else "mobgt_layer_chain_bwd", *ptrs, *dims, *tail, *extra,
                  _p(chain_workspace(dout.device, C, R)), _stream())
    return df, du, dy, da, dx1


class LayerConfig:
    """Per-call constants of one fused layer (not tensors that need gradients)."""

    def __init__(self, variant, num_heads, scale, p_drop, p_att, seed, seed_dev, salt, pack, act_dtype):
        self.variant, self.H, self.scale = variant, num_heads, scale
        self.p, self.p_att = float(p_drop), float(p_att)
        self.seed, self.seed_dev, self.salt = int(seed), seed_dev, int(salt) & 0xFFFFFFFF
        self.pack = pack
        self.act_dtype = act_dtype
        self.from_layer = False   # the layer's input is the output of another fused layer (model.fused_layer_forward) ...
        self.token_host = False   # ... or of the one-launch encoder input, whose backward launch is then the host (forms "l0_token_host")
        self.next_qkv = None      # (packed wqkv, bqkv) of the NEXT fused layer: its QKV projection rides in this layer's chain
        self.packed = None        # (wo, w1, w2) of this layer in MFMA operand order (model.pack_layer_weights)
        self.packed_t = None      # (w2^T, w1^T, wo^T, wqkv^T) likewise, for the backward chain
        self.out_act = self.out_qkv = None
        self.next_norm = None     # pre-LN: (weight, bias) of the NEXT layer's self_attention_norm, applied by this layer's chain
        self.out_preln = False    # ... and this layer's output then carries that layer's normed input + qkv


# the node's parameters (fp32 masters, reference names; nn = the next layer's self_attention_norm, pre-LN only), the layer's shadows,
# what the forward saves (in ctx.save_for_backward's order), the gradient destinations the trainer registered (or None) and the
# block of small gradients
_Params = namedtuple("_Params", "wq bq wk bk wv bv wo bo n1w n1b nxw nxb w1 b1 w2 b2 nnw nnb", defaults=(None, None))
_Shadows = namedtuple("_Shadows", "wqkv bqkv wo bo w1 b1 w2 b2")
_Saved = namedtuple("_Saved", "x xa qkv a lse x1 z u h x2 stats s_wqkv s_wo s_w1 s_w2 n1w nxw nnw")
_Sinks = namedtuple("_Sinks", "qkv wo w1 w2 small nx nn")
_SmallGrads = namedtuple("_SmallGrads", "dbqkv dbo db1 db2 dn1w dn1b dnxw dnxb")


def _aligned(*ts):
    return all(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0) for t in ts)


def _forms_on(names):
    return {name: forms.on(name) for name in names}


def _given(cfg, xa_pre, qkv_pre, p, R, C):
    A, nq = cfg.act_dtype, cfg.next_qkv
    return Given(xa_pre=xa_pre is not None and xa_pre.dtype == A and xa_pre.numel() == R * C,
                 qkv_pre=qkv_pre is not None and qkv_pre.dtype == A and qkv_pre.numel() == 3 * R * C,
                 nx=p.nxw is not None, packed=cfg.packed is not None, n_packed_t=len(cfg.packed_t) if cfg.packed_t is not None else 0,
                 next_qkv=nq is not None and nq[0].dtype == A and tuple(nq[0].shape) == (3 * C, C) and _aligned(nq[0]),
                 next_norm=p.nnw is not None and p.nnw.is_contiguous() and p.nnb is not None, from_layer=bool(cfg.from_layer))


def _operands(cfg, x, xa, sh, p):
    """The one place that looks at the forward's tensors for plan_forward.  Not asked about: tensors the forward allocates itself
    (the attention output going into the chain launch, the out-projection going into the norm + FFN-1 launch) -- fresh, so
    contiguous and aligned.  Every form these predicates guard needs bf16 activations; a group is looked at only where the variant
    and what the caller supplied leave it a reader."""
    if cfg.act_dtype != torch.bfloat16 or xa is None:
        return Operands(False, False, False, False, False, False, False)
    R, C, F = x.shape[0] * x.shape[1], x.shape[2], sh.w1.shape[0]
    stock = cfg.variant == "stock"
    own_norm = () if stock else (p.nxw, p.nxb)                           # (the pre-LN chain applies the NEXT layer's norm, not nx)
    return Operands(gemm_qkv=ops.layer_gemm_ok(xa, sh.wqkv), gemm_w1=ops.layer_gemm_ok(xa, sh.w1),
                    chain=cfg.packed is not None and _aligned(x, sh.bo, sh.b1, sh.b2, p.n1w, p.n1b, *own_norm, *cfg.packed),
                    ln_qkv=stock and _aligned(x, sh.wqkv, sh.bqkv, p.nxw, p.nxb), ln_ffn=_aligned(x, sh.w1, sh.b1, sh.w2, sh.wo),
                    packed_t=cfg.packed_t is not None and _aligned(*cfg.packed_t), wgrad_hip=_wgrad_hip(cfg.act_dtype, F, C, R))


def _input_act(cfg, x, xa_pre, given, R, C):
    """The layer's GEMM-facing input [R, C]: stock -- a buffer its norm fills, or the normed copy the layer below made (None when
    that is missing: plan_forward raises); fq -- x itself (f32), the copy the previous layer's LayerNorm kernel wrote, or a cast."""
    A = cfg.act_dtype
    if cfg.variant == "stock":
        if given.nx:
            return torch.empty(R, C, dtype=A, device=x.device)
        return xa_pre.view(R, C) if given.xa_pre else None
    if A == torch.float32:
        return x.view(R, C)
    return xa_pre.view(R, C) if given.xa_pre else x.view(R, C).to(A)


def _find_sinks(plan, p, C):
    """Destinations in the trainer's flat buffer, if it registered any."""
    # the four weight gradients (q/k/v are adjacent there exactly when they are adjacent in the fused [3C, C] parameter storage)
    sq, sk, sv = ops.grad_sink(p.wq), ops.grad_sink(p.wk), ops.grad_sink(p.wv)
    s_qkv = None
    if sq is not None and sk is not None and sv is not None and sq.is_contiguous() \
            and sk.data_ptr() == sq.data_ptr() + 4 * sq.numel() and sv.data_ptr() == sk.data_ptr() + 4 * sk.numel():
        s_qkv = torch.as_strided(sq, (3 * C, C), (C, 1))
    weights = (s_qkv, ops.grad_sink(p.wo), ops.grad_sink(p.w1), ops.grad_sink(p.w2))
    # the block of small gradients [dbq dbk dbv | dbo | db1 | db2 | dn1w | dn1b | dnxw | dnxb]: one slice of the flat
    # buffer when the trainer laid these parameters out in that order (train.flat_order)
    # (pre-LN chain: the two norm gradients at the end of the block belong to ANOTHER layer when this layer's chain applies its
    #  successor's norm, and do not exist when the layer below applied this layer's: the block is the first eight, the norms'
    #  gradients have destinations of their own)
    preln = plan.body == "preln_chain"
    chain = [ops.grad_sink(t) for t in (p.bq, p.bk, p.bv, p.bo, p.b1, p.b2, p.n1w, p.n1b) + (() if preln else (p.nxw, p.nxb))]
    small = None
    if all(t is not None and t.is_contiguous() for t in chain) and \
            all(chain[j + 1].data_ptr() == chain[j].data_ptr() + 4 * chain[j].numel() for j in range(len(chain) - 1)):
        small = torch.as_strided(chain[0], (sum(t.numel() for t in chain),), (1,))
    nx = (ops.grad_sink(p.nxw), ops.grad_sink(p.nxb)) if preln and p.nxw is not None else (None, None)
    nn = (ops.grad_sink(p.nnw), ops.grad_sink(p.nnb)) if preln and plan.chain_next else (None, None)
    return _Sinks(*weights, small, nx, nn)


def _small_grads(sinks, C, F, n, dev):
    """The first `n` of the layer's small gradients [dbqkv 3C | dbo C | db1 F | db2 C | dn1w C | dn1b C | dnxw C | dnxb C] as
    consecutive views of ONE block: the trainer's slice (train.flat_order lays it out in this order) or a zero-filled buffer."""
    sizes = [3 * C, C, F, C, C, C, C, C][:n]
    block = sinks.small if sinks.small is not None else ops.zeros_f32((sum(sizes),), dev)
    views, o = [], 0
    for size in sizes:
        views.append(block[o:o + size])
        o += size
    return views


def _norm_grads(pair, have, C, dev):
    """(dweight, dbias) of a norm whose gradients have destinations of their own (pre-LN chain), (None, None) without the norm."""
    if not have:
        return None, None
    return tuple(s[:] if s is not None else ops.zeros_f32((C,), dev) for s in pair)


def _forward_chain(plan, cfg, x, a, stats, sh, p):
    """Body "chain" / "preln_chain": everything row-local of the layer -- out-projection ... second residual add [fq: + ffn_norm2] --
    in one launch, + the NEXT layer's QKV projection (pre-LN: its self_attention_norm and projection) when the model named that layer
    (cfg.next_qkv / next_norm)."""
    R, C, F = plan.R, plan.C, plan.F
    stock, nxt = plan.body == "preln_chain", plan.chain_next
    f32, bf = dict(dtype=torch.float32, device=x.device), dict(dtype=cfg.act_dtype, device=x.device)
    x1, x2 = torch.empty(R, C, **f32), torch.empty(R, C, **f32)
    z, u, h = torch.empty(R, C, **bf), torch.empty(R, F, **bf), torch.empty(R, F, **bf)
    out = None if stock else torch.empty(R, C, **f32)              # (pre-LN: the residual stream passes the next layer's norm by)
    out_a = torch.empty(R, C, **bf) if nxt or not stock else None
    qkv_next = torch.empty(R, 3 * C, **bf) if nxt else None
    norm = (p.nxw, p.nxb) if not stock else (p.nnw, p.nnb) if nxt else (None, None)
    _chain_fwd(a, x, cfg.packed, sh, (p.n1w, p.n1b), norm, cfg.next_qkv if nxt else (None, None),
               (x1, z, u, h, x2, out, out_a, qkv_next), stats, plan, cfg)
    if not stock:
        cfg.out_act, cfg.out_qkv = out_a, qkv_next
    elif nxt:
        cfg.out_act, cfg.out_qkv, cfg.out_preln = out_a, qkv_next, True
    return (x2 if stock else out), x1, z, u, h, x2


def _forward_launches(plan, cfg, x, a, stats, sh, p):
    """Body "launches": out-proj ... second LayerNorm as separate launches (every configuration the chain kernel does not cover)."""
    R, C, A, own = plan.R, plan.C, cfg.act_dtype, plan.own
    act = _DT[A]
    seed, sd, salt = cfg.seed, cfg.seed_dev, cfg.salt
    f32 = dict(dtype=torch.float32, device=x.device)
    y = ops.layer_gemm(a.view(R, C), sh.wo, sh.bo) if own else torch.addmm(sh.bo, a.view(R, C), sh.wo.t())
    x1 = torch.empty(R, C, **f32)
    z = torch.empty(R, C, dtype=A, device=x.device)
    if plan.ln_gemm:        # x1 = x + dropout(y), z = LN(x1), u = z W1^T + b1, h = gelu(u): one launch
        u, h = _ln_gemm_fwd(x, y, x1, p.n1w, p.n1b, z, stats[2], stats[3], R, C, cfg.p, seed, sd, salt + 1, sh.w1, sh.b1,
                            ops.GEMM_GELU)
        f = ops.layer_gemm(h, sh.w2, sh.b2)
    elif own:
        _k1_fwd(x, y, x1, p.n1w, p.n1b, z, None, stats[2], stats[3], R, C, cfg.p, seed, sd, salt + 1, act)
        u, h = ops.layer_gemm(z, sh.w1, sh.b1, epilogue=ops.GEMM_GELU)
        f = ops.layer_gemm(h, sh.w2, sh.b2)
    else:
        _k1_fwd(x, y, x1, p.n1w, p.n1b, z, None, stats[2], stats[3], R, C, cfg.p, seed, sd, salt + 1, act)
        u = torch.addmm(sh.b1, z, sh.w1.t())
        h = torch.empty_like(u)
        _lib.call("mobgt_gelu_fwd", _p(u), _p(h), u.numel(), act, _stream())
        f = torch.addmm(sh.b2, h, sh.w2.t())
    x2 = torch.empty(R, C, **f32)
    if plan.variant == "stock":                                   # x = x + dropout(ffn(...))  (model.py:485-488)
        _k1_fwd(x1, f, x2, None, None, None, None, None, None, R, C, cfg.p, seed, sd, salt + 2, act)
        out = x2
    else:                                                         # ... then ffn_norm2 (model_fqandtoyo.py:1742)
        out = torch.empty(R, C, **f32)
        out_a = torch.empty(R, C, dtype=A, device=x.device) if A != torch.float32 else None
        _k1_fwd(x1, f, x2, p.nxw, p.nxb, out_a, out, stats[4], stats[5], R, C, cfg.p, seed, sd, salt + 2, act)
        cfg.out_act = out_a                                       # bf16 copy for the next layer's QKV GEMM
    return out, x1, z, u, h, x2


def _backward_launches(plan, bp, cfg, wb, dout, sv, sm, sinks):
    """d(out) ... d(attention out) as separate launches (every configuration the backward chain does not cover).
    -> (da, dx1, dw2, dw1, dwo)"""
    R, C, F, A, own = plan.R, plan.C, plan.F, cfg.act_dtype, plan.own
    act, dev, st = _DT[A], dout.device, sv.stats
    seed, sd, salt = cfg.seed, cfg.seed_dev, cfg.salt
    db1_in_wgrad = plan.db1_in_wgrad                              # then b1's gradient rides on the dW1 kernel
    df = torch.empty(R, C, dtype=A, device=dev)
    du = None
    if plan.variant == "stock":
        dx2 = dout                                                # grad at x2 = x1 + dropout(f)
        _k1_bwd(None, None, dout, sv.x2, None, None, None, None, df, None, None, sm.db2, R, C, cfg.p, seed, sd, salt + 2, act)
    else:
        dx2 = torch.empty(R, C, dtype=torch.float32, device=dev)  # through ffn_norm2
        if bp.ln_gemm_bwd and db1_in_wgrad:    # ffn_norm2' + dropout' -> df, du = (df W2) * gelu'(u): one launch
            du = _ln_gemm_bwd(None, dout, None, sv.x2, st[4], st[5], sv.nxw, dx2, df, sm.dnxw, sm.dnxb, sm.db2, R, C, cfg.p,
                              seed, sd, salt + 2, sv.s_w2, ops.GEMM_GELU_BWD, sv.u)
        else:
            _k1_bwd(None, dout, None, sv.x2, st[4], st[5], sv.nxw, dx2, df, sm.dnxw, sm.dnxb, sm.db2, R, C, cfg.p, seed, sd,
                    salt + 2, act)
    dw2 = wb.add(df, sv.h, sink=sinks.w2)
    if du is not None:
        pass
    elif own and db1_in_wgrad:
        du = ops.layer_gemm(df, sv.s_w2, None, True, ops.GEMM_GELU_BWD, aux_in=sv.u)      # (df W2) * gelu'(u), one launch
    else:
        dh = df @ sv.s_w2
        du = torch.empty_like(sv.u)
        _lib.call("mobgt_gelu_bwd_colsum", _p(dh), _p(sv.u), _p(du), _p(None if db1_in_wgrad else sm.db1), R, F, act,
                  _stream())
    dz = ops.layer_gemm(du, sv.s_w1, None, True) if own else du @ sv.s_w1
    dw1 = wb.add(du, sv.z, db=sm.db1 if db1_in_wgrad else None, sink=sinks.w1)
    dx1 = torch.empty(R, C, dtype=torch.float32, device=dev)
    dy = torch.empty(R, C, dtype=A, device=dev)
    if bp.ln_gemm_bwd:      # ffn_norm1' + residual + dropout' -> dy, da = dy Wo: one launch
        da = _ln_gemm_bwd(dz, None, dx2, sv.x1, st[2], st[3], sv.n1w, dx1, dy, sm.dn1w, sm.dn1b, sm.dbo, R, C, cfg.p, seed, sd,
                          salt + 1, sv.s_wo, ops.GEMM_BIAS, None)
    else:
        _k1_bwd(dz, None, dx2, sv.x1, st[2], st[3], sv.n1w, dx1, dy, sm.dn1w, sm.dn1b, sm.dbo, R, C, cfg.p, seed, sd, salt + 1, act)
        da = ops.layer_gemm(dy, sv.s_wo, None, True) if own else dy @ sv.s_wo
    dwo = wb.add(dy, sv.a.view(R, C), sink=sinks.wo)
    return da, dx1, dw2, dw1, dwo


def _finish_dx(plan, bp, cfg, sv, sm, dqkv2, dx1, items):
    """The layer's input gradient from dx1 (the gradient at the first residual add) and dqkv, the way the plan names."""
    R, C = plan.R, plan.C
    if bp.dx == "below":
        # nothing more is launched for this layer: the chain launch of the layer below finishes dx = dx1 + dqkv Wqkv in front of its
        # first norm (pre-LN: dx2 = dx1 + norm'(dqkv Wqkv)) and runs the parked weight gradients, if any.  Past 4 096 rows it is the
        # 64-row chain and a 20 us library GEMM otherwise; the weight gradients are the library's there and were issued here.
        kind = "preln" if bp.entry == "preln" else "layer" if bp.wgrads == "below" else "big"
        _park_tail(dx1, dqkv=dqkv2, wqkv=sv.s_wqkv, wqt=cfg.packed_t[3], items=items, R=R, kind=kind)
    elif bp.dx == "norm":                                         # stock: back through self_attention_norm
        dz0 = ops.layer_gemm(dqkv2, sv.s_wqkv, None, True) if plan.own else dqkv2 @ sv.s_wqkv
        dx = torch.empty(R, C, dtype=torch.float32, device=dx1.device)
        _k1_bwd(dz0, None, dx1, sv.x.view(R, C), sv.stats[0], sv.stats[1], sv.nxw, dx, None, sm.dnxw, sm.dnxb, None, R, C, 0.0,
                cfg.seed, cfg.seed_dev, cfg.salt, _DT[cfg.act_dtype])
        return dx
    elif bp.dx == "addmm_out":                                    # dx1 is this function's own buffer: accumulate onto it
        torch.addmm(dx1, dqkv2, sv.s_wqkv, out=dx1)
    elif bp.dx == "own_gemm":
        ops.layer_gemm(dqkv2, sv.s_wqkv, None, True, ops.GEMM_ADD, aux_in=dx1)     # dx1 + dqkv Wqkv, f32, in place
    elif bp.dx == "addmm_f32":
        _addmm_f32(dx1, dqkv2, sv.s_wqkv, inplace=True)
    return dx1                                                    # ("tail": the weight-gradient launch added dqkv Wqkv onto it)


class _FusedLayerFn(torch.autograd.Function):
    """params (fp32 masters, reference names; _Params):
       fq   : wq, bq, wk, bk, wv, bv, wo, bo, n1 = ffn_norm1, nx = ffn_norm2, w1, b1, w2, b2
       stock: wq, bq, wk, bk, wv, bv, wo, bo, n1 = ffn_norm,  nx = self_attention_norm, w1, b1, w2, b2, nn = the next layer's nx
    `shadows`: (wqkv [3C,C], bqkv [3C], wo, bo, w1, b1, w2, b2) in act_dtype (the fused masters when fp32)."""

    @staticmethod
    def forward(ctx, x, token, cfg, shadows, xa_pre, qkv_pre, *params):
        # wq/wk/wv (+ biases) are views of one fused [3C, C] storage (MultiHeadAttention.fuse_qkv_storage); they
        # are separate arguments only so that autograd has an edge to each reference-named parameter.
        p, sh = _Params(*params), _Shadows(*shadows)
        G, T, C = x.shape
        R, F, A = G * T, sh.w1.shape[0], cfg.act_dtype
        x = x.contiguous()
        given = _given(cfg, xa_pre, qkv_pre, p, R, C)
        xa = _input_act(cfg, x, xa_pre, given, R, C)
        plan = plan_forward(cfg.variant, A == torch.bfloat16, R, C, F, any(ctx.needs_input_grad), given, _operands(cfg, x, xa, sh, p),
                            _forms_on(FORWARD_FORMS))
        stats = torch.empty(6, R, dtype=torch.float32, device=x.device)
        seed, sd, salt = cfg.seed, cfg.seed_dev, cfg.salt
        if plan.norm_launch:                                          # y = self_attention_norm(x)  (model.py:480)
            _k1_fwd(x, None, None, p.nxw, p.nxb, xa, None, stats[0], stats[1], R, C, 0.0, seed, sd, salt, _DT[A])
        if plan.qkv == "pre":
            qkv = qkv_pre.view(G, T, 3 * C)                           # written by the previous layer's chain kernel
        elif plan.qkv == "ln_gemm":
            # round 4: xa = self_attention_norm(x) and qkv = xa Wqkv^T + b in ONE launch (csrc/lngemm.hip, no residual input)
            qkv = _ln_gemm_fwd(x, None, None, p.nxw, p.nxb, xa, stats[0], stats[1], R, C, 0.0, seed, sd, salt, sh.wqkv, sh.bqkv,
                               ops.GEMM_BIAS).view(G, T, 3 * C)
        elif plan.qkv == "own":
            qkv = ops.layer_gemm(xa, sh.wqkv, sh.bqkv).view(G, T, 3 * C)
        else:
            qkv = torch.addmm(sh.bqkv, xa, sh.wqkv.t()).view(G, T, 3 * C)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        a, lse = ops._attn_fwd(q, k, v, cfg.pack, cfg.scale, cfg.p_att, seed ^ (salt * 0x9E3779B1), sd)
        cfg.out_qkv = None
        body = _forward_launches if plan.body == "launches" else _forward_chain
        out, x1, z, u, h, x2 = body(plan, cfg, x, a, stats, sh, p)
        ctx.plan, ctx.cfg, ctx.shapes = plan, cfg, (G, T, C)
        ctx.chain_bwd, ctx.stock_chain = plan.chain_bwd, plan.body == "preln_chain"      # (the parity tests read these two off grad_fn)
        ctx.sinks = _find_sinks(plan, p, C)
        ctx.save_for_backward(x, xa, qkv, a, lse, x1, z, u, h, x2, stats, sh.wqkv, sh.wo, sh.w1, sh.w2, p.n1w, p.nxw,
                              p.nnw if plan.chain_next else None)
        return out.view(G, T, C)

    @staticmethod
    def backward(ctx, dout):
        """fq / stock as separate launches or through the fq backward chain; pre-LN chain (model.py:479-489 backwards,
        mobgt_layer_chain_bwd_preln):
            [hosted for the layer above:  t = dqkv_above Wqkv_above;  dx2 = dout + norm_above'(t)]    else dx2 = dout
            df = dropout'(dx2);  du = (df W2) gelu'(u);  dz = du W1;  dx1 = dx2 + ffn_norm'(dz);  dy = dropout'(dx1);  da = dy Wo
        then the attention backward, the four weight gradients and the input gradient, each the way plan_backward names."""
        cfg, plan, sinks = ctx.cfg, ctx.plan, ctx.sinks
        G, T, C = ctx.shapes
        R, F, A, dev = plan.R, plan.F, cfg.act_dtype, dout.device
        sv = _Saved(*ctx.saved_tensors)
        busy = getattr(ctx, "_mobgt_pending", None)     # (model.note_pending_backward: the layer's shadows may be rewritten again)
        if busy is not None:
            busy.done()
        if cfg.token_host and not (STEP.wgrad_on and forms.on("l0_token_host") and forms.on("token_bwd_chain")):
            # (the encoder input's backward is the one launch only inside a train step, and the switches are read now)
            plan = plan._replace(below_hosts=False)
        preln = plan.body == "preln_chain"
        dout = dout.contiguous().view(R, C).float()
        if preln:
            sm = _SmallGrads(*_small_grads(sinks, C, F, 6, dev), *_norm_grads(sinks.nx, sv.nxw is not None, C, dev))
            dnn = _norm_grads(sinks.nn, sv.nnw is not None, C, dev)
        else:
            sm, dnn = _SmallGrads(*_small_grads(sinks, C, F, 8, dev)), (None, None)
        pend = _take_tail(dout)
        # (not asked about: dx1, dqkv and the operands of mobgt_layer_wgrad_big beyond their size -- this pass allocates them itself)
        bp = plan_backward(plan, _forms_on(BACKWARD_FORMS), STEP.wgrad_on,
                           Tail(pend["kind"], pend["R"], bool(pend["items"])) if pend is not None else None,
                           sum(_wgrad_hip(A, m, n, R) for m, n in ((C, F), (F, C), (C, C), (3 * C, C))),
                           all(k is not None for k in sinks[:4]), sinks.small is not None, R * max(3 * C, F) * 2 < (1 << 31))
        if pend is not None and not bp.host:
            _complete_pending(pend)                     # this layer cannot host it: finish it right here, as its own launches
            pend = None
        wb = _WgradBatch()
        if bp.entry is None:
            da, dx1, dw2, dw1, dwo = _backward_launches(plan, bp, cfg, wb, dout, sv, sm, sinks)
        else:
            norm = (sv.nnw,) + dnn if preln else (sv.nxw, sm.dnxw, sm.dnxb)
            df, du, dy, da, dx1 = _chain_bwd(bp.entry, plan, cfg, sv, dout, norm, sm, pend)
            if bp.db1_colsum:
                _lib.call("mobgt_colsum", _p(du), _p(sm.db1), R, F, _DT[A], _stream())
            three = [(df, sv.h, None, sinks.w2), (du, sv.z, sm.db1 if plan.db1_in_wgrad else None, sinks.w1),
                     (dy, sv.a.view(R, C), None, sinks.wo)]
            if bp.wgrads != "big":
                dw2, dw1, dwo = [wb.add(g_, x_, db=db_, sink=k_) for g_, x_, db_, k_ in three]
        dqkv = torch.empty(G, T, 3 * C, dtype=A, device=dev)
        q, k, v = sv.qkv[..., :C], sv.qkv[..., C:2 * C], sv.qkv[..., 2 * C:]
        ops._attn_bwd(q, k, v, sv.a, sv.lse, da.view(G, T, C), dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:], cfg.pack,
                      cfg.scale, cfg.p_att, cfg.seed ^ (cfg.salt * 0x9E3779B1), cfg.seed_dev)
        dqkv2 = dqkv.view(R, 3 * C)
        items = []
        if bp.wgrads == "big":
            # (csrc/wgradbig.hip, round 6; before: three library split-K GEMMs, the grouped kernel for dWo, a column-sum launch)
            four = three + [(dqkv2, sv.xa.view(R, C), sm.dbqkv, sinks.qkv)]
            assert ops.layer_wgrad_big_ok(four)
            dw2, dw1, dwo, dwqkv = ops.layer_wgrad_big(four, R)
        else:
            dwqkv = wb.add(dqkv2, sv.xa, db=sm.dbqkv, sink=sinks.qkv)
        if bp.wgrads == "below":                        # (parked as fresh views: _join_step_wgrads says why)
            items = [(g_, x_, dw_[:], db_[:] if db_ is not None else None) for g_, x_, dw_, db_ in wb.items]
            wb.items = []
        elif bp.wgrads == "step":
            _join_step_wgrads(wb)
        else:
            rode = wb.flush(tail=(dqkv2, sv.s_wqkv, dx1) if bp.dx == "tail" else None)
            assert rode == (bp.dx == "tail")
        dx = _finish_dx(plan, bp, cfg, sv, sm, dqkv2, dx1, items)
        return (dx.view(G, T, C), None, None, None, None, None, dwqkv[:C], sm.dbqkv[:C], dwqkv[C:2 * C], sm.dbqkv[C:2 * C],
                dwqkv[2 * C:], sm.dbqkv[2 * C:], dwo, sm.dbo, sm.dn1w, sm.dn1b, sm.dnxw, sm.dnxb, dw1, sm.db1, dw2, sm.db2) \
            + (dnn if plan.variant == "stock" else ())


def fused_encoder_layer(x, pack, cfg, shadows, params, xa_pre=None, qkv_pre=None):
    cfg.out_act = cfg.out_qkv = None
    cfg.out_preln = False
    out = _FusedLayerFn.apply(x, pack.token, cfg, shadows, xa_pre, qkv_pre, *params)
    if cfg.out_preln:
        out._mobgt_preln = True               # pre-LN: `_mobgt_act` is the NEXT layer's normed input (model.fused_layer_forward)
    if cfg.out_act is not None:
        out._mobgt_act = cfg.out_act          # picked up by the next fused layer (same Python tensor object)
    if cfg.out_qkv is not None:
        out._mobgt_qkv = cfg.out_qkv          # ... and its QKV projection, already computed by this layer's chain kernel
        out._mobgt_from_layer = True          # (the consumer's backward may leave its tail to this layer's: STEP.layer_tails)
    return out
