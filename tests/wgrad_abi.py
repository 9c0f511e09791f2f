"""The weight-gradient kernels' C ABI (include/mobgt_hip.h: the eight entries of csrc/wgrad.hip, mobgt_layer_wgrad_big with its
_tiles / _splits and mobgt_hop_table_bwd) as plain Python callers over device tensors.  Every leading dimension is an argument of
its own, so a pitch wider than the width is reachable; an operand may be a tensor, a raw address (int: the refusals pass
misaligned ones) or None.  Every caller RETURNS the status code (0 = launched); `_lib.check` is the caller's."""
import ctypes

from mobgt_amd import _lib
from mobgt_amd.ops import _stream

EBADDIM, EALIGN, EDTYPE = (_lib.CONSTANTS["MOBGT_" + n] for n in ("EBADDIM", "EALIGN", "EDTYPE"))
BF16, F32 = _lib.CONSTANTS["MOBGT_BF16"], _lib.CONSTANTS["MOBGT_F32"]
VP, I64, CI, CF = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float


def addr(t):
    if t is None:
        return None
    return t if isinstance(t, int) else t.data_ptr()


def _ptrs(ts):
    return (VP * max(1, len(ts)))(*[addr(t) for t in ts])


def _ints(vs, ty=CI):
    return (ty * max(1, len(vs)))(*vs)


def wgrad(g, ldg, x, ldx, dw, ldw, db, R, M, N, act_dtype):
    return _lib.lib().mobgt_linear_wgrad(addr(g), ldg, addr(x), ldx, addr(dw), ldw, addr(db), R, M, N, act_dtype, _stream())


def wgrad_masked(g, ldg, x, ldx, g_mask, x_mask, mask_vals, g_masked_out, dw, ldw, db, db_of_x, R, M, N):
    return _lib.lib().mobgt_linear_wgrad_masked(addr(g), ldg, addr(x), ldx, addr(g_mask), addr(x_mask), float(mask_vals[0]),
                                                float(mask_vals[1]), float(mask_vals[2]), addr(g_masked_out), addr(dw), ldw,
                                                addr(db), int(db_of_x), R, M, N, _stream())


def wgrad_bias(g, ldg, x, ldx, out_bias, dw, ldw, R, M, N, act_dtype):
    return _lib.lib().mobgt_linear_wgrad_bias(addr(g), ldg, addr(x), ldx, addr(out_bias), addr(dw), ldw, R, M, N, act_dtype,
                                              _stream())


def wgrad_mixed(g_bf16, ldg, x_f32, ldx, dw, ldw, db_x, R, M, N):
    return _lib.lib().mobgt_linear_wgrad_mixed(addr(g_bf16), ldg, addr(x_f32), ldx, addr(dw), ldw, addr(db_x), R, M, N, _stream())


def _group_args(n, g, ldg, x, ldx, dw, ldw, db):
    return (n, _ptrs(g), _ints(ldg, I64), _ptrs(x), _ints(ldx, I64), _ptrs(dw), _ints(ldw, I64), _ptrs(db) if db is not None else None)


def wgrad_group(g, ldg, x, ldx, dw, ldw, db, R, M, N, act_dtype, n=None):
    """Lists of n entries; db: None (a null array) or a list that may hold None entries.  `n` overrides len(g) (the refusals)."""
    n = len(g) if n is None else n
    return _lib.lib().mobgt_linear_wgrad_group(*_group_args(n, g, ldg, x, ldx, dw, ldw, db), R, _ints(M), _ints(N), act_dtype,
                                               _stream())


def backward_tail(g, ldg, x, ldx, dw, ldw, db, R, M, N, act_dtype, a, lda, b_kn, ldb, c, ldc, gM, gN, gK, n=None):
    n = len(g) if n is None else n
    return _lib.lib().mobgt_layer_backward_tail(*_group_args(n, g, ldg, x, ldx, dw, ldw, db), R, _ints(M), _ints(N), act_dtype,
                                                addr(a), lda, addr(b_kn), ldb, addr(c), ldc, gM, gN, gK, _stream())


def _multi_args(n, g, ldg, x, ldx, g_mask, x_mask, mask_vals, dw, ldw, db, db_of_x, R, M, N, in_f32):
    flat = [float(v) for mv in mask_vals for v in mv]
    return (n, _ptrs(g), _ints(ldg, I64), _ptrs(x), _ints(ldx, I64), _ptrs(g_mask), _ptrs(x_mask), _ints(flat or [0.0], CF),
            _ptrs(dw), _ints(ldw, I64), _ptrs(db), _ints([int(v) for v in db_of_x]), _ints(R, I64), _ints(M), _ints(N), _ints(in_f32))


def wgrad_multi(g, ldg, x, ldx, g_mask, x_mask, mask_vals, dw, ldw, db, db_of_x, R, M, N, in_f32, n=None):
    """Lists of n entries (mask_vals: n triples; g_mask / x_mask / db entries may be None)."""
    n = len(g) if n is None else n
    return _lib.lib().mobgt_linear_wgrad_multi(*_multi_args(n, g, ldg, x, ldx, g_mask, x_mask, mask_vals, dw, ldw, db, db_of_x, R,
                                                            M, N, in_f32), _stream())


def wgrad_multi_hop(g, ldg, x, ldx, g_mask, x_mask, mask_vals, dw, ldw, db, db_of_x, R, M, N, in_f32, hop, n=None):
    """hop: None (with_hop = 0) or (d_table, edge_encoder, edge_dis_encoder, d_edge_encoder, d_edge_dis_encoder, D, n_edge, rt)."""
    n = len(g) if n is None else n
    if hop is None:
        tail = (0, None, None, None, None, None, 0, 0, 0)
    else:
        tail = (1,) + tuple(addr(t) for t in hop[:5]) + tuple(int(v) for v in hop[5:])
    return _lib.lib().mobgt_linear_wgrad_multi_hop(*_multi_args(n, g, ldg, x, ldx, g_mask, x_mask, mask_vals, dw, ldw, db, db_of_x,
                                                                R, M, N, in_f32), *tail, _stream())


def hop_table_bwd(d_table, edge_encoder, edge_dis_encoder, d_edge_encoder, d_edge_dis_encoder, D, n_edge, H, rt):
    return _lib.lib().mobgt_hop_table_bwd(addr(d_table), addr(edge_encoder), addr(edge_dis_encoder), addr(d_edge_encoder),
                                          addr(d_edge_dis_encoder), D, n_edge, H, int(rt), _stream())


def wgrad_big(g, ldg, x, ldx, part, colsum, M, N, R, S, n=None):
    """Lists of n entries; colsum: None (a null array) or a list that may hold None entries."""
    n = len(g) if n is None else n
    return _lib.lib().mobgt_layer_wgrad_big(n, _ptrs(g), _ints(ldg, I64), _ptrs(x), _ints(ldx, I64), _ptrs(part),
                                            _ptrs(colsum) if colsum is not None else None, _ints(M), _ints(N), R, S, _stream())


def big_tiles(M, N):
    return _lib.lib().mobgt_layer_wgrad_big_tiles(M, N)


def big_splits(R, ntiles):
    return _lib.lib().mobgt_layer_wgrad_big_splits(R, ntiles)
