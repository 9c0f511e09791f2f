"""The bitmask GCN kernels' C ABI (include/mobgt_hip.h: the four entries of csrc/maskgemm.hip with their two size functions,
mobgt_small_gemm_f32_act of csrc/sgemm.hip and mobgt_bias_act_fwd / _fwd_t of csrc/layer.hip) as plain Python callers over device
tensors.  Every leading dimension is an argument of its own, so a pitch wider than the width is reachable; an operand may be a
tensor, a raw address (int: the refusals pass misaligned ones) or None.  Every caller RETURNS the status code (0 = launched);
`_lib.check` is the caller's."""
from mobgt_amd import _lib
from mobgt_amd.ops import _stream

EBADDIM, EALIGN, EDTYPE = (_lib.CONSTANTS["MOBGT_" + n] for n in ("EBADDIM", "EALIGN", "EDTYPE"))
BF16, F32 = _lib.CONSTANTS["MOBGT_BF16"], _lib.CONSTANTS["MOBGT_F32"]


def addr(t):
    if t is None:
        return None
    return t if isinstance(t, int) else t.data_ptr()


def workspace_bytes(K, N):
    return int(_lib.lib().mobgt_mask_gemm_workspace_bytes(K, N))


def rows_bwd_lds_bytes(ld_mask_words, R):
    return int(_lib.lib().mobgt_mask_rows_bwd_lds_bytes(ld_mask_words, R))


def mask_gemm(mask, ld_mask_words, x, ldx, bscale, rscale, bias, out, ld_out, work, M, K, N):
    return _lib.lib().mobgt_mask_gemm(addr(mask), ld_mask_words, addr(x), ldx, addr(bscale), addr(rscale), addr(bias), addr(out),
                                      ld_out, addr(work), M, K, N, _stream())


def l1_fwd(mask, ld_mask_words, rscale, y0t, ld_y0t, t, w1, b1, slope, dropout_p, seed, seed_dev, salt, y, yt, ld_yt, zero,
           zero_floats, M, K):
    return _lib.lib().mobgt_mask_gemm_l1_fwd(addr(mask), ld_mask_words, addr(rscale), addr(y0t), ld_y0t, addr(t), addr(w1), addr(b1),
                                             float(slope), float(dropout_p), int(seed), addr(seed_dev), int(salt) & 0xFFFFFFFF,
                                             addr(y), addr(yt), ld_yt, addr(zero), zero_floats, M, K, _stream())


def rows_fwd(mask, ld_mask_words, rows, rscale, y1t, ld_y1t, w2, b2, u, parts, rs_rows, R, K, NO):
    return _lib.lib().mobgt_mask_rows_fwd(addr(mask), ld_mask_words, addr(rows), addr(rscale), addr(y1t), ld_y1t, addr(w2), addr(b2),
                                          addr(u), addr(parts), addr(rs_rows), R, K, NO, _stream())


def rows_bwd(mask_t, ld_mask_words, rows, gut, ld_gut, y1, mask_vals, w1, bscale, dy1, dtt, ld_dtt, R, P):
    return _lib.lib().mobgt_mask_rows_bwd(addr(mask_t), ld_mask_words, addr(rows), addr(gut), ld_gut, addr(y1), float(mask_vals[0]),
                                          float(mask_vals[1]), float(mask_vals[2]), addr(w1), addr(bscale), addr(dy1), addr(dtt),
                                          ld_dtt, R, P, _stream())


def small_gemm_act(a, lda, a_mask, mask_vals, b, ldb, b_is_nk, bias, leaky, slope, dropout_p, seed, seed_dev, salt, c, ldc, c_dtype,
                   ct, ld_t, ct_scale, M, N, K, k_b):
    return _lib.lib().mobgt_small_gemm_f32_act(addr(a), lda, addr(a_mask), float(mask_vals[0]), float(mask_vals[1]),
                                               float(mask_vals[2]), addr(b), ldb, int(b_is_nk), addr(bias), int(leaky), float(slope),
                                               float(dropout_p), int(seed), addr(seed_dev), int(salt) & 0xFFFFFFFF, addr(c), ldc,
                                               c_dtype, addr(ct), ld_t, addr(ct_scale), M, N, K, k_b, _stream())


def bias_act_fwd(x, bias, y, R, C, slope, dropout_p, seed, seed_dev, salt):
    return _lib.lib().mobgt_bias_act_fwd(addr(x), addr(bias), addr(y), R, C, float(slope), float(dropout_p), int(seed),
                                         addr(seed_dev), int(salt) & 0xFFFFFFFF, _stream())


def bias_act_fwd_t(x, bias, y, y_t, ld_t, R, C, slope, dropout_p, seed, seed_dev, salt):
    return _lib.lib().mobgt_bias_act_fwd_t(addr(x), addr(bias), addr(y), addr(y_t), ld_t, R, C, float(slope), float(dropout_p),
                                           int(seed), addr(seed_dev), int(salt) & 0xFFFFFFFF, _stream())
