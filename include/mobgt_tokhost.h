/* C ABI of mobgt_amd/libmobgt_tokhost.so -- the encoder input's one-launch backward (mobgt_token_bwd_chain of include/mobgt_hip.h,
 * csrc/tokbwd_body.h) in the form that also finishes what the FIRST encoder layer's backward left undone behind its attention
 * backward (model_fqandtoyo.py:1731-1743 backwards; autograd of linear_q / k / v, :1687-1689).  Every other layer leaves that to the
 * mobgt_layer_chain_bwd launch of the layer below it; the first layer has no layer below, and the next launch on the device is this one.
 *
 * A library of its own: the other headers, their exports and their ABI versions are not touched.  gfx950 code objects only.  One
 * plain launch on `stream` (the last argument), graph-capturable: no allocation, no host synchronisation, and NO workgroup waits for
 * another (no counter, no fence).  Buffers are caller-owned device memory.  Return: 0 on success, a MOBGT_TOKHOST_E* code (checked
 * before anything is launched), or a positive hipError_t of the launch.
 */
#ifndef MOBGT_TOKHOST_H
#define MOBGT_TOKHOST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_TOKHOST_EBADDIM (-1)   /* a size outside the limits, a null buffer, half a tail, dx1 that is not dout */
#define MOBGT_TOKHOST_EALIGN (-2)    /* a pointer that violates the documented alignment                             */

#define MOBGT_TOKHOST_ABI_VERSION 1
int mobgt_tokhost_abi_version(void);

/* weight-gradient problems one launch hosts */
#define MOBGT_TOKHOST_MAX_WG 4
/* token rows G*(N+1) up to which a launch hosts anything: the rows up to which mobgt_layer_backward_tail, whose sums are reproduced,
 * runs its 8-wave form */
#define MOBGT_TOKHOST_MAX_ROWS 1024

/* The first 26 arguments are mobgt_token_bwd_chain's (include/mobgt_hip.h; model_fqandtoyo.py:1264-1298, 1338-1347, FuseEmbeddings
 * 444-456), with the same results:  d = dropouts'(dout[g, 1 + n]);  d_add = d;  d_nf = d * real;  dx4 = (d_nf * leaky'(y4)) w4;
 * d_pt = (dx4[:, :W2] * leaky'(y2)) w2;  d_token += sum of the graph-token rows' d.  (C, W2) = (192, 160), G >= 1, N >= 1.
 *   tail_dqkv [G*(N+1), 3C] bf16 + tail_wqkv_t (the layer's Wqkv^T, packed by mobgt_pack_mfma_b(transposed = 1)): `dout` then
 *     holds only the layer's dx1; every row workgroup forms its rows of dout = dx1 + dqkv Wqkv before it reads them (the graph-token
 *     rows too: their column sums are d_token) and writes them back in place.  dx1 must BE dout.  The sum over K runs in the order
 *     of mobgt_layer_backward_tail's product (eight partial sums over the k-steps i, i + 8, i + 16, added in order, then dx1), so
 *     the two agree bit for bit.  Both null: no tail.
 *   wg_*: n_wg <= MOBGT_TOKHOST_MAX_WG weight-gradient problems dW [M,N] += g^T x (+ db [M] += column sums of g) over the G*(N+1)
 *     token rows, bf16 operands, the argument arrays of mobgt_layer_chain_bwd; run by extra workgroups of this launch with the
 *     tiles, splits and sums of mobgt_layer_backward_tail's.  n_wg = 0: none.
 * d_token: a workgroup adds its (up to 16) graphs' rows in float64 and rounds once (mobgt_token_bwd_chain: f32 atomics per row).
 * No tail and n_wg = 0: the launch is mobgt_token_bwd_chain's kernel.  tail_dqkv / tail_wqkv_t / dx1 16-byte aligned; operand
 * alignment of the problems as mobgt_linear_wgrad.  With a tail or problems, G*(N+1) <= MOBGT_TOKHOST_MAX_ROWS. */
int mobgt_tokhost_token_bwd_chain(const float* dout, const float* real, const float* y4, const float* y2, int64_t ld_y2,
                                  const float* w4, const float* w2, float* d_nf, float* d_add, float* dx4, int64_t ld_dx4,
                                  float* d_pt, float* d_token, int G, int N, int C, int W2, float slope4, float slope2, float p_pos,
                                  float p_in, uint64_t seed, const uint64_t* seed_dev, uint32_t salt_nf, uint32_t salt_tok,
                                  uint32_t salt_in, const void* tail_dqkv, const void* tail_wqkv_t, float* dx1, int n_wg,
                                  const void* const* wg_g, const int64_t* wg_ldg, const void* const* wg_x, const int64_t* wg_ldx,
                                  float* const* wg_dw, const int64_t* wg_ldw, float* const* wg_db, const int* wg_M, const int* wg_N,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
