/* C ABI of mobgt_amd/libmobgt_tokscatter.so -- the scatter of the encoder input's gradients into the embedding tables' gradients
 * (the backward of mobgt_embed_gather_multi of include/mobgt_hip.h; model_fqandtoyo.py:1259-1298 backwards) for a few hundred
 * positions, as one BURST per position: the wave that owns a position requests all of its indices, then every piece of every
 * job's gradient row, and only then issues its atomics -- three dependent memory round trips where mobgt_embed_gather_multi's
 * backward walks the jobs one behind the other (about twenty at the fq model's widths).
 *
 * A library of its own: the other headers, their exports and their ABI versions are not touched.  gfx950 code objects only.  One
 * plain launch on `stream` (the last argument), graph-capturable: no allocation, no host synchronisation, and NO workgroup waits
 * for another (no counter, no fence).  Buffers are caller-owned device memory.  Return: 0 on success, a MOBGT_TOKSCATTER_E* code
 * (checked before anything is launched), or a positive hipError_t of the launch.
 */
#ifndef MOBGT_TOKSCATTER_H
#define MOBGT_TOKSCATTER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_TOKSCATTER_EBADDIM (-1)   /* a size outside the limits, a null buffer, an identity job or a ride that cannot be   */
#define MOBGT_TOKSCATTER_EALIGN (-2)    /* a pointer or stride that violates the documented alignment                           */
#define MOBGT_TOKSCATTER_EDTYPE (-3)    /* unknown index dtype code                                                             */

#define MOBGT_TOKSCATTER_ABI_VERSION 1
int mobgt_tokscatter_abi_version(void);

/* index dtype codes (those of include/mobgt_hip.h) */
#define MOBGT_TOKSCATTER_I64 0
#define MOBGT_TOKSCATTER_I32 1
/* jobs of one launch, and the widest table row: a lane holds MAX_WIDTH / 64 values per job in registers; anything wider is refused */
#define MOBGT_TOKSCATTER_MAX_JOBS 8
#define MOBGT_TOKSCATTER_MAX_WIDTH 192
/* widest contraction (= the identity job's width) and output of the product that may ride */
#define MOBGT_TOKSCATTER_RIDE_MAX_K 192
#define MOBGT_TOKSCATTER_RIDE_MAX_N 64

/* d_tables[t][idx[t][r], :] += buf[t][r * ld[t] + coff[t] : + width[t]]  for r < R and the n <= MAX_JOBS jobs t, by f32 atomics;
 * position r is skipped by job t when idx[t][r] < 0 or == skip[t] (skip null: nothing is skipped by value), a job whose d_tables[t]
 * is null is skipped altogether.  idx [R] of idx_dtype (one type for all jobs); width[t] in 1 .. MAX_WIDTH, any value (no multiple of
 * 4 asked: the kernel moves single floats); f32 pointers 4-byte aligned.  extra_row0 (optional): a [width[extra_job]] vector added
 * to ROW 0 of d_tables[extra_job].  R <= 0: nothing is launched.
 *
 * identity_job (-1: none): a job whose table is the position list itself -- row r of d_tables[identity_job] ([R, width], row stride
 * width) belongs to position r and to nobody else.  Its rows are WRITTEN with plain stores, zeros where the position is skipped, so
 * that destination needs no zero-fill; the index is only read for its sign / skip value.  extra_job may not be the identity job.
 *
 * The ride (ride_gut null: none; needs an identity job): with g = the identity job's gradient rows (buf[j] + coff[j], [R, K = width[j]],
 * rows the job skips counting as zeros),
 *     ride_gut[c * ride_ldt + r] = bf16( (g ride_w^T)[r, c] * ride_scale[r] )     r < R, c < ride_n,  ride_w f32 [ride_n, K] (row stride ride_ldw)
 * -- what mobgt_small_gemm_f32_act(g, ride_w, b_is_nk = 1, c = null, c_t_bf16 = ride_gut, c_t_scale = ride_scale) leaves, bit for
 * bit, computed by extra workgroups of the same launch from the gradient rows directly (they wait for nobody).  K % 16 == 0,
 * K <= RIDE_MAX_K, ride_n <= RIDE_MAX_N, ride_ldt >= R; the gradient rows and ride_w 16-byte aligned with row strides that are
 * multiples of 4 (MOBGT_TOKSCATTER_EALIGN otherwise).  ride_scale null: no scaling. */
int mobgt_tokscatter_bwd(int n, float* const* d_tables, const void* const* idx, const int64_t* skip, const int* width,
                         const int* coff, const float* const* buf, const int64_t* ld, int64_t R, int idx_dtype,
                         const float* extra_row0, int extra_job, int identity_job, const float* ride_w, int64_t ride_ldw,
                         const float* ride_scale, void* ride_gut, int64_t ride_ldt, int ride_n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
