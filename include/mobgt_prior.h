/* C ABI of mobgt_amd/libmobgt_prior.so -- the fitted Markov tables (include/mobgt_baseline.h, mobgt_amd/baseline.py) blended as a
 * prior into a model's scores on the device: one launch over [G, V] f32 scores.
 *
 * The rule is stated in the docstring of mobgt_amd/prior.py (blend_host there is the same rule as a plain definition).  In short:
 * three f32 tables of logarithms, made on the host and only gathered from here -- lg[e] = f32(log1p(val[e])) beside the cg CSR,
 * lu[e] = f32(log1p(uval[e])) beside the cu keys, lp[p] = f32(log1p(pop[p])) -- and three f32 weights in device memory,
 * weights[0 .. 2] = (wu, wg, wp), read by the kernel.  Row g has the anchor a = the last entry of hist[g, 0 .. n) that is not 0
 * (an id outside 1 .. P: no anchor) and the user u = user[g] - user_offset (outside [0, U): no user rows).  Column c is POI
 * p = c + label_offset.  Every operation is rounded on its own (no FMA), in exactly this order:
 *
 *     s = scores[g, c]
 *     if 1 <= p <= P and lp[p - 1] > 0:                                   s = s + wp * lp[p - 1]
 *     if a exists and row a of the CSR holds p (entry e) and lg[e] > 0:  s = s + wg * lg[e]
 *     if additionally the cu keys hold (u, a, p) (entry e') and lu[e'] > 0:  s = s + wu * lu[e']
 *     out[g, c] = s
 *
 * A term that does not apply is not added, so -0.0 survives; non-finite scores go through the arithmetic as IEEE gives.
 *
 * A library of its own: the other headers and their ABI versions are not touched.  gfx950 code objects only.  One plain launch on
 * `stream` (the last argument), graph-capturable: no allocation, no host synchronisation, no workgroup waits for another, no
 * atomics on scores.  Buffers are caller-owned device memory; rows have unit element stride.  Return: 0 on success, one of the
 * MOBGT_PRIOR_E* codes (checked before anything is launched), or a positive hipError_t of the launch.  Every element of
 * out[:, 0 .. V) is written exactly once, by one workgroup; nothing else is written but status[0].  A pointer to a buffer of zero
 * elements may be null.  An index read from a buffer is checked against the size of what it indexes before it is used; what fails
 * is skipped and flagged in status[0].  lp, lg, lu and the keys are values, never indices.
 */
#ifndef MOBGT_PRIOR_H
#define MOBGT_PRIOR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_PRIOR_EBADDIM (-1)   /* a size or a parameter outside the limits                            */
#define MOBGT_PRIOR_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */
#define MOBGT_PRIOR_EDTYPE (-3)    /* hist_dtype or user_dtype is not one of the two below                */

/* hist_dtype / user_dtype */
#define MOBGT_PRIOR_I32 0
#define MOBGT_PRIOR_I64 1

/* columns of a row one workgroup blends: the grid is (ceil(V / CHUNK), G) */
#define MOBGT_PRIOR_CHUNK 2048

/* threads of a workgroup: CHUNK / THREADS columns each */
#define MOBGT_PRIOR_THREADS 256

/* the rows of one launch (the grid's second dimension) */
#define MOBGT_PRIOR_MAX_G 65535

/* bits of status[0]; sticky: the kernel only ORs into the word, the caller zeroes it */
#define MOBGT_PRIOR_SBADINDEX 1    /* a rowptr pair that is descending or lies beyond nnz, or an entry of col outside [0, P) */

#define MOBGT_PRIOR_ABI_VERSION 1
int mobgt_prior_abi_version(void);

/* out[g, c] = the blend of scores[g, c] (the rule above).  out == scores (in place, then ld_out == ld_scores) and buffers that do
 * not overlap are both legal.
 *
 * In:  scores [G, >= V] f32, ld_scores elements between rows
 *      hist [G, n_hist_cols] int32 / int64 (hist_dtype), ld_hist elements between rows: POI ids, 0 = padding
 *      user [G] int32 / int64 (user_dtype), ld_user elements between rows
 *      rowptr [P + 1] int64, col [nnz] int32 (0-based POIs, ascending inside a row), lg [nnz] f32       the cg CSR
 *      ukey [nnzU] int64 (ascending, distinct: (u * P + a - 1) * P + (b - 1)), lu [nnzU] f32              the cu table; nnzU = 0: none
 *      lp [P] f32
 *      weights [3] f32        (wu, wg, wp), read on the device
 * Out: out [G, >= V] f32, ld_out elements between rows; columns from V on are left alone
 *      status [1] int32       SBADINDEX is ORed in with a vector atomic; never cleared here
 *
 * A workgroup of THREADS threads per (chunk of CHUNK columns, row).  It finds the row's anchor (the search of
 * mobgt_amd/csrc_prior/blend_rows.h, shared by the three priors), checks the anchor's rowptr pair, and finds -- by searches that probe 64 places a step, a lane a
 * place, with the same result in every lane -- the part of CSR row a whose columns lie in its chunk and, if that part is not
 * empty, the (u, a) range of ukey.  It loads its chunk of the row into LDS with the popularity term added, adds the entries'
 * terms there (a thread an entry; cu(u, a, p) by a binary search of the (u, a) range), and stores the chunk.  A rowptr pair
 * that is descending or beyond nnz makes the row count as empty; an entry of col outside [0, P) is skipped; both raise
 * SBADINDEX.  An entry whose column falls outside the chunk or [0, V) is skipped silently (V and P need not agree).
 * Limits: 0 <= G <= MAX_G; 0 <= V, nnz, nnzU, n_hist_cols < 2^31; 1 <= P < 2^31; 0 <= U and U * P * P < 2^63; ld_scores, ld_out
 * >= V; ld_hist >= n_hist_cols; ld_user >= 1; label_offset and user_offset 0 or 1; out == scores only with ld_out == ld_scores
 * -- else EBADDIM.  G = 0 or V = 0: nothing is launched. */
int mobgt_prior_blend_rows(const float* scores, int64_t ld_scores, float* out, int64_t ld_out, int64_t G, int64_t V,
                           int64_t label_offset,
                           const void* hist, int hist_dtype, int64_t ld_hist, int64_t n_hist_cols,
                           const void* user, int user_dtype, int64_t ld_user, int64_t user_offset,
                           const void* rowptr, const void* col, const float* lg, int64_t nnz,
                           const void* ukey, const float* lu, int64_t nnzU, int64_t U,
                           const float* lp, int64_t P, const float* weights, void* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
