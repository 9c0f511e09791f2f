/* C ABI of mobgt_amd/libmobgt_priorfit.so -- what a maximum-likelihood fit of the priors' weights needs of one batch: the
 * softmax expectation of K features and of their K (K + 1) / 2 products over [G, V] scores, for L candidate weight rows at once.
 *
 * The rule is stated in the docstring of mobgt_amd/priorfit.py (terms_host there is the same rule in numpy float64).  In short,
 * everything converted to f64 when loaded and all arithmetic f64:
 *     z[l, g, c] = base[g, c] + W[l, 0] * feats[0, g, c] + ... + W[l, K - 1] * feats[K - 1, g, c]      (0 for an absent base;
 *                  summed in this order, every product and sum rounded on its own: no FMA)
 *     p = softmax(z[l, g, :]),   mu_k = sum_c p_c F_kc,   t = y[g] + target_offset
 *     terms[l, g, :] = ( n,  nll = logsumexp(z) - z[t],  g_k = mu_k - F_k[t],  H_kj = sum_c p_c F_kc F_jc - mu_k mu_j  for k <= j,
 *                        row-major )                                                       NT = 2 + K + K (K + 1) / 2 doubles
 * Row g counts (n = 1) if t is in [0, V), no z[l, g, :] of any l is NaN or +inf, no feature value of the row is non-finite, no
 * z[l, g, :] is -inf throughout, and every z[l, g, t] is finite.  -inf in base is a masked column of probability 0.  A row that
 * does not count has all NT terms 0 for every l; unless its target is merely out of range, SNONFINITE is ORed into status[0].
 *
 * A library of its own: the other headers and their ABI versions are not touched.  gfx950 code objects only.  The entry point is
 * a plain launch sequence on `stream` (the last argument), graph-capturable: no allocation, no host read, no host
 * synchronisation, no workgroup waits for another; the only atomic is the integer OR into status[0], so the same inputs give
 * the same bits on every run.  Buffers are caller-owned device memory; rows have unit element stride.  Return: 0 on success, one
 * of the MOBGT_PRIORFIT_E* codes (checked before anything is launched), or a positive hipError_t of a launch.  EVERY element of
 * terms is written by every call that launches anything (G = 0 or V = 0 launches nothing); the workspace needs no preparation.
 */
#ifndef MOBGT_PRIORFIT_H
#define MOBGT_PRIORFIT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_PRIORFIT_EBADDIM (-1)   /* a size or a parameter outside the limits                            */
#define MOBGT_PRIORFIT_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */
#define MOBGT_PRIORFIT_EDTYPE (-3)    /* y_dtype is not one of the two below                                 */

/* y_dtype */
#define MOBGT_PRIORFIT_I32 0
#define MOBGT_PRIORFIT_I64 1

/* limits: features, weight rows, rows of scores */
#define MOBGT_PRIORFIT_MAX_K 8
#define MOBGT_PRIORFIT_MAX_L 16
#define MOBGT_PRIORFIT_MAX_G 65535

/* doubles of one (l, g) of terms at K = MAX_K: 2 + K + K (K + 1) / 2 (mobgt_priorfit_nt gives it for any K) */
#define MOBGT_PRIORFIT_MAX_NT 46

/* the partials launch: threads of a workgroup, the columns of a row it owns -- the grid is (ceil(V / CHUNK), G) -- and the
 * consecutive columns a thread holds in registers (one 16-byte load per plane where the row allows it) */
#define MOBGT_PRIORFIT_THREADS 256
#define MOBGT_PRIORFIT_CHUNK 1024
#define MOBGT_PRIORFIT_COLS 4

/* the combine launch: one wave per (l, g), a lane per summed term */
#define MOBGT_PRIORFIT_WAVE 64

/* bits of status[0]; sticky: the kernel only ORs into the word, the caller zeroes it */
#define MOBGT_PRIORFIT_SNONFINITE 1   /* a row broke one of the finiteness conditions of the rule and was left out */

#define MOBGT_PRIORFIT_ABI_VERSION 1
int mobgt_priorfit_abi_version(void);

/* NT of K features: 2 + K + K (K + 1) / 2; K outside 1 .. MAX_K: EBADDIM. */
int mobgt_priorfit_nt(int K);

/* Bytes of the workspace mobgt_priorfit_terms needs for these sizes: one record of 1 + NT doubles -- a flag, the chunk's maximum
 * m, Z = sum e, A_k = sum e F_k, B_kj = sum e F_k F_j (k <= j), e = exp(z - m) -- per (g, l, chunk of CHUNK columns).  0 where
 * nothing is launched; sizes outside the limits below: EBADDIM. */
int64_t mobgt_priorfit_work_bytes(int K, int64_t G, int64_t V, int L);

/* terms[l, g, :] of the rule above for every l in [0, L) and g in [0, G).
 * In:  base [G, >= V] f32, ld_base elements between rows; NULL: absent (z starts from 0)
 *      feats [K, G, >= V] f32: ld_feats elements between rows, plane_feats elements between features
 *      y [G] int32 / int64 (y_dtype), ld_y elements between rows;  target_offset: added to y[g]
 *      W [L, K] f64, contiguous, read on the device
 *      work: work_bytes of the same sizes, 8-byte aligned; holds nothing the caller need keep or prepare
 * Out: terms [L, G, NT] f64, contiguous
 *      status [1] int32: SNONFINITE is ORed in with a vector atomic; never cleared here
 * Two launches.  Partials: a workgroup of THREADS threads per (chunk, row) loads its COLS columns per thread of base and of the
 * K planes once and, for each l in turn, reduces the chunk's record across the workgroup and stores it.  Combine: one wave per
 * (l, g) takes the maximum of the chunks' m, sums the records in chunk order, each scaled by exp(m_chunk - m) -- a chunk whose m
 * is -inf is skipped, never rescaled -- reads z[t] and F_k[t] and writes the NT terms.  Columns from V on are never read.
 * Limits: 1 <= K <= MAX_K; 1 <= L <= MAX_L; 0 <= G <= MAX_G; 0 <= V < 2^31; ld_base, ld_feats, plane_feats >= V (planes may
 * interleave rows: only the strides are read); ld_y >= 1 -- else EBADDIM.  G = 0 or V = 0: nothing is launched. */
int mobgt_priorfit_terms(const float* base, int64_t ld_base, const float* feats, int64_t ld_feats, int64_t plane_feats, int K,
                         int64_t G, int64_t V, const void* y, int y_dtype, int64_t ld_y, int64_t target_offset, const double* W,
                         int L, void* work, double* terms, void* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
