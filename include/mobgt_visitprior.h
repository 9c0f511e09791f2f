/* C ABI of mobgt_amd/libmobgt_visitprior.so -- a fitted per-user visit-frequency and recency prior on a model's next-POI scores:
 * how often this user has been at a POI and how long ago, counted in the user's own train check-ins, as two f32 tables over a
 * CSR by user, added to the scores on the device.
 *
 * The rule is stated in the docstring of mobgt_amd/visitprior.py (the host forms there are the same rule as plain definitions).  In
 * short: the train rows of user u, in dataset order, are numbered 0 .. N_u - 1, and for every POI p among them
 *     n(u, p)    = how many of those rows have POI p                                   (cnt)
 *     last(u, p) = the largest number among those rows;  age(u, p) = N_u - 1 - last    (age)
 * are exact integers, stored as a CSR by user: rowptr int64 [U + 1], col int32 [nnz] (the 0-based POI, strictly ascending inside
 * a row), cnt and age int32 [nnz], tot int32 [U] = N_u.  The host turns them into two f32 tables F and R [nnz] (no transcendental
 * runs in a kernel), and the blend adds, where row g has u = user[g] - user_offset in [0, U) and entry e of row u has the column
 * c = col[e] + 1 - label_offset in [0, V),
 *     v = scores[g, c]
 *     v = v + w_visits * F[e]
 *     v = v + w_recency * R[e]
 *     out[g, c] = v
 * in this order, every product and every sum rounded to f32 on its own (no FMA).  Every other element is copied bit for bit.  The
 * history ids are not read: the prior has no anchor.
 *
 * A library of its own: the other headers and their ABI versions are not touched.  gfx950 code objects only.  Every function is
 * a plain launch sequence on `stream` (the last argument), graph-capturable: no allocation, no host synchronisation, no
 * workgroup waits for another; integers only in the fit, no atomics on floats anywhere, so no result depends on an order.  Buffers
 * are caller-owned device memory; rows have unit element stride.  Return: 0 on success, one of the MOBGT_VISITPRIOR_E* codes
 * (checked before anything is launched), or a positive hipError_t of a launch.  Only status[0] is ORed into.  A pointer to a buffer
 * of zero elements may be null.  A value read from a buffer is checked against the size of what it indexes before it is used as an
 * index; what fails is skipped and flagged in status[0].
 */
#ifndef MOBGT_VISITPRIOR_H
#define MOBGT_VISITPRIOR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_VISITPRIOR_EBADDIM (-1)   /* a size or a parameter outside the limits                            */
#define MOBGT_VISITPRIOR_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */
#define MOBGT_VISITPRIOR_EDTYPE (-3)    /* hist_dtype or user_dtype is not one of the two below                */

/* hist_dtype, user_dtype */
#define MOBGT_VISITPRIOR_I32 0
#define MOBGT_VISITPRIOR_I64 1

/* threads of every workgroup of this library */
#define MOBGT_VISITPRIOR_THREADS 256

/* blend_rows: columns of a row one workgroup owns -- the grid is (ceil(V / CHUNK), G) -- and the rows of one launch */
#define MOBGT_VISITPRIOR_CHUNK 1024
#define MOBGT_VISITPRIOR_MAX_G 65535

/* a key is u * P + (p - 1): U * P stays below 2^62 (KEY_BITS), P, U, nnz and the check-ins below 2^31 */
#define MOBGT_VISITPRIOR_KEY_BITS 62

/* bits of status[0]; sticky: the kernels only OR into the word, the caller zeroes it.  SBADINDEX -- blend: a rowptr pair that is
 * descending or beyond nnz (the row counts as empty) or an entry of col outside [0, P) (skipped); keys: a session index or a key
 * slot that does not match.  SBADVALUE -- keys / fill: a POI outside 1 .. P, a user outside [0, U), an age outside [0, N_u) */
#define MOBGT_VISITPRIOR_SBADINDEX 1
#define MOBGT_VISITPRIOR_SBADVALUE 2

#define MOBGT_VISITPRIOR_ABI_VERSION 1
int mobgt_visitprior_abi_version(void);

/* The fit's first launch: one 64-bit key and one number per train check-in.  Row i of the packed check-ins belongs to session
 * s = sid[i]; where slot0[s] >= 0 (a train session) its k-th row (k = i - first[s]) writes
 *     keys[slot0[s] + k] = users[s] * P + (poi - 1)        ord[slot0[s] + k] = ord0[s] + k
 * In:  seq [M, 3] int32 rows (poi, time slot, category), only the POI is read;  sid [M] int32
 *      first [S] int64 the session's first row;  slot0 [S] int64 its first key slot, -1 for a session out of train
 *      ord0 [S] int64 the number of its first row among its user's train rows;  users [S] int64
 * Out: keys [T] int64, set to -1 on `stream` by the call itself and then written;  ord [T] int32
 * A session index outside [0, S), a row before its session's first or a key slot outside [0, T) skips the row and raises
 * SBADINDEX; a POI outside 1 .. P, a user outside [0, U) or a number outside [0, 2^31) skips it and raises SBADVALUE (its key
 * stays -1).
 * Limits: 0 <= M, S, T < 2^31; 1 <= P < 2^31; 0 <= U < 2^31; U * P < 2^KEY_BITS -- else EBADDIM.  M = 0 or T = 0 launches no kernel. */
int mobgt_visitprior_keys(const void* seq, const void* sid, int64_t M, const void* first, const void* slot0, const void* ord0,
                          const void* users, int64_t S, int64_t P, int64_t U, void* keys, void* ord, int64_t T, void* status,
                          void* stream);

/* The fit's last launch, over the keys sorted ascending (stably, so ord ascends inside a run of equal keys), ord moved with them,
 * and pos [T] int64 the inclusive cumulative count of run heads (pos[i] - 1 is the run of key i; nnz = pos[T - 1]): for run r
 * of key k = u * P + q with the rows [i, j) of the sorted arrays
 *     col[r] = q      cnt[r] = j - i      age[r] = tot[u] - 1 - ord[j - 1]
 * and rowptr[u] = the number of runs whose key lies below u * P, for u in 0 .. U.
 * In:  keys [T] int64, ord [T] int32, pos [T] int64, tot [U] int32 (N_u)
 * Out: rowptr [U + 1] int64; col, cnt, age [nnz] int32
 * A key outside [0, U * P), a run index outside [0, nnz) or an age outside [0, tot[u]) writes nothing for its run and raises
 * SBADVALUE.
 * Limits: 0 <= nnz <= T < 2^31; P, U as above -- else EBADDIM.  T = 0 still writes rowptr (all 0). */
int mobgt_visitprior_fill(const void* keys, const void* ord, const void* pos, int64_t T, int64_t P, int64_t U, int64_t nnz,
                          const void* tot, void* rowptr, void* col, void* cnt, void* age, void* status, void* stream);

/* out[g, c] = the blend of scores[g, c] (the rule above).  out == scores (in place, then ld_out == ld_scores) and buffers that
 * do not overlap are both legal.
 * In:  scores [G, >= V] f32, ld_scores elements between rows
 *      hist [G, n_hist_cols] int32 / int64 (hist_dtype), ld_hist elements between rows: checked as the other priors check it
 *           (mobgt_amd/csrc_prior/blend_rows.h) and NOT read
 *      user [G] int32 / int64 (user_dtype), ld_user elements between rows; u = user[g] - user_offset
 *      rowptr [U + 1] int64; col [nnz] int32; freq, rec [nnz] f32 (F and R)
 *      weights [2] f32 (visits, recency), read on the device
 * Out: out [G, >= V] f32, ld_out elements between rows; columns from V on are left alone
 *      status [1] int32: SBADINDEX is ORed in with a vector atomic; never cleared here
 * A workgroup of THREADS threads per (chunk of CHUNK columns, row).  Out of place it first copies its chunk (16-byte loads and
 * stores where both rows are 16-byte aligned, single elements otherwise).  It then takes row u -- all of it if it has at most
 * THREADS entries, else the entries whose column lies in its chunk, found by two searches in the ascending col -- and after one
 * barrier a thread per entry checks that the entry's column is one of the chunk's, reads the SCORE, adds the two terms and
 * stores: a chunk without entries is a plain copy, and in place it writes nothing at all.  An element is read and written by
 * its own workgroup only.  The order of col is relied on for speed only: whatever col holds, an entry is range-checked before
 * it is an index and applied only inside the chunk of its workgroup (a row whose col does not ascend strictly has no defined
 * result beyond that, and visitprior.VisitPrior refuses such tables).
 * Limits: 0 <= G <= MAX_G; 0 <= V, n_hist_cols, nnz, U < 2^31; 1 <= P < 2^31; U * P < 2^KEY_BITS; ld_scores, ld_out >= V;
 * ld_hist >= n_hist_cols; ld_user >= 1; label_offset and user_offset 0 or 1; out == scores only with ld_out == ld_scores -- else
 * EBADDIM.  G = 0 or V = 0: nothing is launched. */
int mobgt_visitprior_blend_rows(const float* scores, int64_t ld_scores, float* out, int64_t ld_out, int64_t G, int64_t V,
                                int64_t label_offset, const void* hist, int hist_dtype, int64_t ld_hist, int64_t n_hist_cols,
                                const void* user, int user_dtype, int64_t ld_user, int64_t user_offset, const void* rowptr,
                                const void* col, const float* freq, const float* rec, int64_t nnz, int64_t U, int64_t P,
                                const float* weights, void* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
