/* C ABI of mobgt_amd/libmobgt_ctxprior.so -- a fitted category-transition and time-of-day prior on a model's next-POI scores: what
 * kind of place follows what kind of place, and what kind of place people go to at this time of day, as two f32 tables over the
 * categories, added to the scores on the device.
 *
 * The rule is stated in the docstring of mobgt_amd/ctxprior.py (the host forms there are the same rule as plain definitions).  In
 * short: with C = n_cat categories 1 .. C, S = n_slots time slots 0 .. S - 1 and poi_cat[p - 1] in 0 .. C the category of POI p,
 *     gc[a - 1, b - 1]   consecutive check-in pairs inside one TRAIN session with categories a -> b       (UniverseCounts.graph_cat)
 *     st[s, b - 1]       the same pairs whose FIRST row has slot s and whose second row has category b     (slot_hist, here)
 * are exact integer counts; the host turns them into two f32 tables Tc [C, C] and Tt [S, C] (no transcendental runs in a kernel),
 * and the blend adds, where row g has an anchor position j (the last entry of hist[g, 0 .. n) that is not 0, its id in 1 .. P),
 * ca = cat[g, j], ta = time[g, j], column c is a POI p = c + label_offset in 1 .. P and k = poi_cat[p - 1] is in 1 .. C,
 *     v = scores[g, c]
 *     if 1 <= ca <= C:   v = v + w_category * Tc[ca - 1, k - 1]
 *     if 0 <= ta <  S:   v = v + w_time * Tt[ta, k - 1]
 *     out[g, c] = v
 * in this order, every product and every sum rounded to f32 on its own (no FMA).  Every other element is copied bit for bit.
 *
 * A library of its own: the other headers and their ABI versions are not touched.  gfx950 code objects only.  Every function is
 * a plain launch sequence on `stream` (the last argument), graph-capturable: no allocation, no host synchronisation, no
 * workgroup waits for another; atomics are on integers only, so no result depends on an order.  Buffers are caller-owned device
 * memory; rows have unit element stride.  Return: 0 on success, one of the MOBGT_CTXPRIOR_E* codes (checked before anything is
 * launched), or a positive hipError_t of a launch.  EVERY element of every output is written by every call: the caller never
 * pre-zeroes anything (the histogram is cleared on `stream` by the call itself); only status[0] is ORed into.  A pointer to a
 * buffer of zero elements may be null.  A value read from a buffer is checked against the size of what it indexes before it is
 * used as an index; what fails is skipped and, in slot_hist, flagged in status[0].
 */
#ifndef MOBGT_CTXPRIOR_H
#define MOBGT_CTXPRIOR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_CTXPRIOR_EBADDIM (-1)   /* a size or a parameter outside the limits                            */
#define MOBGT_CTXPRIOR_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */
#define MOBGT_CTXPRIOR_EDTYPE (-3)    /* hist_dtype or ctx_dtype is not one of the two below                 */

/* hist_dtype, ctx_dtype */
#define MOBGT_CTXPRIOR_I32 0
#define MOBGT_CTXPRIOR_I64 1

/* threads of every workgroup of this library */
#define MOBGT_CTXPRIOR_THREADS 256

/* the categories and the slots of one prior.  blend_rows stages two rows of MAX_CAT products in LDS (2 * 4 * 4096 = 32 KB of a
 * CU's 160 KB: five workgroups of a CU hold theirs at once); MAX_CAT is mobgt_universe.h's limit, so every UniverseCounts fits.
 * Tc is [n_cat, n_cat] f32 (64 MB at the limit), the slot histogram [n_slots, n_cat] int64 (32 MB at both limits). */
#define MOBGT_CTXPRIOR_MAX_CAT 4096
#define MOBGT_CTXPRIOR_MAX_SLOTS 1024

/* slot_hist: up to this many cells (n_slots * n_cat) a workgroup counts in a 32-bit histogram of its own in LDS: 4 * 32768 =
 * 128 KB of a CU's 160 KB (163 840 bytes), the rest left to the runtime; with more cells every count goes to global memory as a
 * 64-bit vector atomic */
#define MOBGT_CTXPRIOR_LDS_CELLS 32768

/* slot_hist: sessions a workgroup takes per step (a wave per session), and the most workgroups of one launch (each walks the
 * sessions b, b + grid, ... in steps, so its LDS histogram is cleared and flushed once) */
#define MOBGT_CTXPRIOR_SESSIONS 64
#define MOBGT_CTXPRIOR_MAX_GRID 1024

/* blend_rows: columns of a row one workgroup blends -- the grid is (ceil(V / CHUNK), G) -- and the rows of one launch */
#define MOBGT_CTXPRIOR_CHUNK 1024
#define MOBGT_CTXPRIOR_MAX_G 65535

/* bits of status[0]; sticky: the kernel only ORs into the word, the caller zeroes it */
#define MOBGT_CTXPRIOR_SBADINDEX 1    /* an offsets pair that is descending or lies outside [0, M]: the session is skipped        */
#define MOBGT_CTXPRIOR_SBADVALUE 2    /* a pair whose slot is outside [0, n_slots) or whose destination category is outside 1 .. n_cat */

#define MOBGT_CTXPRIOR_ABI_VERSION 1
int mobgt_ctxprior_abi_version(void);

/* counts[s * n_cat + b - 1] = #{pairs (k - 1, k) of consecutive check-ins inside one TRAIN session : seq[k - 1, 1] = s and
 * seq[k, 2] = b}.  Session i holds the rows offsets[i] .. offsets[i + 1] - 1 and is a train session where train[i] != 0; a session
 * of fewer than two rows has no pair; the pair into a session's last (target) row counts, no pair spans two sessions.
 * In:  seq [M, 3] int32        check-ins as data.SessionDataset packs them: rows (poi, time slot, category); the POI is not read
 *      offsets [n_sessions + 1] int64;  train [n_sessions] uint8
 * Out: counts [n_slots * n_cat] int64, cleared on `stream` by the call itself
 *      status [1] int32        S* bits are ORed in with a vector atomic; never cleared here
 * An offsets pair that is descending or lies outside [0, M] skips its session (train or not) and raises SBADINDEX; a pair whose
 * slot is outside [0, n_slots) or whose destination category is outside 1 .. n_cat is skipped and raises SBADVALUE.
 * A wave per session, its lanes over the session's pairs, SESSIONS sessions per workgroup and step, at most MAX_GRID workgroups.
 * While n_slots * n_cat <= LDS_CELLS a workgroup counts in LDS (32-bit: M < 2^31 pairs) and flushes its non-zero cells once with
 * 64-bit vector atomics; beyond, every count is such an atomic on global memory.  Both forms give the same integers.
 * Limits: 0 <= M < 2^31, 0 <= n_sessions < 2^31, 1 <= n_slots <= MAX_SLOTS, 1 <= n_cat <= MAX_CAT -- else EBADDIM.
 * n_sessions = 0 or M = 0 clears counts and launches nothing else. */
int mobgt_ctxprior_slot_hist(const void* seq, int64_t M, const void* offsets, int64_t n_sessions, const void* train, int n_slots,
                             int n_cat, void* counts, void* status, void* stream);

/* out[g, c] = the blend of scores[g, c] (the rule above).  out == scores (in place, then ld_out == ld_scores) and buffers that
 * do not overlap are both legal.
 * In:  scores [G, >= V] f32, ld_scores elements between rows
 *      hist [G, n_hist_cols] int32 / int64 (hist_dtype), ld_hist elements between rows: POI ids, 0 = padding
 *      time, cat [G, n_hist_cols] int32 / int64 (ctx_dtype, one flag for both), ld_ctx elements between rows (one stride for
 *                both): the raw slot and the category at hist's positions
 *      poi_cat [P] int32;  cat_table [n_cat, n_cat] f32;  slot_table [n_slots, n_cat] f32
 *      weights [2] f32 (category, time), read on the device
 * Out: out [G, >= V] f32, ld_out elements between rows; columns from V on are left alone
 * A workgroup of THREADS threads per (chunk of CHUNK columns, row).  It finds the row's anchor position (the search of
 * mobgt_amd/csrc_prior/blend_rows.h, shared by the three priors), reads ca and ta there, stages the PRODUCTS w_category * Tc[ca - 1, :] and
 * w_time * Tt[ta, :] in LDS (n_cat floats each, only those whose context is valid), and every thread blends CHUNK / THREADS
 * columns: the score and poi_cat, two LDS reads, two adds, one store.  An element is read and written by the same thread, so in
 * place is safe.
 * Limits: 0 <= G <= MAX_G; 0 <= V, n_hist_cols < 2^31; 1 <= P < 2^31; n_cat and n_slots as above; ld_scores, ld_out >= V;
 * ld_hist, ld_ctx >= n_hist_cols; label_offset 0 or 1; out == scores only with ld_out == ld_scores -- else EBADDIM.
 * G = 0 or V = 0: nothing is launched. */
int mobgt_ctxprior_blend_rows(const float* scores, int64_t ld_scores, float* out, int64_t ld_out, int64_t G, int64_t V,
                              int64_t label_offset, const void* hist, int hist_dtype, int64_t ld_hist, int64_t n_hist_cols,
                              const void* time, const void* cat, int ctx_dtype, int64_t ld_ctx, const int32_t* poi_cat, int64_t P,
                              const float* cat_table, const float* slot_table, int n_cat, int n_slots, const float* weights,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
