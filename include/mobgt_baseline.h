/* C ABI of mobgt_amd/libmobgt_baseline.so -- the Markov baseline of next-POI prediction on the device: the exact rank of every
 * sample's target, and the top-k list, under ONE strict total order of the POIs.
 *
 * The rule is stated in the docstring of mobgt_amd/baseline.py (ranks_host / topk_host there are the same rule as a plain
 * definition).  In short: tables counted over the train sessions -- cg(a, b) the transitions a -> b (a CSR, UniverseCounts.graph_adj),
 * cu(u, a, b) the same per user (sorted distinct 64-bit keys (u * P + a - 1) * P + (b - 1) with their counts), pop_rank a
 * permutation of the POIs (0 = the most visited, equal counts lower id first).  A sample is (session s, cut c): user u = users[s],
 * previous POI a = poi(r_{c-1}), target t = poi(r_c), history r_0 .. r_{c-1}.  Candidate p in 1 .. P has the key
 *
 *     K(p) = (cu(u, a, p), cg(a, p), -pop_rank(p))      compared lexicographically, larger first: strict and total
 *
 * `order` selects how much of it is used: 0 the full key, 1 cu taken as 0, 2 cu and cg taken as 0.  With G_a = row a of the CSR
 * (every (u, a, .) entry of cu is an entry of G_a, and every entry of G_a precedes every POI outside it):
 *
 *     rank    = #{p in G_a : K(p) > K(t)} + [cg(a, t) == 0] * (pop_rank(t) - #{p in G_a : pop_rank(p) < pop_rank(t)})
 *     revisit = 1 if t is among the history POIs, else 0
 *     ids[j]  = the POI of rank j for j < min(k, P), -1 beyond
 *
 * Integers: every result is exact.  Under order 2 the row is not read at all (rank = pop_rank(t)).
 *
 * A library of its own: the other headers and their ABI versions are not touched.  gfx950 code objects only.  Plain launches on
 * `stream` (the last argument): no allocation, no host synchronisation, no workgroup waits for another.  Buffers are caller-owned
 * device memory, C-contiguous.  Return: 0 on success, one of the MOBGT_BASELINE_E* codes (checked before anything is launched),
 * or a positive hipError_t of a launch.  EVERY element of every output is written by every call: the caller never pre-zeroes
 * anything.  A pointer to a buffer of zero elements may be null.  An index read from a buffer is checked against the size of
 * what it indexes before it is used; what fails is skipped and flagged in status[0].
 */
#ifndef MOBGT_BASELINE_H
#define MOBGT_BASELINE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_BASELINE_EBADDIM (-1)   /* a size or a parameter outside the limits                            */
#define MOBGT_BASELINE_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */

/* history rows of one sample (= MOBGT_PREFIXES_MAX_L = MOBGT_DATA_MAX_LP, the limit of the rest of the data path).  The cuts live
 * in device memory, which the host side of the ABI does not read: a sample beyond the limit is refused by the kernel (STOOLONG). */
#define MOBGT_BASELINE_MAX_L 4096

/* entries of a row, history rows, entries of pop_order one wave takes per step */
#define MOBGT_BASELINE_WAVE 64

/* the longest list of mobgt_baseline_topk: one lane per position */
#define MOBGT_BASELINE_MAX_K 64

/* samples of one workgroup: one wave each */
#define MOBGT_BASELINE_SAMPLES_PER_BLOCK 4

#define MOBGT_BASELINE_ORDER_USER 0
#define MOBGT_BASELINE_ORDER_GLOBAL 1
#define MOBGT_BASELINE_ORDER_POPULARITY 2

/* bits of status[0] */
#define MOBGT_BASELINE_SBADINDEX 1    /* a sample that failed its checks, or an entry of col / pop_order outside [0, P) */
#define MOBGT_BASELINE_STOOLONG 2     /* a sample with more than MAX_L history rows                                     */

#define MOBGT_BASELINE_ABI_VERSION 1
int mobgt_baseline_abi_version(void);

/* The rank of every sample's target and whether the target is a revisit.
 *
 * In:  seq [M, 3] int32       rows (poi, time slot, category); only the POI column is read
 *      offsets [S + 1] int64  session s is rows offsets[s] .. offsets[s + 1] - 1
 *      users [S] int64        a user outside [0, U) has no rows in the cu table: the sample backs off to cg and popularity
 *      session, cut [Q] int32 the samples (PrefixStats.session / .cut): history rows 0 .. cut - 1, target row cut
 *      rowptr [P + 1] int64, col [nnz] int32 (0-based, ascending inside a row), val [nnz] int32      the cg CSR
 *      ukey [nnzU] int64 (ascending, distinct), uval [nnzU] int32                                    the cu table; nnzU = 0: none
 *      pop_rank [P] int32     read as a value only, never as an index
 * Out: rank [Q] int32         0-based; -1 for a sample that failed its checks
 *      revisit [Q] uint8      0 / 1; 0 for a sample that failed its checks
 *      status [1] int32       0, or SBADINDEX / STOOLONG bits
 * A sample fails its checks (rank -1, revisit 0, SBADINDEX) when its session is outside [0, S), its offsets pair is not
 * 0 <= offsets[s] <= offsets[s + 1] <= M, its cut is outside 1 .. L (L = the session's rows - 1), the POI of row cut - 1 or of
 * row cut is outside 1 .. P, or the rowptr pair of the previous POI is descending or lies beyond nnz; with cut > MAX_L it fails
 * with STOOLONG.  An entry of col outside [0, P) is skipped and SBADINDEX is raised; the sample's rank counts the other entries.
 *
 * Two launches: one that clears status, then ONE WAVE PER SAMPLE, SAMPLES_PER_BLOCK samples per workgroup.  The wave finds
 * cg(a, t) in the row and the (u, a) range of the cu table by binary search (every lane the same addresses), then cu(u, a, t) inside
 * that range.  The lanes stride over the row 64 entries a step: a lane takes val, gathers pop_rank[col], searches the (u, a)
 * range for its col and compares the key with K(t); the counts are reduced by shuffles and the correction term is added.  The
 * lanes then stride over the history rows 64 a step for revisit.  No LDS.
 * Limits: 0 <= Q, S, M, nnz, nnzU < 2^31; 1 <= P < 2^31; 0 <= U and U * P * P < 2^63; order in 0 .. 2 -- else EBADDIM. */
int mobgt_baseline_ranks(const void* seq, const void* offsets, const void* users, int64_t S, int64_t M, const void* session,
                         const void* cut, int64_t Q, const void* rowptr, const void* col, const void* val, int64_t nnz,
                         const void* ukey, const void* uval, int64_t nnzU, int64_t U, const void* pop_rank, int64_t P, int64_t order,
                         void* rank, void* revisit, void* status, void* stream);

/* The k best POIs of every sample, best first.
 *
 * In:  as mobgt_baseline_ranks, and
 *      pop_order [P] int32    the inverse of pop_rank: pop_order[j] = the 0-based POI of popularity rank j
 *      k                      the length of a list
 * Out: ids [Q, k] int32       1-based POI ids; -1 from position P on; a row of -1 for a sample that failed its checks
 *      status [1] int32       as above
 * One wave per sample.  The first min(k, |G_a|) positions are the best entries of the row under K, best first: the order is
 * strict, so every round selects the largest key below the key taken in the round before (lane i holds entry i of the row;
 * entries from 64 on are read again every round), a maximum over the wave by shuffles.  The rest comes from pop_order from its
 * front, 64 a step: a binary search in the row's col drops the members of G_a, a ballot and a prefix count place the others.
 * An entry of col or of pop_order outside [0, P) is skipped and SBADINDEX is raised.
 * Limits: those of mobgt_baseline_ranks, and 1 <= k <= MAX_K -- else EBADDIM. */
int mobgt_baseline_topk(const void* seq, const void* offsets, const void* users, int64_t S, int64_t M, const void* session,
                        const void* cut, int64_t Q, const void* rowptr, const void* col, const void* val, int64_t nnz,
                        const void* ukey, const void* uval, int64_t nnzU, int64_t U, const void* pop_rank, const void* pop_order,
                        int64_t P, int64_t order, int64_t k, void* ids, void* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
