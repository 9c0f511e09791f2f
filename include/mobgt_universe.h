/* C ABI of mobgt_amd/libmobgt_universe.so -- the POI table's counts and the two transition graphs from check-in SESSIONS, on the
 * device.
 *
 * The reference derives three inputs of Graphormer.__init__ from the check-in sessions on the host
 * (graphormer/foursquare_process.py): the Graph_poi.csv columns checkin_cnt, cat and the category frequency
 * (build_users_locations_dict, :262-294), Graph_cat.csv (:654-668) and Graph_adj.csv (:678-687, both in prepare_global_data, one
 * pandas .loc increment per transition into dense num_cat^2 and P^2 frames).  All are plain counts.  This library counts them
 * from the packed check-ins mobgt_amd.data.SessionDataset holds: the small spaces (POIs, categories, category pairs) with integer
 * atomics, the P^2 space of POI pairs as one 64-bit key per transition, which the caller sorts and mobgt_universe_run_heads /
 * mobgt_universe_run_fill turn into a CSR -- nothing of size P^2 exists anywhere.
 *
 * Ids are dense: POIs 1 .. P and categories 1 .. n_cat (the reference's vid_list / catid_list numbering).  Every count is an
 * integer atomic or a plain store: the results are exact and independent of the order of execution.
 *
 * A library of its own: the other headers and their ABI versions are not touched.  gfx950 code objects only.  Plain launches on
 * `stream` (the last argument): no allocation, no host synchronisation, no workgroup waits for another.  Buffers are caller-owned
 * device memory, C-contiguous.  Return: 0 on success, one of the MOBGT_UNIVERSE_E* codes (checked before anything is launched),
 * or a positive hipError_t of a launch.  EVERY element of every output is written by every call: the caller never pre-zeroes
 * anything.  A pointer to a buffer of zero elements may be null.
 */
#ifndef MOBGT_UNIVERSE_H
#define MOBGT_UNIVERSE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_UNIVERSE_EBADDIM (-1)   /* a size outside the limits                                           */
#define MOBGT_UNIVERSE_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */

/* limits: P^2 must fit a 63-bit key with room to spare; n_cat int32 counters must fit a workgroup's LDS beside graph_cat's, and
 * n_cat^2 int32 counters are one buffer (64 MB at the limit) */
#define MOBGT_UNIVERSE_MAX_P 1000000
#define MOBGT_UNIVERSE_MAX_CAT 4096

/* mobgt_universe_counts keeps a workgroup's category counts in LDS (integer atomics there, one flush per workgroup): cat_cnt
 * always (16 KB at MOBGT_UNIVERSE_MAX_CAT), graph_cat while n_cat <= MOBGT_UNIVERSE_LDS_MAX_CAT (4 * 96^2 = 36 KB of a
 * workgroup's 64 KB).  Above that threshold graph_cat takes global integer atomics.  The result is the same either way. */
#define MOBGT_UNIVERSE_LDS_MAX_CAT 96

/* check-ins one workgroup of mobgt_universe_counts owns (a contiguous chunk of the packed array) */
#define MOBGT_UNIVERSE_CHUNK 4096

/* bits of status[0] of mobgt_universe_counts */
#define MOBGT_UNIVERSE_SBADPOI 1      /* a POI id outside 1 .. P                                             */
#define MOBGT_UNIVERSE_SBADCAT 2      /* a category id outside 1 .. n_cat                                    */
#define MOBGT_UNIVERSE_SBADSESSION 4  /* sid[i] outside 0 .. S - 1, or a key slot outside 0 .. T - 1         */

#define MOBGT_UNIVERSE_ABI_VERSION 1
int mobgt_universe_abi_version(void);

/* foursquare_process.py:276-289 (the check-in counts of POIs and categories), :293 (a POI's category), :654-668 (Graph_cat)
 * and the transitions of :678-687 (Graph_adj), for M packed check-ins of S sessions.
 *
 * In:  seq [M, 3] int32   check-ins in visit order, session after session: rows (poi, time slot, category); the slot is not read
 *      sid [M] int32      the session of every check-in, non-decreasing (np.repeat(arange(S), lengths))
 *      first [S] int32    the index of session s's first check-in
 *      slot0 [S] int32    -1: not a train session, its transitions are not counted.  Else the slot of its first transition in
 *                         `keys`: the exclusive prefix sum of (length - 1) over the train sessions, so T = their sum is known
 *                         on the host before the launch
 * Out: checkin_cnt [P] int32      check-ins at POI p over ALL sessions (:279-282)
 *      cat_cnt [n_cat] int32      check-ins of category c over ALL sessions (:284-289)
 *      poi_cat_min, poi_cat_max [P] int32   the smallest and the largest category seen at POI p; INT32_MAX and 0 for a POI
 *                                 without a check-in.  Equal where the POI has one category, which is then its `cat` (:293-294)
 *      graph_cat [n_cat, n_cat] int32   graph_cat[a - 1, b - 1] = consecutive check-in pairs (i - 1, i) inside one TRAIN
 *                                 session with categories a -> b (:654-668)
 *      keys [T] int64             for the transition into check-in i of train session s, keys[slot0[s] + i - first[s] - 1] =
 *                                 (p - 1) * P + (q - 1), p -> q its POIs (:685-687); -1 where a transition was skipped
 *      status [1] int32           0, or MOBGT_UNIVERSE_S* bits
 * Check-in i forms a transition with i - 1 only if sid[i - 1] == sid[i]: no pair spans two sessions.  Self transitions count
 * (the diagonal), nothing is clipped.  An id outside 1 .. P / 1 .. n_cat is NEVER used as an index: the check-in is skipped,
 * with the transitions it is part of, and its bit is raised in status; so are a sid outside 0 .. S - 1 and a slot outside
 * 0 .. T - 1.  With status = 0 every key is in 0 .. P^2 - 1.
 *
 * Two launches: a fill of every output (zeros; INT32_MAX for poi_cat_min; -1 for keys), then ONE launch over the check-ins,
 * ceil(M / MOBGT_UNIVERSE_CHUNK) workgroups of 256 threads, workgroup b owning check-ins b * CHUNK .. + CHUNK - 1 (it reads
 * check-in b * CHUNK - 1 for the transition across its edge).  checkin_cnt, poi_cat_min / max: global integer atomics.
 * cat_cnt: LDS integer atomics and one flush of the non-zero counters per workgroup; graph_cat: the same up to the threshold
 * above, global integer atomics beyond.  keys: plain 8-byte stores.  M = 0 launches the fill only.
 *
 * Limits: 0 <= M < 2^31, 0 <= S, 0 <= T < 2^31, 1 <= P <= MOBGT_UNIVERSE_MAX_P, 1 <= n_cat <= MOBGT_UNIVERSE_MAX_CAT -- else
 * MOBGT_UNIVERSE_EBADDIM; a null (with a non-zero size) or misaligned pointer: MOBGT_UNIVERSE_EALIGN. */
int mobgt_universe_counts(const void* seq, const void* sid, int64_t M, const void* first, const void* slot0, int64_t S, int64_t P,
                          int n_cat, void* checkin_cnt, void* cat_cnt, void* poi_cat_min, void* poi_cat_max, void* graph_cat,
                          void* keys, int64_t T, void* status, void* stream);

/* The first of the two launches that turn the SORTED keys into the CSR of Graph_adj (:678-687): marks where a run of equal
 * keys begins.
 *
 * In:  keys [T] int64   ascending (torch.sort of mobgt_universe_counts' keys)
 * Out: head [T] int32   1 where i = 0 or keys[i] != keys[i - 1], else 0.  Every element is written.
 * One launch, one thread per key.  The caller's inclusive prefix sum of `head` (torch.cumsum, int64) is `pos`, below; its last
 * element is nnz.  Limits: 1 <= T < 2^31 -- else MOBGT_UNIVERSE_EBADDIM. */
int mobgt_universe_run_heads(const void* keys, int64_t T, void* head, void* stream);

/* The second: the CSR itself.
 *
 * In:  keys [T] int64   ascending, every key in 0 .. P^2 - 1
 *      pos [T] int64    the inclusive prefix sum of mobgt_universe_run_heads' output: pos[i] - 1 is the run of key i
 * Out: rowptr [P + 1] int64   rowptr[r] = number of runs whose key is below r * P (a binary search in keys per row, then pos)
 *      col [nnz] int32        col[k] = key % P of run k: ascending inside a row, because the keys ascend
 *      val [nnz] int32        the length of run k = Graph_adj[key / P, key % P]; the first key of a run finds the run's end by
 *                             a binary search in keys, so a run of any length (beyond 65 535 too) costs one thread log2(T) loads
 * Every element of the three outputs is written, given that pos is what its description says; a run index outside 0 .. nnz - 1
 * is never used as an index (the element is skipped).  One launch, max(T, P + 1) threads.  T = 0: rowptr is all zeros.
 * Limits: 0 <= T < 2^31, 0 <= nnz <= T, 1 <= P <= MOBGT_UNIVERSE_MAX_P -- else MOBGT_UNIVERSE_EBADDIM. */
int mobgt_universe_run_fill(const void* keys, const void* pos, int64_t T, int64_t P, int64_t nnz, void* rowptr, void* col, void* val,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
