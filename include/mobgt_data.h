/* C ABI of mobgt_amd/libmobgt_data.so -- the device half of the data path that starts from check-in SESSIONS.
 *
 * The reference turns a user's session (a visit-ordered list of check-ins, the last one the prediction target) into a
 * trajectory graph on the host, with a pandas loop that increments one cell per transition
 * (graphormer/gen_pickles.py:735-833, gen_poigraph_d1228_nyc_avg_maxtime), and pickles the result; everything downstream
 * (owndata.py:343-357, wrapper.py:25-102, collator.py:310-458) starts from that dict.  This library builds the dict's
 * arrays for a whole padded batch on the device, in the layout mobgt_spd_batched / mobgt_collate_finish of
 * include/mobgt_hip.h read (mobgt_amd.data.RawLayout), so a fresh batch travels to the device as its check-ins -- a few
 * thousand integers -- instead of as dense [N, N] count matrices.
 *
 * A library of its own: the ABI of libmobgt_hip.so (include/mobgt_hip.h) is not touched.  gfx950 code objects only.
 * All functions return 0 on success, one of the MOBGT_DATA_E* codes, or a positive hipError_t of the launch; buffers are
 * caller-owned device memory, C-contiguous.
 */
#ifndef MOBGT_DATA_H
#define MOBGT_DATA_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_DATA_EBADDIM (-1)  /* a size outside the limits below                                     */
#define MOBGT_DATA_EALIGN (-2)   /* a pointer that is null or not 4-byte aligned                        */

/* supported sizes of mobgt_sessions_to_raw (a history of Lp check-ins has at most Lp nodes; the largest shape bucket of
 * mobgt_amd.data.BUCKETS is 1024, longer graphs pad to multiples of 256) */
#define MOBGT_DATA_MAX_LP 4096
#define MOBGT_DATA_MAX_N 4096

/* status[g] of mobgt_sessions_to_raw */
#define MOBGT_DATA_SOK 0
#define MOBGT_DATA_SBADLEN 1     /* len[g] < 1 or len[g] > Lp                                           */
#define MOBGT_DATA_SNODES 2      /* more than N distinct POIs in the history                            */

#define MOBGT_DATA_ABI_VERSION 1
int mobgt_data_abi_version(void);

/* graphormer/gen_pickles.py:755-832 (one iteration of gen_poigraph_d1228_nyc_avg_maxtime's loop over a user's sessions) for
 * G sessions at once, padded as mobgt_amd.data.DeviceCollator.pack_host pads the dicts (collator.py:11-101 padding: zeros).
 *
 * In:  seq [G, Lp, 3] int32  the HISTORY check-ins of session g in visit order, rows (poi, time slot, category); rows at and
 *                            beyond len[g] are never read (:757-760, :774-775: all_traj[:-1], current_time, current_cat)
 *      len [G] int32         history length L of session g, 1 <= L <= Lp
 * Out: n_nodes [G] int32     n = number of distinct POIs of the history (:766, :820)
 *      x [G, N] int32        node a = the POI whose LAST occurrence is the a-th last occurrence in visit order
 *                            (:789-791 drop_duplicates(keep='last'), :821 node_name); node n - 1 is the last check-in's POI
 *      counts [G, N, N] int32  counts[a, b] = number of i in 1 .. L-1 with node(hist[i-1]) = a and node(hist[i]) = b
 *                            (:783-785 the .loc increments, :817-818 the reorder to node order, :822 edge_type); self
 *                            transitions count on the diagonal; nothing is clipped
 *      time, cat [G, N] int32  the values at the node's last occurrence (:786-787 later visits overwrite, :804, :812, :827, :830)
 *      time_normal [G, N] f32  0 if time = 0, else (float)((double)time / 48) (:805-809, then FloatTensor :828)
 *      status [G] int32      MOBGT_DATA_SOK, or why graph g was refused (MOBGT_DATA_S*): its outputs are then all zero and
 *                            n_nodes[g] = 0
 * EVERY element of every output is written by every call, padding (node >= n) as zeros: no buffer needs clearing.  The user
 * id and the target (:824, :829) pass through on the host and are not arguments.
 *
 * One graph-capturable launch of G workgroups; workgroup g owns graph g's outputs, zero-fills them, passes a workgroup
 * barrier and counts (LDS integer atomics for n <= 64, else global integer atomics on its own tile: exact either way).  No
 * workgroup waits for another, no state between calls.  Last occurrences are found by a backward scan per check-in:
 * O(L^2) compares per session in the worst case.  One workgroup also zero-fills its whole N x N tile (4 N^2 bytes: 4 MB at
 * N = 1024, 64 MB at N = 4096); with few sessions per launch that fill, on G compute units, is the likely cost at large N.
 *
 * Limits: 1 <= Lp <= MOBGT_DATA_MAX_LP, 1 <= N <= MOBGT_DATA_MAX_N, 0 <= G (G = 0 launches nothing) -- else
 * MOBGT_DATA_EBADDIM; a null or misaligned pointer: MOBGT_DATA_EALIGN.  POI ids, time slots and categories are any int32. */
int mobgt_sessions_to_raw(const void* seq, const void* len, void* counts, void* x, void* time, void* cat, void* time_normal,
                          void* n_nodes, void* status, int G, int Lp, int N, void* stream);

#ifdef __cplusplus
}
#endif
#endif
