/* C ABI of mobgt_amd/libmobgt_pairbins.so -- the distance bins of one batch's pairs, on the device.
 *
 * include/mobgt_bins.h builds poi_pos = np.digitize(distance, edges) (graphormer/collator.py:429-437) for all P^2 pairs at once,
 * as a table.  Where no table of all pairs can exist (P = 100 000) this library runs the same search for the pairs of one batch
 * only: one launch, so a collator can issue it on a copy stream beside a step.  THE SQUARED CHORD c2 is the one
 * include/mobgt_bins.h defines bit for bit, the limits on P and on the number of thresholds are that header's
 * (MOBGT_BINS_MAX_P, MOBGT_BINS_MIN_THRESHOLDS .. MOBGT_BINS_MAX_THRESHOLDS), and the search is the table kernel's own code
 * (mobgt_amd/csrc_bins/bins_search.h).
 *
 * A library of its own: include/mobgt_bins.h, the other headers and their ABI versions are not touched.  gfx950 code objects
 * only.  A plain launch on `stream` (the last argument): no allocation, no host synchronisation, no workgroup waits for
 * another.  Buffers are caller-owned device memory, C-contiguous.  Return: 0 on success, one of the MOBGT_PAIRBINS_E* codes
 * (checked before anything is launched), or a positive hipError_t of the launch.  EVERY element of the output is written by every
 * call: the caller never pre-zeroes anything.
 */
#ifndef MOBGT_PAIRBINS_H
#define MOBGT_PAIRBINS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_PAIRBINS_EBADDIM (-1)   /* a size outside the limits                                           */
#define MOBGT_PAIRBINS_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */

/* the padded node count of a batch */
#define MOBGT_PAIRBINS_MAX_N 32768

#define MOBGT_PAIRBINS_ABI_VERSION 1
int mobgt_pairbins_abi_version(void);

/* In:  unit [P, 3] f64        row i is POI i + 1 (mobgt_geo_unit_vectors)
 *      thresholds [nthr] f64  on the device, non-decreasing (the caller checks that much on the host; the kernel cannot)
 *      x [G, N] int32         POI ids, 0 = pad; 1 <= G, 1 <= N <= MOBGT_PAIRBINS_MAX_N, G * ceil(N / 8) < 2^31
 * Out: poi_pos [G, N, N] int16   for x[g, a] and x[g, b] both in 1 .. P:
 *                                poi_pos[g, a, b] = #{k : thresholds[k] <= c2(x[g, a] - 1, x[g, b] - 1)};
 *                                every other pair (a pad, an id outside 1 .. P) holds 0, what mobgt_collate_finish
 *                                (include/mobgt_hip.h) writes for a pair that is not real.  An id outside 1 .. P is never used
 *                                as an index.
 * poi_pos needs the alignment of an int16 only (a view into a byte buffer, N may be odd): eight bytes are stored at a time
 * wherever the address allows, single elements at the head and the tail of a row. */
int mobgt_bins_batch(const void* unit, int64_t P, const void* thresholds, int nthr, const int32_t* x, int G, int N, void* poi_pos,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
