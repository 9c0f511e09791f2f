/* C ABI of mobgt_amd/libmobgt_bins.so -- the distance-bin edges and the distance-bin table from coordinates, on the device.
 *
 * The reference un-pickles a (P+1) x (P+1) f64 distance matrix, takes the Freedman-Diaconis bin count from two percentiles and
 * the maximum over all P^2 values (graphormer/collator.py:301-308) and digitizes the matrix against np.histogram's edges
 * (graphormer/collator.py:429-437).  Both are functions of the POI coordinates alone.  This library computes what they need
 * from the [P, 3] f64 unit vectors of mobgt_geo_unit_vectors (include/mobgt_geo.h) without a distance matrix: order statistics
 * of the squared chord by a radix select that stores nothing of size P^2, and the int16 bin table by a search of every pair's
 * squared chord among thresholds the host derives from the edges.
 *
 * THE SQUARED CHORD of pair (i, j) is defined bit for bit.  With u the unit vectors and d* = u_i* - u_j*,
 *     c2(i, j) = ((dx * dx) + (dy * dy)) + (dz * dz)
 * every subtraction, product and sum rounded once to f64, nothing contracted into an FMA.  So c2 is exactly symmetric,
 * c2(i, i) = +0.0, and numpy on the same unit vectors reproduces it bit for bit.  |u_i - u_j|^2 = 4 sin^2(d / 2R): c2 is an
 * increasing function of the great-circle distance, and a non-negative f64 orders as its 64-bit pattern.
 *
 * A library of its own: the ABIs of libmobgt_hip.so, libmobgt_data.so and libmobgt_geo.so are not touched.  gfx950 code objects
 * only.  All functions are plain launches on `stream` (the last argument): no allocation, no host synchronisation, no
 * workgroup waits for another.  Buffers are caller-owned device memory, C-contiguous.  Return: 0 on success, one of the
 * MOBGT_BINS_E* codes (checked before anything is launched), or a positive hipError_t of the launch (the convention of
 * include/mobgt_data.h).  EVERY element of every output is written by every call: the caller never pre-zeroes anything.
 */
#ifndef MOBGT_BINS_H
#define MOBGT_BINS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_BINS_EBADDIM (-1)   /* a size outside the limits below                                     */
#define MOBGT_BINS_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */

/* 1 <= P <= MOBGT_BINS_MAX_P (that of include/mobgt_geo.h): P^2 < 2^49, counts and flat table offsets are 64-bit. */
#define MOBGT_BINS_MAX_P 16777216
/* the radix select descends MOBGT_BINS_DIGIT_BITS bits of the pattern per launch: 64 / 8 = 8 launches per order statistic,
 * whatever P is, and a histogram of MOBGT_BINS_RADIX = 2^8 counts to read back after each */
#define MOBGT_BINS_DIGIT_BITS 8
#define MOBGT_BINS_RADIX 256
/* columns whose unit vectors one workgroup of the select keeps in LDS at a time (48 KB) */
#define MOBGT_BINS_TILE 2048
/* 2 <= nthr <= MOBGT_BINS_MAX_THRESHOLDS: a table entry counts thresholds and is an int16 */
#define MOBGT_BINS_MIN_THRESHOLDS 2
#define MOBGT_BINS_MAX_THRESHOLDS 32767

#define MOBGT_BINS_ABI_VERSION 1
int mobgt_bins_abi_version(void);

/* One level of the radix select that replaces np.percentile(x, [75, 25]), np.max(x) and np.min(x) of
 * graphormer/collator.py:301-308: the histogram of the next digit of the pattern of c2 over the multiset of all P^2 ordered
 * pairs (the P diagonal zeros and both (i, j) and (j, i) included), restricted to the pairs whose pattern starts with `prefix`.
 * In:  unit [P, 3] f64
 *      prefix, prefix_bits    the leading prefix_bits bits of the pattern, as a number (prefix < 2^prefix_bits); prefix_bits
 *                             is a multiple of MOBGT_BINS_DIGIT_BITS, 0 <= prefix_bits <= 64 - MOBGT_BINS_DIGIT_BITS
 * Out: counts [MOBGT_BINS_RADIX] int64   counts[d] = #{(i, j) : pattern(c2(i, j)) >> (64 - prefix_bits - DIGIT_BITS)
 *                                                               == prefix * RADIX + d}
 * counts is cleared on `stream` by the call itself.  The host picks the digit that holds the wanted rank and descends. */
int mobgt_bins_chord2_digits(const void* unit, int64_t P, uint64_t prefix, int prefix_bits, void* counts, void* stream);

/* np.digitize(distance, edges) of graphormer/collator.py:429-437 for every pair at once, from unit vectors and thresholds on
 * c2 (the edges of collator.py:301-308's np.histogram mapped through 4 sin^2(e / 2R) by the host).
 * In:  unit [P, 3] f64
 *      thresholds [nthr] f64  non-decreasing (the caller checks that much on the host; the kernel cannot)
 * Out: table [(P + 1), (P + 1)] int16   for a, b >= 1: table[a, b] = #{k : thresholds[k] <= c2(a - 1, b - 1)}, that is
 *                             np.searchsorted(thresholds, c2, side="right"); row 0 and column 0 (the pad POI, at distance 0
 *                             from every POI) hold #{k : thresholds[k] <= 0.0}
 * table needs the alignment of an int16 only: the kernel stores eight bytes at a time wherever the address allows and single
 * elements at the head and the tail of a row. */
int mobgt_bins_table(const void* unit, int64_t P, const void* thresholds, int nthr, void* table, void* stream);

#ifdef __cplusplus
}
#endif
#endif
