/* C ABI of mobgt_amd/libmobgt_geo.so -- the within-radius POI graph from coordinates, on the device.
 *
 * The reference computes Graph_dist.csv, the 0/1 "within 3 km" matrix the distance GCN runs on, with a Python double loop over
 * all P^2 POI pairs: one LLs2Dist call (graphormer/foursquare_process.py:15-23, the haversine great-circle distance with
 * R = 6371 km) and up to two pandas .loc writes per pair (graphormer/foursquare_process.py:689-702, `if dist<=3 and dist>0`).
 * This library decides the same pairs on the device and writes the result in the two forms the GCN kernels of
 * libmobgt_hip.so read: the bit words of modelGNN.MaskAdj (csrc/maskgemm.hip) and the CSR of modelGNN.CsrAdj (csrc/spmm.hip).
 *
 * MEMBERSHIP.  Pair (i, j), i != j, is an edge iff 0 < d(i, j) <= r.  It is decided in f64 on unit vectors
 * u = (cos lat cos lon, cos lat sin lon, sin lat): |u_i - u_j|^2 = 4 sin^2(d / 2R), so the test is
 *     0 < (x_i - x_j)^2 + (y_i - y_j)^2 + (z_i - z_j)^2 <= chord2_max,      chord2_max = 4 sin^2(r / 2R) from the host.
 * The squared differences are formed component by component and summed in the order x, y, z: swapping i and j negates each
 * difference exactly, so the test is exactly symmetric whatever is contracted into FMAs.  POIs with identical coordinates
 * have identical unit vectors, chord^2 = 0, and are not neighbours -- as in the reference (`dist>0`).
 *
 * A library of its own: the ABIs of libmobgt_hip.so and libmobgt_data.so are not touched.  gfx950 code objects only.
 * All functions are plain launches on `stream` (the last argument): no allocation, no host synchronisation, no workgroup
 * waits for another.  Buffers are caller-owned device memory, C-contiguous.  Return: 0 on success, one of the MOBGT_GEO_E*
 * codes, or a positive hipError_t of the launch (the convention of include/mobgt_data.h).  EVERY element of every output is
 * written by every call.
 */
#ifndef MOBGT_GEO_H
#define MOBGT_GEO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_GEO_EBADDIM (-1)   /* a size outside the limits below                                     */
#define MOBGT_GEO_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */

/* 1 <= P <= MOBGT_GEO_MAX_P: column indices are int32, and P * W * 4 bytes of words (W <= P / 32 + 4) stay far below 2^63.
 * nnz = rowptr[P] is an int64 like every CSR offset. */
#define MOBGT_GEO_MAX_P 16777216
/* columns one wave walks per step of its row: 64 lanes x one 32-bit word (the LDS tile of column unit vectors) */
#define MOBGT_GEO_TILE 2048

#define MOBGT_GEO_ABI_VERSION 1
int mobgt_geo_abi_version(void);

/* The operands of LLs2Dist (graphormer/foursquare_process.py:15-23), once per POI instead of once per pair.
 * In:  coords_deg [P, 2] f64  latitude, longitude in degrees (radians = deg * pi / 180, :17-18, :20)
 * Out: unit [P, 3] f64        (cos lat cos lon, cos lat sin lon, sin lat) */
int mobgt_geo_unit_vectors(const void* coords_deg, void* unit, int64_t P, void* stream);

/* graphormer/foursquare_process.py:689-702 as bit words (distances as :15-23).
 * In:  unit [P, 3] f64, chord2_max
 * Out: words [P, W] int32, W = ceil(P / 128) * 4 (MaskAdj.from_dense01's row pitch): bit j of row i (bit j % 32 of word
 *                             j / 32, little-endian bit order) is set iff (i, j) is an edge or i == j -- A + I, what
 *                             MaskAdj.mask holds; bits at columns >= P are zero
 *      deg [P] int32          number of edges of row i (the diagonal not counted) */
int mobgt_geo_radius_words(const void* unit, int64_t P, double chord2_max, void* words, void* deg, void* stream);

/* The same test (graphormer/foursquare_process.py:15-23, :689-702), only the degrees: nothing of size P^2 is stored.
 * Out: deg [P] int32 */
int mobgt_geo_radius_count(const void* unit, int64_t P, double chord2_max, void* deg, void* stream);

/* graphormer/foursquare_process.py:689-702 (distances as :15-23) as the CSR of the normalised adjacency (D+I)^-1 (A+I)
 * that model_fqandtoyo.py:211-214 builds from it.
 * In:  unit [P, 3] f64, chord2_max
 *      rowptr [P + 1] int64   the exclusive prefix sum of deg + 1 (deg from mobgt_geo_radius_count / _words), rowptr[0] = 0
 * Out: col [nnz] int32        row i: its neighbours and i itself, ascending, at rowptr[i] .. rowptr[i + 1] - 1
 *      val [nnz] f32          every value of row i is (float)(1.0 / (deg_i + 1.0)) = (float)(1.0 / (rowptr[i+1] - rowptr[i]))
 * nnz = rowptr[P].  A row never writes at or beyond rowptr[i + 1]: with a non-decreasing rowptr whose last element is the
 * size of col and val, no store leaves the buffers even if rowptr does not belong to these coordinates (the caller checks
 * that much on the host; the kernel cannot). */
int mobgt_geo_radius_fill(const void* unit, int64_t P, double chord2_max, const void* rowptr, void* col, void* val, void* stream);

#ifdef __cplusplus
}
#endif
#endif
