/* C ABI of mobgt_amd/libmobgt_geoprior.so -- a fitted distance-decay prior on a model's next-POI scores: how far the train
 * transitions travelled, as a table over the distance bins of include/mobgt_bins.h, added to the scores on the device.
 *
 * The rule is stated in the docstring of mobgt_amd/geoprior.py (the host forms there are the same rule as plain definitions).  In
 * short: with the [P, 3] f64 unit vectors and the nthr non-decreasing f64 thresholds of a geo.PairBins,
 *     bin(i, j) = #{k : thresholds[k] <= c2(i, j)}   in 0 .. nthr,   B = nthr + 1 bins,
 * c2 the squared chord of include/mobgt_bins.h bit for bit and the count that of csrc_bins/bins_search.h.  Two exact integer
 * histograms over the bins are counted here -- n over all P^2 ordered pairs, t over the entries of the train transition CSR, each
 * weighted by its count -- the host turns them into ONE f32 table (no transcendental runs in a kernel), and the blend adds
 *     out[g, c] = scores[g, c] + w * table[bin(a - 1, p - 1)]
 * where row g has an anchor a (the last entry of hist[g, 0 .. n) that is not 0; an id outside 1 .. P: no anchor) and column c is
 * a POI p = c + label_offset in 1 .. P; the product and the sum are each rounded to f32 on their own (no FMA).  Every other
 * element is copied bit for bit.
 *
 * A library of its own: the other headers and their ABI versions are not touched.  gfx950 code objects only.  Every function is
 * a plain launch sequence on `stream` (the last argument), graph-capturable: no allocation, no host synchronisation, no
 * workgroup waits for another; atomics are on integers only, so no result depends on an order.  Buffers are caller-owned device
 * memory; rows have unit element stride.  Return: 0 on success, one of the MOBGT_GEOPRIOR_E* codes (checked before anything is
 * launched), or a positive hipError_t of a launch.  EVERY element of every output is written by every call: the caller never
 * pre-zeroes anything (the histograms are cleared on `stream` by the call itself); only status[0] is ORed into.  A pointer to a
 * buffer of zero elements may be null.  An index read from a buffer is checked against the size of what it indexes before it is
 * used; what fails is skipped and, in csr_hist, flagged in status[0].
 */
#ifndef MOBGT_GEOPRIOR_H
#define MOBGT_GEOPRIOR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGT_GEOPRIOR_EBADDIM (-1)   /* a size or a parameter outside the limits                            */
#define MOBGT_GEOPRIOR_EALIGN (-2)    /* a pointer that is null or not aligned to its element type           */
#define MOBGT_GEOPRIOR_EDTYPE (-3)    /* hist_dtype is not one of the two below                              */

/* hist_dtype */
#define MOBGT_GEOPRIOR_I32 0
#define MOBGT_GEOPRIOR_I64 1

/* threads of every workgroup of this library */
#define MOBGT_GEOPRIOR_THREADS 256

/* pair_hist: columns whose unit vectors a workgroup keeps in LDS at a time (24 KB), and the rows a workgroup owns */
#define MOBGT_GEOPRIOR_TILE 1024
#define MOBGT_GEOPRIOR_ROWS 16

/* pair_hist: up to this many bins a workgroup counts in a 32-bit histogram of its own in LDS, beside the 16 KB of coarse
 * thresholds and the tile (4 * 28672 + 16384 + 24576 = 155 648 of a CU's 163 840 bytes); with more bins (B = 32 768 would need
 * 172 032) every count goes to global memory as a 64-bit vector atomic */
#define MOBGT_GEOPRIOR_LDS_BINS 28672

/* csr_hist: CSR rows per workgroup */
#define MOBGT_GEOPRIOR_CSR_ROWS 64

/* blend_rows: columns of a row one workgroup blends -- the grid is (ceil(V / CHUNK), G) -- and the rows of one launch */
#define MOBGT_GEOPRIOR_CHUNK 1024
#define MOBGT_GEOPRIOR_MAX_G 65535

/* bits of status[0]; sticky: the kernel only ORs into the word, the caller zeroes it */
#define MOBGT_GEOPRIOR_SBADINDEX 1    /* a rowptr pair that is descending or lies outside [0, nnz], or an entry of col outside [0, P) */

#define MOBGT_GEOPRIOR_ABI_VERSION 1
int mobgt_geoprior_abi_version(void);

/* counts[b] = #{(i, j) in [0, P)^2 : bin(i, j) = b}: all ordered pairs, the diagonal included (the multiset of
 * mobgt_bins_chord2_digits); the counts sum to P * P.
 * In:  unit [P, 3] f64;  thresholds [nthr] f64, non-decreasing (the caller checks that much on the host; the kernel cannot)
 * Out: counts [nthr + 1] int64, cleared on `stream` by the call itself
 * c2 is exactly symmetric, so each unordered pair i < j is walked once, tile against tile as mobgt_bins_chord2_digits walks
 * them, and counted twice; the P diagonal zeros are added by workgroup 0.  Every `stride`-th threshold sits in LDS (bins_search.h).
 * Limits: 1 <= P <= MOBGT_BINS_MAX_P, MOBGT_BINS_MIN_THRESHOLDS <= nthr <= MOBGT_BINS_MAX_THRESHOLDS -- else EBADDIM. */
int mobgt_geoprior_pair_hist(const void* unit, int64_t P, const void* thresholds, int nthr, void* counts, void* stream);

/* counts[b] = the sum of val[e] over the entries e of the CSR, e in row a, with bin(a, col[e]) = b; the counts sum to sum(val)
 * where no entry is skipped.
 * In:  unit, thresholds as above
 *      rowptr [P + 1] int64, col [nnz] int32 (0-based POIs), val [nnz] int32       the train transition CSR
 * Out: counts [nthr + 1] int64, cleared on `stream` by the call itself
 *      status [1] int32       SBADINDEX is ORed in with a vector atomic; never cleared here
 * A row whose rowptr pair is descending or lies outside [0, nnz] is skipped, an entry of col outside [0, P) is skipped; both
 * raise SBADINDEX.  A wave per row, CSR_ROWS rows per workgroup; 64-bit vector atomics on counts.
 * Limits: as above and 0 <= nnz < 2^31 -- else EBADDIM. */
int mobgt_geoprior_csr_hist(const void* unit, int64_t P, const void* thresholds, int nthr, const void* rowptr, const void* col,
                            const void* val, int64_t nnz, void* counts, void* status, void* stream);

/* out[g, c] = the blend of scores[g, c] (the rule above).  out == scores (in place, then ld_out == ld_scores) and buffers that
 * do not overlap are both legal.
 * In:  scores [G, >= V] f32, ld_scores elements between rows
 *      hist [G, n_hist_cols] int32 / int64 (hist_dtype), ld_hist elements between rows: POI ids, 0 = padding
 *      unit, thresholds as above;  table [nthr + 1] f32;  weight [1] f32, read on the device
 * Out: out [G, >= V] f32, ld_out elements between rows; columns from V on are left alone
 * A workgroup of THREADS threads per (chunk of CHUNK columns, row).  It stages the coarse thresholds and finds the row's anchor
 * (the search of mobgt_amd/csrc_prior/blend_rows.h, shared by the three priors), stages the anchor's unit vector, and every thread blends
 * CHUNK / THREADS columns: one f64 chord, one search, one gather from the table.  An element is read and written by the same
 * thread, so in place is safe.
 * Limits: 0 <= G <= MAX_G; 0 <= V, n_hist_cols < 2^31; P and nthr as above; ld_scores, ld_out >= V; ld_hist >= n_hist_cols;
 * label_offset 0 or 1; out == scores only with ld_out == ld_scores -- else EBADDIM.  G = 0 or V = 0: nothing is launched. */
int mobgt_geoprior_blend_rows(const float* scores, int64_t ld_scores, float* out, int64_t ld_out, int64_t G, int64_t V,
                              int64_t label_offset, const void* hist, int hist_dtype, int64_t ld_hist, int64_t n_hist_cols,
                              const void* unit, int64_t P, const void* thresholds, int nthr, const float* table,
                              const float* weight, void* stream);

#ifdef __cplusplus
}
#endif
#endif
