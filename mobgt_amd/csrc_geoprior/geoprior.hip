// include/mobgt_geoprior.h: the distance-decay prior -- two integer histograms over the distance bins, and the fitted table
// blended into a model's scores.  The rule is the docstring of mobgt_amd/geoprior.py; the header repeats it in short.
//
// pair_hist_kernel -- the bins of all P^2 ordered pairs, nothing of size P^2 stored.  The walk is digits_kernel's
// (../csrc_bins/bins.hip): a workgroup of 4 waves owns ROWS consecutive rows, 4 per wave, a row's unit vector in registers; the
// columns' unit vectors pass through LDS in tiles of TILE columns, lane l of a wave takes column 64 b + l; c2 is exactly symmetric,
// so only the pairs i < j are walked and counted twice, and the P diagonal zeros are added by workgroup 0.  In a city most pairs
// of a wave land in a few bins: the lanes that hold the bin of the first remaining lane add once, with the popcount of their
// ballot, up to PEEL times; what is left goes one atomic per lane.  Up to LDS_BINS bins the workgroup counts in a 32-bit histogram
// of its own in LDS (a workgroup's ROWS x P pairs fit it) and flushes the bins that are not empty once, with 64-bit vector
// atomics; with more bins every add is such an atomic on global memory.
//
// csr_hist_kernel -- the bins of the entries of the transition CSR, each weighted by its count: a wave per row, a lane per entry,
// 64-bit vector atomics on global memory (there are nnz entries, not P^2).  A rowptr pair and an entry of col are checked before
// they are used as indices.
//
// blend_kernel -- ONE WORKGROUP PER (CHUNK OF COLUMNS, ROW): the anchor is found as ../csrc_prior/blend_rows.h describes, the
// coarse thresholds and the anchor's unit vector are staged once,
// then a thread blends CHUNK / THREADS columns, each read and written by that thread only, so in place is safe.
//
// Built with -ffp-contract=off (Makefile): c2 is mobgt_bins.h's bit-exact expression, and a term is one product and one sum, each
// rounded on its own.  chord2 and the search are ../csrc_bins/bins_search.h's.  No workgroup reads what another writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_bins.h"
#include "mobgt_geoprior.h"
#include "../csrc_bins/bins_search.h"
#include "../csrc_prior/blend_rows.h"

namespace {

constexpr int TPB = MOBGT_GEOPRIOR_THREADS;
constexpr int WAVES = TPB / WAVE;
constexpr int TILE = MOBGT_GEOPRIOR_TILE;
constexpr int ROWS = MOBGT_GEOPRIOR_ROWS;
constexpr int RPW = ROWS / WAVES;                  // rows per wave (pair_hist_kernel)
constexpr int LDS_BINS = MOBGT_GEOPRIOR_LDS_BINS;
constexpr int CSR_ROWS = MOBGT_GEOPRIOR_CSR_ROWS;
constexpr int CHUNK = MOBGT_GEOPRIOR_CHUNK;
constexpr int PEEL = 4;                            // bins a wave adds with one lane each before the per-lane atomics
constexpr size_t LDS_FIXED = (size_t)(COARSE + TILE * 3) * sizeof(double);
constexpr size_t LDS_MAX = LDS_FIXED + (size_t)LDS_BINS * sizeof(unsigned);
static_assert(TPB % WAVE == 0 && ROWS % WAVES == 0 && TILE % WAVE == 0 && CHUNK % TPB == 0 && CSR_ROWS % WAVES == 0, "whole waves, whole steps");
static_assert((uint64_t)ROWS * MOBGT_BINS_MAX_P < (1ull << 32), "a workgroup's pairs fit a 32-bit count");
static_assert(LDS_MAX <= 160 * 1024, "the histogram fits beside the thresholds and the tile");
static_assert(MOBGT_BINS_MAX_THRESHOLDS + 1 > LDS_BINS, "the global form is reachable");
static_assert(MOBGT_GEOPRIOR_I32 == ROWS_I32 && MOBGT_GEOPRIOR_I64 == ROWS_I64, "blend_rows.h's dtype codes are this header's");

// counts[b] += 2 * #{(i, j), i < j, bin(i, j) = b}, + P at bin(i, i).  Dynamic LDS: COARSE thresholds, the tile, then -- IN_LDS
// only -- nthr + 1 counts.
template <bool IN_LDS>
__global__ __launch_bounds__(TPB) void pair_hist_kernel(const double* __restrict__ unit, int64_t P, const double* __restrict__ thr, int nthr,
                                                        int stride, int ncoarse, unsigned long long* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* s_c = reinterpret_cast<double*>(smem);
    double* s_u = s_c + COARSE;
    unsigned* s_hist = reinterpret_cast<unsigned*>(s_u + TILE * 3);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int B = nthr + 1;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS + wave * RPW;

    if (IN_LDS)
        for (int q = t; q < B; q += TPB) s_hist[q] = 0u;
    for (int q = t; q < ncoarse; q += TPB) s_c[q] = thr[(int64_t)q * stride];
    int64_t row[RPW];
    double xi[RPW], yi[RPW], zi[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        row[r] = row0 + r;
        const int64_t ld = row[r] < P ? row[r] : P - 1;
        xi[r] = unit[3 * ld]; yi[r] = unit[3 * ld + 1]; zi[r] = unit[3 * ld + 2];
    }

    // (the first tile that holds a column right of the workgroup's first row)
    for (int64_t c0 = (int64_t)blockIdx.x * ROWS / TILE * TILE; c0 < P; c0 += TILE) {
        const int64_t n_tile = (P - c0 < TILE ? P - c0 : TILE) * 3;     // doubles of this tile
        __syncthreads();                                                // (the previous tile has been read; s_c and s_hist are set)
        for (int64_t q = t; q < n_tile; q += TPB) s_u[q] = unit[c0 * 3 + q];
        __syncthreads();

        for (int b = 0; b < TILE / 64; ++b) {
            if (c0 + 64 * b >= P) break;                                // (uniform)
            if (c0 + 64 * b + 63 <= row0) continue;                     // (uniform in the wave: no column right of any of its rows)
            const int64_t j = c0 + 64 * b + lane;
            const bool in = j < P;
            const int jl = in ? 64 * b + lane : 0;                      // (never read LDS words the tile did not fill)
            const double xj = s_u[3 * jl], yj = s_u[3 * jl + 1], zj = s_u[3 * jl + 2];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const bool mine = in && j > row[r] && row[r] < P;
                int bin = 0;
                if (mine) bin = count_thresholds(s_c, ncoarse, thr, nthr, stride, chord2(xi[r], yi[r], zi[r], xj, yj, zj));    // in 0 .. nthr
                unsigned long long rem = __ballot(mine);
                for (int it = 0; it < PEEL && rem != 0ull; ++it) {      // (uniform in the wave)
                    const int leader = __ffsll((long long)rem) - 1;
                    const int b0 = __builtin_amdgcn_readlane(bin, leader);
                    const unsigned long long m = __ballot(mine && bin == b0) & rem;
                    if (lane == leader) {
                        if (IN_LDS) atomicAdd(&s_hist[b0], (unsigned)__popcll(m));
                        else atomicAdd(&counts[b0], 2ull * (unsigned long long)__popcll(m));
                    }
                    rem &= ~m;
                }
                if ((rem >> lane) & 1ull) {
                    if (IN_LDS) atomicAdd(&s_hist[bin], 1u);
                    else atomicAdd(&counts[bin], 2ull);
                }
            }
        }
    }
    __syncthreads();
    if (IN_LDS)
        for (int q = t; q < B; q += TPB) {
            const unsigned v = s_hist[q];
            if (v != 0u) atomicAdd(&counts[q], 2ull * v);               // (i, j) and (j, i)
        }
    if (blockIdx.x == 0 && t == 0)                                      // c2(i, i) = +0.0
        atomicAdd(&counts[count_thresholds(s_c, ncoarse, thr, nthr, stride, 0.0)], (unsigned long long)P);
}

// counts[bin(a, col[e])] += val[e] for the entries e of row a; workgroup blockIdx.x owns rows blockIdx.x * CSR_ROWS .. + CSR_ROWS - 1.
__global__ __launch_bounds__(TPB) void csr_hist_kernel(const double* __restrict__ unit, int64_t P, const double* __restrict__ thr, int nthr,
                                                       int stride, int ncoarse, const int64_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col, const int32_t* __restrict__ val, int64_t nnz,
                                                       unsigned long long* __restrict__ counts, int32_t* __restrict__ status) {
    __shared__ double s_c[COARSE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int q = t; q < ncoarse; q += TPB) s_c[q] = thr[(int64_t)q * stride];
    __syncthreads();
    bool flag = false;
    for (int r = wave; r < CSR_ROWS; r += WAVES) {
        const int64_t a = (int64_t)blockIdx.x * CSR_ROWS + r;
        if (a >= P) break;                                              // (uniform in the wave)
        const int64_t r0 = rowptr[a], r1 = rowptr[a + 1];
        if (r0 < 0 || r1 < r0 || r1 > nnz) {                            // the row is skipped
            flag = flag || lane == 0;
            continue;
        }
        const double xa = unit[3 * a], ya = unit[3 * a + 1], za = unit[3 * a + 2];
        for (int64_t e = r0 + lane; e < r1; e += WAVE) {
            const int64_t q = col[e];
            if (q < 0 || q >= P) {                                      // the entry is skipped
                flag = true;
                continue;
            }
            const int bin = count_thresholds(s_c, ncoarse, thr, nthr, stride, chord2(xa, ya, za, unit[3 * q], unit[3 * q + 1], unit[3 * q + 2]));
            atomicAdd(&counts[bin], (unsigned long long)(long long)val[e]);
        }
    }
    if (flag) atomicOr(status, MOBGT_GEOPRIOR_SBADINDEX);
}

struct Rows : BlendRows { int hist64; };

__global__ __launch_bounds__(TPB) void blend_kernel(Rows in, const double* __restrict__ unit, int64_t P, const double* __restrict__ thr, int nthr,
                                                    int stride, int ncoarse, const float* __restrict__ table, const float* __restrict__ weight) {
    __shared__ double s_c[COARSE];
    __shared__ double s_a[3];
    __shared__ int32_t last_of_wave[WAVES];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.y;
    const int64_t c0 = (int64_t)blockIdx.x * CHUNK;                     // < V
    const int32_t width = (int32_t)(in.V - c0 < CHUNK ? in.V - c0 : CHUNK);
    const float w = weight[0];

    for (int q = tid; q < ncoarse; q += TPB) s_c[q] = thr[(int64_t)q * stride];
    // the anchor: the last entry of the history row that is not 0 (blend_rows.h)
    int32_t last = anchor_scan<TPB>(in, g, tid, last_of_wave);
    __syncthreads();
    last = anchor_max<TPB>(last, last_of_wave);

    // the same in every lane of the workgroup; an id outside 1 .. P is never an index
    const int64_t a = last >= 0 ? load_id(in.hist, in.hist64, g * in.ld_hist + last) : 0;
    const bool anchored = a >= 1 && a <= P;
    if (anchored && tid < 3) s_a[tid] = unit[3 * (a - 1) + tid];
    __syncthreads();
    const double xa = anchored ? s_a[0] : 0.0, ya = anchored ? s_a[1] : 0.0, za = anchored ? s_a[2] : 0.0;

    const float* src = in.scores + g * in.ld_scores + c0;
    float* dst = in.out + g * in.ld_out + c0;
    for (int32_t j = tid; j < width; j += TPB) {
        float s = src[j];
        const int64_t p = c0 + j + in.label_offset;                     // the column's POI, 1-based
        if (anchored && p >= 1 && p <= P) {
            const double* u = unit + 3 * (p - 1);
            const int bin = count_thresholds(s_c, ncoarse, thr, nthr, stride, chord2(xa, ya, za, u[0], u[1], u[2]));     // in 0 .. nthr
            s = __fadd_rn(s, __fmul_rn(w, table[bin]));
        }
        dst[j] = s;
    }
}

bool bad_bins(int64_t P, int nthr) {
    return P < 1 || P > MOBGT_BINS_MAX_P || nthr < MOBGT_BINS_MIN_THRESHOLDS || nthr > MOBGT_BINS_MAX_THRESHOLDS;
}

// more than the default 64 KB of dynamic LDS needs the attribute once per function (not a stream operation)
int lds_opt_in() {
    static const int rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(pair_hist_kernel<true>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
    return rc;
}

}  // namespace

extern "C" int mobgt_geoprior_abi_version(void) { return MOBGT_GEOPRIOR_ABI_VERSION; }

extern "C" int mobgt_geoprior_pair_hist(const void* unit, int64_t P, const void* thresholds, int nthr, void* counts, void* stream) {
    if (bad_bins(P, nthr)) return MOBGT_GEOPRIOR_EBADDIM;
    const int B = nthr + 1;
    if (bad_ptr(unit, 8, P * 3) || bad_ptr(thresholds, 8, nthr) || bad_ptr(counts, 8, B)) return MOBGT_GEOPRIOR_EALIGN;
    const int stride = (nthr + COARSE - 1) / COARSE, ncoarse = (nthr + stride - 1) / stride;
    const bool in_lds = B <= LDS_BINS;
    if (in_lds) {
        const int rc = lds_opt_in();
        if (rc != 0) return rc;
    }
    const hipError_t rc = hipMemsetAsync(counts, 0, (size_t)B * sizeof(unsigned long long), (hipStream_t)stream);
    if (rc != hipSuccess) return (int)rc;
    const dim3 grid((unsigned)((P + ROWS - 1) / ROWS));
    if (in_lds)
        hipLaunchKernelGGL(pair_hist_kernel<true>, grid, dim3(TPB), LDS_FIXED + (size_t)B * sizeof(unsigned), (hipStream_t)stream,
                           (const double*)unit, P, (const double*)thresholds, nthr, stride, ncoarse, (unsigned long long*)counts);
    else
        hipLaunchKernelGGL(pair_hist_kernel<false>, grid, dim3(TPB), LDS_FIXED, (hipStream_t)stream, (const double*)unit, P,
                           (const double*)thresholds, nthr, stride, ncoarse, (unsigned long long*)counts);
    return (int)hipGetLastError();
}

extern "C" int mobgt_geoprior_csr_hist(const void* unit, int64_t P, const void* thresholds, int nthr, const void* rowptr, const void* col,
                                       const void* val, int64_t nnz, void* counts, void* status, void* stream) {
    if (bad_bins(P, nthr) || bad_size(nnz)) return MOBGT_GEOPRIOR_EBADDIM;
    const int B = nthr + 1;
    if (bad_ptr(unit, 8, P * 3) || bad_ptr(thresholds, 8, nthr) || bad_ptr(rowptr, 8, P + 1) || bad_ptr(col, 4, nnz) ||
        bad_ptr(val, 4, nnz) || bad_ptr(counts, 8, B) || bad_ptr(status, 4, 1))
        return MOBGT_GEOPRIOR_EALIGN;
    const int stride = (nthr + COARSE - 1) / COARSE, ncoarse = (nthr + stride - 1) / stride;
    const hipError_t rc = hipMemsetAsync(counts, 0, (size_t)B * sizeof(unsigned long long), (hipStream_t)stream);
    if (rc != hipSuccess) return (int)rc;
    hipLaunchKernelGGL(csr_hist_kernel, dim3((unsigned)((P + CSR_ROWS - 1) / CSR_ROWS)), dim3(TPB), 0, (hipStream_t)stream,
                       (const double*)unit, P, (const double*)thresholds, nthr, stride, ncoarse, (const int64_t*)rowptr, (const int32_t*)col,
                       (const int32_t*)val, nnz, (unsigned long long*)counts, (int32_t*)status);
    return (int)hipGetLastError();
}

extern "C" int mobgt_geoprior_blend_rows(const float* scores, int64_t ld_scores, float* out, int64_t ld_out, int64_t G, int64_t V,
                                         int64_t label_offset, const void* hist, int hist_dtype, int64_t ld_hist, int64_t n_hist_cols,
                                         const void* unit, int64_t P, const void* thresholds, int nthr, const float* table,
                                         const float* weight, void* stream) {
    const Rows in = {{scores, out, ld_scores, ld_out, V, label_offset, hist, ld_hist, n_hist_cols}, hist_dtype == MOBGT_GEOPRIOR_I64};
    if (bad_rows_dims(in, G, MOBGT_GEOPRIOR_MAX_G) || bad_bins(P, nthr)) return MOBGT_GEOPRIOR_EBADDIM;
    if (bad_id_dtype(hist_dtype)) return MOBGT_GEOPRIOR_EDTYPE;
    if (bad_rows_ptrs(in, in.hist64, G) || bad_ptr(unit, 8, P * 3) || bad_ptr(thresholds, 8, nthr) || bad_ptr(table, 4, nthr + 1) || bad_ptr(weight, 4, 1))
        return MOBGT_GEOPRIOR_EALIGN;
    if (G == 0 || V == 0) return 0;
    const int stride = (nthr + COARSE - 1) / COARSE, ncoarse = (nthr + stride - 1) / stride;
    const dim3 grid((unsigned)((V + CHUNK - 1) / CHUNK), (unsigned)G);
    hipLaunchKernelGGL(blend_kernel, grid, dim3(TPB), 0, (hipStream_t)stream, in, (const double*)unit, P, (const double*)thresholds, nthr,
                       stride, ncoarse, table, weight);
    const hipError_t err = hipGetLastError();
    return err != hipSuccess ? (int)err : 0;
}
