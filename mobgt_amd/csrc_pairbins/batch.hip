// include/mobgt_pairbins.h: the distance bins of one batch's pairs, where no table of all pairs can exist (P = 100 000).
//
// batch_kernel -- table_kernel's search (../csrc_bins/bins.hip) for the pairs of one batch only (DeviceCollator(pair_bins=)): a
// workgroup owns BROWS rows of one graph's [N, N] block of poi_pos; the graph's POI ids are turned into unit vectors in LDS once
// per workgroup (BTILE columns at a time: one tile while N <= 1024), an id outside 1 .. P is marked there and never used as an
// index.  The thresholds sit in LDS as in table_kernel, and chord2, the search and the store are the one copy both kernels
// include (../csrc_bins/bins_search.h): four int16 of an aligned 8-byte word at once, single elements where a row or a tile
// starts or ends inside a word.
//
// Built with -ffp-contract=off (Makefile): c2 is mobgt_bins.h's bit-exact expression.  No workgroup reads what another writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_bins.h"
#include "mobgt_pairbins.h"
#include "../csrc_bins/bins_search.h"

namespace {

constexpr int TPB = 256;
constexpr int BROWS = 8;                           // rows of one graph per workgroup
constexpr int BTILE = 1024;                        // columns whose unit vectors a workgroup keeps in LDS at a time (24 KB)

// poi_pos[g, a, b] = #{k : thr[k] <= c2(x[g, a] - 1, x[g, b] - 1)} where both ids lie in 1 .. P, 0 elsewhere.  Workgroup
// blockIdx.x owns rows (blockIdx.x % nrb) * BROWS .. + BROWS - 1 of graph blockIdx.x / nrb.
__global__ __launch_bounds__(TPB) void batch_kernel(const double* __restrict__ unit, int64_t P, const double* __restrict__ thr, int nthr,
                                                    int stride, int ncoarse, const int32_t* __restrict__ x, int N, int nrb,
                                                    int16_t* __restrict__ poi_pos) {
    __shared__ double s_c[COARSE];
    __shared__ double s_u[BTILE * 3];                                   // the tile's columns
    __shared__ double s_r[BROWS * 3];                                   // the workgroup's rows
    __shared__ unsigned char s_ok[BTILE], s_rok[BROWS];                 // whether the id is a POI's (1 .. P)
    const int t = threadIdx.x;
    const int64_t g = blockIdx.x / nrb;
    const int a0 = (int)(blockIdx.x % nrb) * BROWS;
    const int32_t* xg = x + g * N;
    for (int q = t; q < ncoarse; q += TPB) s_c[q] = thr[(int64_t)q * stride];
    if (t < BROWS) {
        const int64_t id = a0 + t < N ? (int64_t)xg[a0 + t] : 0;
        const bool ok = id >= 1 && id <= P;
        const int64_t i = ok ? id - 1 : 0;                              // (an id outside 1 .. P is never an index)
        s_rok[t] = ok;
        s_r[3 * t] = unit[3 * i]; s_r[3 * t + 1] = unit[3 * i + 1]; s_r[3 * t + 2] = unit[3 * i + 2];
    }
    const int64_t skew = (int64_t)((reinterpret_cast<uintptr_t>(poi_pos) & 7u) >> 1);       // elements from an 8-byte boundary to poi_pos[0]

    for (int c0 = 0; c0 < N; c0 += BTILE) {
        const int w = N - c0 < BTILE ? N - c0 : BTILE;                  // columns of this tile
        __syncthreads();                                                // (the previous tile has been read)
        for (int q = t; q < w; q += TPB) {
            const int64_t id = xg[c0 + q];
            const bool ok = id >= 1 && id <= P;
            const int64_t j = ok ? id - 1 : 0;
            s_ok[q] = ok;
            s_u[3 * q] = unit[3 * j]; s_u[3 * q + 1] = unit[3 * j + 1]; s_u[3 * q + 2] = unit[3 * j + 2];
        }
        __syncthreads();

        // a row's piece of this tile touches at most (w + VEC - 1) / VEC + 1 words; item = (row, word of the piece)
        const int wpr = (w + VEC - 1) / VEC + 1;
        for (int item = t; item < BROWS * wpr; item += TPB) {
            const int r = item / wpr, a = a0 + r;
            if (a >= N) break;                                          // (rows ascend with the item)
            const int64_t f0 = (g * N + a) * N + c0 + skew, f1 = f0 + w - 1;     // the piece's first and last element, from the boundary
            const int64_t word = f0 / VEC + (item - r * wpr);
            if (word > f1 / VEC) continue;
            const bool rok = s_rok[r];
            const double xa = s_r[3 * r], ya = s_r[3 * r + 1], za = s_r[3 * r + 2];
            int16_t v[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int64_t col = word * VEC + k - f0;                 // within the tile
                v[k] = 0;
                if (rok && col >= 0 && col < w && s_ok[col])
                    v[k] = (int16_t)count_thresholds(s_c, ncoarse, thr, nthr, stride,
                                                     chord2(xa, ya, za, s_u[3 * col], s_u[3 * col + 1], s_u[3 * col + 2]));
            }
            store_vec(poi_pos + (word * VEC - skew), v, word * VEC, f0, f1);
        }
    }
}

bool bad_ptr(const void* p, uintptr_t align) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0; }

}  // namespace

extern "C" int mobgt_pairbins_abi_version(void) { return MOBGT_PAIRBINS_ABI_VERSION; }

extern "C" int mobgt_bins_batch(const void* unit, int64_t P, const void* thresholds, int nthr, const int32_t* x, int G, int N, void* poi_pos,
                                void* stream) {
    if (P < 1 || P > MOBGT_BINS_MAX_P || nthr < MOBGT_BINS_MIN_THRESHOLDS || nthr > MOBGT_BINS_MAX_THRESHOLDS || G < 1 || N < 1 || N > MOBGT_PAIRBINS_MAX_N) return MOBGT_PAIRBINS_EBADDIM;
    const int nrb = (N + BROWS - 1) / BROWS;
    if ((int64_t)G * nrb > INT32_MAX) return MOBGT_PAIRBINS_EBADDIM;        // (one workgroup per BROWS rows of a graph)
    if (bad_ptr(unit, 8) || bad_ptr(thresholds, 8) || bad_ptr(x, 4) || bad_ptr(poi_pos, 2)) return MOBGT_PAIRBINS_EALIGN;
    const int stride = (nthr + COARSE - 1) / COARSE, ncoarse = (nthr + stride - 1) / stride;
    hipLaunchKernelGGL(batch_kernel, dim3((unsigned)(G * nrb)), dim3(TPB), 0, (hipStream_t)stream, (const double*)unit, P,
                       (const double*)thresholds, nthr, stride, ncoarse, x, N, nrb, (int16_t*)poi_pos);
    return (int)hipGetLastError();
}
