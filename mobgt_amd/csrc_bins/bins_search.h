// Device functions of the distance-bin search, shared by table_kernel (bins.hip) and batch_kernel (../csrc_pairbins/batch.hip):
// the squared chord of include/mobgt_bins.h, the count of thresholds at or below it, and the store of four int16 of one aligned
// 8-byte word.  Every file that includes this is built with -ffp-contract=off: chord2 is the header's bit-exact expression.
#ifndef MOBGT_BINS_SEARCH_H
#define MOBGT_BINS_SEARCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int COARSE = 2048;                       // thresholds a workgroup keeps in LDS
constexpr int VEC = 4;                             // int16 per lane and store

// The header's c2: every operation rounded once (contraction is off for this file).
__device__ __forceinline__ double chord2(double xi, double yi, double zi, double xj, double yj, double zj) {
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// #{k : thr[k] <= c2}: s_c holds every `stride`-th threshold (ncoarse of them, in LDS); a pair searches those, then the
// stride - 1 thresholds between two of them in global memory.
__device__ __forceinline__ int count_thresholds(const double* s_c, int ncoarse, const double* __restrict__ thr, int nthr, int stride,
                                                double c2) {
    int lo = 0, hi = ncoarse;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_c[mid] <= c2) lo = mid + 1; else hi = mid;
    }
    if (stride == 1 || lo == 0) return lo;
    // thr[(lo - 1) * stride] <= c2, and c2 < thr[lo * stride] if there is one
    int a = (lo - 1) * stride + 1, b = lo * stride < nthr ? lo * stride : nthr;
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (thr[mid] <= c2) a = mid + 1; else b = mid;
    }
    return a;
}

// Four int16 that share an aligned 8-byte word: one store if [f0, f1] (elements counted from the 8-byte boundary) holds the
// whole word e0 .. e0 + 3, single elements otherwise.  dst: the word's address.
__device__ __forceinline__ void store_vec(int16_t* dst, const int16_t (&v)[VEC], int64_t e0, int64_t f0, int64_t f1) {
    if (e0 >= f0 && e0 + VEC - 1 <= f1) {
        uint2 w;
        w.x = (uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16);
        w.y = (uint32_t)(uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16);
        *reinterpret_cast<uint2*>(dst) = w;
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (e0 + k >= f0 && e0 + k <= f1) dst[k] = v[k];
    }
}

}  // namespace
#endif
