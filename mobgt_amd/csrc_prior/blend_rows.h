// What the blend_rows kernels share (prior.hip, ../csrc_geoprior/geoprior.hip, ../csrc_ctxprior/ctxprior.hip,
// ../csrc_visitprior/visitprior.hip): the leading fields of their row arguments, the anchor search of the three that have an
// anchor, the wave's search in a CSR row, and the argument checks of mobgt_*_blend_rows that all of them make.
//
// THE ANCHOR SEARCH.  The anchor position of row g is the LAST i in [0, n_hist) with hist[g, i] != 0, -1 if there is none.  A
// workgroup of TPB threads finds it in two phases around ONE barrier, which is the caller's:
//     last = anchor_scan<TPB>(in, g, tid, last_of_wave);     thread tid keeps the last such i of tid, tid + TPB, ...; the wave takes
//                                                            the maximum by xor shuffles and lane 0 writes it to last_of_wave[wave]
//     ... whatever else the kernel wants done before the barrier (prior.hip loads its chunk here) ...
//     __syncthreads();
//     last = anchor_max<TPB>(last, last_of_wave);            the maximum over the waves: the same value in every lane
// last_of_wave is TPB / WAVE int32 in LDS.  The position is not yet an anchor: the id there is checked against 1 .. P by the kernel
// before it indexes anything.
#ifndef MOBGT_BLEND_ROWS_H
#define MOBGT_BLEND_ROWS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int WAVE = 64;
constexpr int ROWS_I32 = 0, ROWS_I64 = 1;          // every library's *_I32 / *_I64: each .hip asserts its header's against these

// A kernel's Rows begins with these: struct Rows : BlendRows { int hist64; ... }.  hist64 (the ids are int64) is every Rows' own
// member, because prior.hip keeps it behind its user fields: the three kernels' arguments lie where they always lay.
struct BlendRows {
    const float* scores;
    float* out;
    int64_t ld_scores, ld_out, V, label_offset;
    const void* hist;
    int64_t ld_hist, n_hist;
};

__device__ inline int64_t load_id(const void* p, int wide, int64_t i) {
    return wide ? static_cast<const int64_t*>(p)[i] : static_cast<const int32_t*>(p)[i];
}

// (R: the kernel's Rows, by value as the kernel holds it)
template <int TPB, class R>
__device__ __forceinline__ int32_t anchor_scan(R in, int64_t g, int tid, int32_t* last_of_wave) {
    int32_t last = -1;
    for (int64_t i = tid; i < in.n_hist; i += TPB) {
        if (load_id(in.hist, in.hist64, g * in.ld_hist + i) != 0) last = (int32_t)i;
    }
#pragma unroll
    for (int d = WAVE / 2; d; d /= 2) {
        const int32_t o = __shfl_xor(last, d, WAVE);
        last = o > last ? o : last;
    }
    if (tid % WAVE == 0) last_of_wave[tid / WAVE] = last;
    return last;
}

template <int TPB>
__device__ __forceinline__ int32_t anchor_max(int32_t last, const int32_t* last_of_wave) {
#pragma unroll
    for (int w = 0; w < TPB / WAVE; ++w) last = last_of_wave[w] > last ? last_of_wave[w] : last;
    return last;
}

// THE SEARCH IN A CSR ROW (prior.hip, ../csrc_visitprior/visitprior.hip).  The first i in [lo, hi) with a[i] >= x, hi if there is
// none; a ascending.  By a whole wave: a step probes 64 places of [lo, hi), a lane a place, and keeps the gap between the last
// probe below x and the one after it, so 2^31 elements take six dependent loads where a lane's own bisection takes 31.  Every lane
// of the wave must call it with the same arguments; the result is the same in every lane, and lies in [lo, hi] whatever `a` holds.
template <class T>
__device__ inline int32_t wave_lower(const T* __restrict__ a, int32_t lo, int32_t hi, T x, int lane) {
    while (lo < hi) {
        const int64_t step = ((int64_t)hi - lo + WAVE - 1) / WAVE;
        const int64_t at = lo + lane * step;
        const int below = __popcll(__ballot(at < hi && a[at] < x));    // (ascending: the probes below x are the first `below`)
        if (below == 0) return lo;
        const int64_t last = lo + (below - 1) * step;                   // < hi: that probe was made
        lo = (int32_t)(last + 1);
        hi = (int32_t)(last + step < hi ? last + step : hi);
    }
    return lo;
}

// null only where the buffer has no element
bool bad_ptr(const void* p, uintptr_t align, int64_t n) {
    return (p == nullptr && n > 0) || (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0;
}

bool bad_size(int64_t v) { return v < 0 || v > INT32_MAX; }

bool bad_id_dtype(int d) { return d != ROWS_I32 && d != ROWS_I64; }

// The checks of mobgt_*_blend_rows on what BlendRows holds.  Every entry point keeps the order: its *_EBADDIM conditions with
// bad_rows_dims, then the dtypes (*_EDTYPE), then its pointers with bad_rows_ptrs (*_EALIGN); the codes returned are its own.
bool bad_rows_dims(const BlendRows& in, int64_t G, int64_t max_g) {
    return G < 0 || G > max_g || bad_size(in.V) || bad_size(in.n_hist) || in.ld_scores < in.V || in.ld_out < in.V ||
           in.ld_hist < in.n_hist || in.label_offset < 0 || in.label_offset > 1 ||
           (in.out == in.scores && in.out != nullptr && in.ld_out != in.ld_scores);
}

bool bad_rows_ptrs(const BlendRows& in, int hist64, int64_t G) {
    return bad_ptr(in.scores, 4, G * in.V) || bad_ptr(in.out, 4, G * in.V) || bad_ptr(in.hist, hist64 ? 8 : 4, G * in.n_hist);
}

}  // namespace
#endif
