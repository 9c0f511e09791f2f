// Per-row candidate words from coordinates (mobgt_near_words): "the POIs within r of where this row's user is", as the allow words
// [G, ld_words] that mobgt_topk_rows_masked_rows / mobgt_rank_metrics_masked_rows read (cand_body.h, ld_allow > 0).
//
// Contract (include/mobgt_hip.h): column c of row g is near when an anchor a of the row has
//     ((dx*dx) + (dy*dy)) + (dz*dz) <= chord2_max,    dx = pos[c].x - pos[a].x, ...
// in f32, every operation rounded on its own (__fsub_rn / __fmul_rn / __fadd_rn: hipcc would contract the sums into FMAs, and a
// torch statement of the rule could then not reproduce the bits).  pos holds unit vectors, so the squared chord orders pairs as
// the great-circle distance does; a column without a POI is +inf and compares false against everything (inf - inf = NaN too).
//
// One launch, grid (column ranges, G): a workgroup owns NEAR_COLS columns of one row, each lane NEAR_ITERS of them in registers
// (coalesced 16-byte loads of pos).  The row's anchors are staged in LDS NEAR_CHUNK ids at a time -- thread j gathers the unit
// vector of id j of the chunk, +inf for padding and ids outside [0, V) -- and every lane walks the staged vectors (one LDS
// broadcast read per anchor).  A wave leaves the walk once all of its columns are near.  A 64-lane ballot per (wave, step) is two
// output words, ANDed with the shared allow words when given.  Plain stores only, every word of [0, ceil(V / 32)) written, no
// state between calls and no workgroup waiting for another: a captured graph replays the launch freely.
#include "common.h"
#include "../../include/mobgt_hip.h"

namespace {

constexpr int NEAR_THREADS = 256;                  // 4 waves
constexpr int NEAR_ITERS = 2;                      // columns per lane
constexpr int NEAR_COLS = NEAR_THREADS * NEAR_ITERS;   // 512 columns = 16 words per workgroup
constexpr int NEAR_CHUNK = NEAR_THREADS;           // anchors staged per round, one per thread
constexpr int NEAR_POLL = 8;                       // anchors between two looks at "is the whole wave near already"

__device__ __forceinline__ int64_t near_id(const void* hist, int i64, int64_t at) {
    return i64 ? reinterpret_cast<const int64_t*>(hist)[at] : (int64_t)reinterpret_cast<const int32_t*>(hist)[at];
}

__device__ __forceinline__ bool near_pred(const float4& c, const float4& a, float chord2_max) {
    const float dx = __fsub_rn(c.x, a.x), dy = __fsub_rn(c.y, a.y), dz = __fsub_rn(c.z, a.z);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return d2 <= chord2_max;                       // (false on NaN: a column or an anchor without a POI)
}

template <bool ANY>
__global__ __launch_bounds__(NEAR_THREADS) void near_words_kernel(const float4* __restrict__ pos, int64_t V, const void* __restrict__ hist,
                                                                  int i64, int64_t ld_hist, int64_t n_hist, int64_t hist_offset,
                                                                  float chord2_max, const uint32_t* __restrict__ allow_and,
                                                                  uint32_t* __restrict__ words, int64_t ld_words) {
    __shared__ float4 s_a[NEAR_CHUNK];
    __shared__ int s_cnt[2];                       // ANY: staged anchors of the chunk that matter (last valid + 1), by round parity
    __shared__ int s_last;                         // LAST: index of the row's last valid id, -1 = none
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t g = blockIdx.y, W = (V + 31) / 32;
    const int64_t base = (int64_t)blockIdx.x * NEAR_COLS;
    const float inf = __builtin_inff();

    float4 pc[NEAR_ITERS];
    bool near[NEAR_ITERS];
#pragma unroll
    for (int i = 0; i < NEAR_ITERS; ++i) {
        const int64_t c = base + (i * (NEAR_THREADS / 64) + w) * 64 + lane;
        pc[i] = c < V ? pos[c] : make_float4(inf, inf, inf, 0.f);
        near[i] = false;
    }

    if constexpr (ANY) {
        int par = 0;
        for (int64_t j0 = 0; j0 < n_hist; j0 += NEAR_CHUNK, par ^= 1) {
            // Two counters, alternating: a wave may still be about to read the previous round's counter (nothing but that
            // round's second barrier lies behind it) while thread 0 is already here.  The counter reset here was last read two
            // rounds ago, and both barriers of the previous round lie between that read and this store.
            if (threadIdx.x == 0) s_cnt[par] = 0;
            __syncthreads();                       // (the previous chunk's s_a has been read; the reset is visible to the atomics)
            const int64_t j = j0 + threadIdx.x;
            float4 a = make_float4(inf, inf, inf, 0.f);
            if (j < n_hist) {
                const int64_t p = near_id(hist, i64, g * ld_hist + j);
                const uint64_t col = (uint64_t)p - (uint64_t)hist_offset;     // (unsigned: no overflow)
                if (p != 0 && col < (uint64_t)V) {
                    a = pos[col];
                    atomicMax(&s_cnt[par], (int)threadIdx.x + 1);
                }
            }
            s_a[threadIdx.x] = a;
            __syncthreads();
            const int cnt = s_cnt[par];
            for (int q0 = 0; q0 < cnt; q0 += NEAR_POLL) {
                bool all = true;
#pragma unroll
                for (int i = 0; i < NEAR_ITERS; ++i) all &= near[i];
                if (__ballot(!all) == 0) break;    // (wave-uniform; the barriers stay outside this loop)
                const int q1 = q0 + NEAR_POLL < cnt ? q0 + NEAR_POLL : cnt;
                for (int q = q0; q < q1; ++q) {
                    const float4 a4 = s_a[q];
#pragma unroll
                    for (int i = 0; i < NEAR_ITERS; ++i) near[i] |= near_pred(pc[i], a4, chord2_max);
                }
            }
        }
    } else {
        if (threadIdx.x == 0) s_last = -1;
        __syncthreads();
        int last = -1;
        for (int64_t j = threadIdx.x; j < n_hist; j += NEAR_THREADS) {
            const int64_t p = near_id(hist, i64, g * ld_hist + j);
            if (p != 0 && (uint64_t)p - (uint64_t)hist_offset < (uint64_t)V) last = (int)j;
        }
        if (last >= 0) atomicMax(&s_last, last);
        __syncthreads();
        last = s_last;
        if (last >= 0) {                           // (uniform over the workgroup)
            const int64_t col = near_id(hist, i64, g * ld_hist + last) - hist_offset;
            const float4 a4 = pos[col];
#pragma unroll
            for (int i = 0; i < NEAR_ITERS; ++i) near[i] = near_pred(pc[i], a4, chord2_max);
        }
    }

#pragma unroll
    for (int i = 0; i < NEAR_ITERS; ++i) {
        const unsigned long long b = __ballot(near[i]);    // (columns >= V hold +inf: never near, their bits are 0)
        const int64_t wi = base / 32 + (i * (NEAR_THREADS / 64) + w) * 2 + lane;
        if (lane < 2 && wi < W) {
            uint32_t v = lane ? (uint32_t)(b >> 32) : (uint32_t)b;
            if (allow_and) v &= allow_and[wi];
            words[g * ld_words + wi] = v;
        }
    }
}

}  // namespace

extern "C" int mobgt_near_words(const float* pos, int64_t V, const void* hist, int hist_dtype, int64_t ld_hist, int64_t n_hist_cols,
                                int64_t hist_offset, int mode, float chord2_max, const uint32_t* allow_and, uint32_t* words,
                                int64_t ld_words, int64_t G, void* stream) {
    if (G <= 0 || G > 65535 || V <= 0 || V >= (int64_t)INT32_MAX) return MOBGT_EBADDIM;
    if (!pos || (!hist && n_hist_cols > 0) || !words || n_hist_cols < 0 || n_hist_cols >= (int64_t)INT32_MAX || ld_hist < n_hist_cols || ld_words < (V + 31) / 32) return MOBGT_EBADDIM;
    if (mode != MOBGT_NEAR_LAST && mode != MOBGT_NEAR_ANY) return MOBGT_EBADDIM;
    if (hist_dtype != MOBGT_I64 && hist_dtype != MOBGT_I32) return MOBGT_EDTYPE;
    if ((uintptr_t)pos & 15) return MOBGT_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((V + NEAR_COLS - 1) / NEAR_COLS), (unsigned)G);
    const float4* p4 = reinterpret_cast<const float4*>(pos);
    const int i64 = hist_dtype == MOBGT_I64;
    if (mode == MOBGT_NEAR_ANY)
        hipLaunchKernelGGL(near_words_kernel<true>, grid, dim3(NEAR_THREADS), 0, st, p4, V, hist, i64, ld_hist, n_hist_cols, hist_offset,
                           chord2_max, allow_and, words, ld_words);
    else
        hipLaunchKernelGGL(near_words_kernel<false>, grid, dim3(NEAR_THREADS), 0, st, p4, V, hist, i64, ld_hist, n_hist_cols, hist_offset,
                           chord2_max, allow_and, words, ld_words);
    return (int)hipGetLastError();
}
