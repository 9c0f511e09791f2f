// Row-wise top-k over stored scores (mobgt_topk_rows): the ranked next-POI list of Graphormer.recommend_step / train.PredictLoop.
//
// Contract (include/mobgt_hip.h): ids[g, :k], vals[g, :k] equal torch.sort(scores, dim=1, descending=True, stable=True)[:, :k]
// bit for bit -- descending score, equal scores in ascending column order (the metrics' tie rule, mobgt_target_rank), -0.0 tied
// with +0.0, NaN (either sign) above +inf.  Every score maps to an order-preserving 64-bit key
//     (flipped float bits << 32) | ~column
// so that ONE descending unsigned compare of keys is that whole order, and no two keys of a row are equal.
//
// Two launches, slab-and-finish as mobgt_rank_metrics: launch 1 gives every TK_CHUNK columns of a row to one workgroup, which
// writes the chunk's k best keys, sorted, to its slice of `work` (plain stores); launch 2, one workgroup per row, merges the
// chunks' lists and writes ids / vals.  No workgroup waits for another and nothing is left armed between calls, so a captured
// graph replays the pair freely.
//
// The selection is wave-wide: a wave keeps its running best 64 keys sorted across its lanes (lane i holds the i-th).  A batch of
// 64 new keys that can change the top k (ballot against the k-th key) is sorted by a 21-stage bitonic network across lanes,
// reversed, folded in by a lane-wise max (the best 64 of both lists, as a bitonic sequence) and re-sorted by a 6-stage merge.
// The waves of a workgroup then fold their lists pairwise through LDS.
//
// mobgt_topk_rows_masked restricts each row to its candidates (an allow bitmap shared by the rows -- or one per row, through
// mobgt_topk_rows_masked_rows -- and a per-row list of excluded ids).  A non-candidate takes the key 0, which is below every real key, so the same selection never picks it: launch 1 builds
// its chunk's 32 candidate words in LDS (the allow words with the row's excluded ids cleared) before the ballot, and launch 2
// writes a final key 0 -- a row with fewer than k candidates -- as id -1, val -inf.  No extra launch, no [G, V / 32] buffer.
#include "common.h"
#include "../../include/mobgt_hip.h"
#include "cand_body.h"

namespace {

constexpr int TK_MAXK = MOBGT_TOPK_MAX_K;
constexpr int TK_WAVES1 = 4;                       // launch 1: 256 threads
constexpr int TK_ITERS = 4;                        // 64-key batches per wave
constexpr int TK_CHUNK = 64 * TK_WAVES1 * TK_ITERS;  // 1024 columns per workgroup of launch 1
constexpr int TK_WAVES2 = 16;                      // launch 2: 1024 threads, one row

inline int64_t tk_chunks(int64_t V) { return (V + TK_CHUNK - 1) / TK_CHUNK; }

__device__ __forceinline__ uint64_t tk_key(uint32_t u, uint32_t col) {
    uint32_t h;
    if ((u & 0x7fffffffu) > 0x7f800000u) {
        h = 0xffffffffu;                           // NaN: above +inf (0xff800000)
    } else {
        if (u == 0x80000000u) u = 0u;              // -0.0 ties +0.0
        h = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((uint64_t)h << 32) | (uint32_t)~col;   // >= 0x007fffff << 32 (-inf): 0 is below every real key
}

__device__ __forceinline__ uint64_t kmax(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t kmin(uint64_t a, uint64_t b) { return a < b ? a : b; }

// a bitonic sequence across the wave -> descending (lane 0 the largest)
__device__ __forceinline__ uint64_t wave_merge_desc(uint64_t x, int lane) {
#pragma unroll
    for (int j = 32; j >= 1; j >>= 1) {
        const uint64_t o = __shfl_xor(x, j, 64);
        x = (lane & j) ? kmin(x, o) : kmax(x, o);
    }
    return x;
}

__device__ __forceinline__ uint64_t wave_sort_desc(uint64_t x, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
        const bool desc = (lane & size) == 0;      // (size 64: every lane -- the whole wave descending)
#pragma unroll
        for (int j = size >> 1; j >= 1; j >>= 1) {
            const uint64_t o = __shfl_xor(x, j, 64);
            x = (((lane & j) == 0) == desc) ? kmax(x, o) : kmin(x, o);
        }
    }
    return x;
}

// top (sorted descending) <- the best 64 of top and b (b sorted descending)
__device__ __forceinline__ uint64_t wave_fold(uint64_t top, uint64_t b, int lane) {
    return wave_merge_desc(kmax(top, __shfl(b, 63 - lane, 64)), lane);
}

// the k-th best key so far: a new key must exceed it to matter
__device__ __forceinline__ uint64_t kth(uint64_t top, int k) { return __shfl(top, k - 1, 64); }

// the waves' lists folded pairwise through LDS; the result is wave 0's `top`
template <int NW>
__device__ __forceinline__ uint64_t block_fold(uint64_t top, uint64_t* s_keys, int w, int lane) {
#pragma unroll
    for (int s = 1; s < NW; s <<= 1) {
        if ((w & (2 * s - 1)) == s) s_keys[w * 64 + lane] = top;
        __syncthreads();
        if ((w & (2 * s - 1)) == 0) top = wave_fold(top, s_keys[(w + s) * 64 + lane], lane);
        __syncthreads();
    }
    return top;
}

// launch 1: grid (chunks, G); the chunk's k best keys, descending, -> work[g][chunk][0, k) (0 = no column).  MASK: columns that
// are not candidates take the key 0 (below every real key), so they are never selected; ROWS: allow words per row (cand_body.h).
template <bool MASK, bool ROWS = false>
__global__ __launch_bounds__(64 * TK_WAVES1) void topk_chunk_kernel(const float* __restrict__ scores, int64_t ld, int64_t V, int k,
                                                                    uint64_t* __restrict__ work, CandMask m) {
    __shared__ uint64_t s_keys[TK_WAVES1 * 64];
    __shared__ uint32_t s_ok[TK_CHUNK / 32];       // MASK: the chunk's candidate bits
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t g = blockIdx.y, nch = gridDim.x;
    const uint32_t* row = reinterpret_cast<const uint32_t*>(scores + g * ld);
    const int64_t c0 = (int64_t)blockIdx.x * TK_CHUNK + w * 64 + lane;
    uint64_t key[TK_ITERS];
#pragma unroll
    for (int i = 0; i < TK_ITERS; ++i) {           // (all loads in flight before the first sort)
        const int64_t c = c0 + i * 64 * TK_WAVES1;
        key[i] = c < V ? tk_key(row[c], (uint32_t)c) : 0;
    }
    if constexpr (MASK) {
        cand_bits<TK_CHUNK / 32, 64 * TK_WAVES1, ROWS>(s_ok, m, g, (int64_t)blockIdx.x * TK_CHUNK, V);   // (cand_body.h)
#pragma unroll
        for (int i = 0; i < TK_ITERS; ++i) {
            const int r = w * 64 + lane + i * 64 * TK_WAVES1;
            if (!((s_ok[r >> 5] >> (r & 31)) & 1u)) key[i] = 0;
        }
    }
    uint64_t top = 0, thr = 0;
#pragma unroll
    for (int i = 0; i < TK_ITERS; ++i) {
        if (__ballot(key[i] > thr) == 0) continue;   // (wave-uniform)
        top = wave_fold(top, wave_sort_desc(key[i], lane), lane);
        thr = kth(top, k);
    }
    top = block_fold<TK_WAVES1>(top, s_keys, w, lane);
    if (w == 0 && lane < k) work[(g * nch + blockIdx.x) * k + lane] = top;
}

// launch 2: one workgroup per row; wave w folds the chunk lists w, w + 16, ...; wave 0 writes the row's k results.  MASK: a row
// with m < k candidates ends in the key 0 from position m on, written as id -1, val -inf.
template <bool MASK>
__global__ __launch_bounds__(64 * TK_WAVES2) void topk_finish_kernel(const float* __restrict__ scores, int64_t ld, int64_t nch, int k,
                                                                     const uint64_t* __restrict__ work, int64_t col_offset,
                                                                     int64_t* __restrict__ ids, float* __restrict__ vals) {
    __shared__ uint64_t s_keys[TK_WAVES2 * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t g = blockIdx.x;
    const uint64_t* lists = work + g * nch * k;
    uint64_t top = 0, thr = 0;
    for (int64_t j = w; j < nch; j += TK_WAVES2) {
        const uint64_t b = lane < k ? lists[j * k + lane] : 0;     // (sorted descending: lane 0 its best)
        if (__shfl(b, 0, 64) <= thr) continue;
        top = wave_fold(top, b, lane);
        thr = kth(top, k);
    }
    top = block_fold<TK_WAVES2>(top, s_keys, w, lane);
    if (w == 0 && lane < k) {
        const uint32_t col = ~(uint32_t)top;       // (V >= k real keys per row: the first k are columns, never the 0 filler)
        if (MASK && top == 0) {
            ids[g * k + lane] = -1;
            vals[g * k + lane] = -__builtin_inff();
            return;
        }
        ids[g * k + lane] = (int64_t)col + col_offset;
        reinterpret_cast<uint32_t*>(vals)[g * k + lane] = reinterpret_cast<const uint32_t*>(scores + g * ld)[col];   // the stored bits
    }
}

}  // namespace

extern "C" int64_t mobgt_topk_work_bytes(int64_t G, int64_t V, int64_t k) {
    if (G <= 0 || V <= 0 || k <= 0 || k > TK_MAXK) return 0;
    return 8 * G * tk_chunks(V) * k;
}

namespace {

int topk_launch(const float* scores, int64_t ld, int64_t G, int64_t V, int64_t k, int64_t col_offset, int64_t* ids, float* vals,
                void* work, const CandMask& m, bool masked, void* stream) {
    if (G <= 0 || G > 65535 || V <= 0 || V >= (int64_t)INT32_MAX || k < 1 || k > TK_MAXK || k > V || ld < V) return MOBGT_EBADDIM;
    if (!scores || !ids || !vals || !work) return MOBGT_EBADDIM;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nch = tk_chunks(V);
    uint64_t* wk = reinterpret_cast<uint64_t*>(work);
    if (masked && m.ld_allow > 0) {
        hipLaunchKernelGGL((topk_chunk_kernel<true, true>), dim3((unsigned)nch, (unsigned)G), dim3(64 * TK_WAVES1), 0, st, scores, ld, V,
                           (int)k, wk, m);
        hipLaunchKernelGGL(topk_finish_kernel<true>, dim3((unsigned)G), dim3(64 * TK_WAVES2), 0, st, scores, ld, nch, (int)k,
                           (const uint64_t*)wk, col_offset, ids, vals);
    } else if (masked) {
        hipLaunchKernelGGL(topk_chunk_kernel<true>, dim3((unsigned)nch, (unsigned)G), dim3(64 * TK_WAVES1), 0, st, scores, ld, V,
                           (int)k, wk, m);
        hipLaunchKernelGGL(topk_finish_kernel<true>, dim3((unsigned)G), dim3(64 * TK_WAVES2), 0, st, scores, ld, nch, (int)k,
                           (const uint64_t*)wk, col_offset, ids, vals);
    } else {
        hipLaunchKernelGGL(topk_chunk_kernel<false>, dim3((unsigned)nch, (unsigned)G), dim3(64 * TK_WAVES1), 0, st, scores, ld, V,
                           (int)k, wk, m);
        hipLaunchKernelGGL(topk_finish_kernel<false>, dim3((unsigned)G), dim3(64 * TK_WAVES2), 0, st, scores, ld, nch, (int)k,
                           (const uint64_t*)wk, col_offset, ids, vals);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int mobgt_topk_rows(const float* scores, int64_t ld, int64_t G, int64_t V, int64_t k, int64_t col_offset, int64_t* ids,
                               float* vals, void* work, void* stream) {
    return topk_launch(scores, ld, G, V, k, col_offset, ids, vals, work, CandMask{}, false, stream);
}

extern "C" int mobgt_topk_rows_masked_rows(const float* scores, int64_t ld, int64_t G, int64_t V, int64_t k, int64_t col_offset,
                                           const uint32_t* allow, int64_t ld_allow, const void* excl, int excl_dtype, int64_t ld_excl,
                                           int64_t n_excl_cols, int64_t excl_offset, int64_t* ids, float* vals, void* work,
                                           void* stream) {
    if (excl && (n_excl_cols < 0 || ld_excl < n_excl_cols)) return MOBGT_EBADDIM;
    if (excl && excl_dtype != MOBGT_I64 && excl_dtype != MOBGT_I32) return MOBGT_EDTYPE;
    if (ld_allow < 0 || (allow && ld_allow > 0 && ld_allow < (V + 31) / 32)) return MOBGT_EBADDIM;
    const bool use_excl = excl && n_excl_cols > 0;
    const CandMask m{allow, use_excl ? excl : nullptr, ld_excl, n_excl_cols, excl_offset, excl_dtype == MOBGT_I64, allow ? ld_allow : 0};
    return topk_launch(scores, ld, G, V, k, col_offset, ids, vals, work, m, allow || use_excl, stream);
}

extern "C" int mobgt_topk_rows_masked(const float* scores, int64_t ld, int64_t G, int64_t V, int64_t k, int64_t col_offset,
                                      const uint32_t* allow, const void* excl, int excl_dtype, int64_t ld_excl, int64_t n_excl_cols,
                                      int64_t excl_offset, int64_t* ids, float* vals, void* work, void* stream) {
    return mobgt_topk_rows_masked_rows(scores, ld, G, V, k, col_offset, allow, 0, excl, excl_dtype, ld_excl, n_excl_cols, excl_offset,
                                       ids, vals, work, stream);
}
