// The candidate restriction shared by mobgt_topk_rows_masked (topk.hip) and mobgt_rank_metrics_masked (skinny.hip): an allow
// bitmap shared by the rows (NULL: every column) or one per row (ld_allow > 0: the *_masked_rows entry points), and a per-row
// list of excluded ids (NULL: none).  Column c of row g is a candidate when its allow bit is set and no entry p of
// excl[g, 0:n_excl] has p != 0 && p - excl_offset == c.
#pragma once

struct CandMask {
    const uint32_t* allow;                         // ceil(V / 32) words, bit c & 31 of word c >> 5 = column c may be a candidate
    const void* excl;                              // [G, ld_excl] int32 / int64 ids; 0 = padding; id - excl_offset = column
    int64_t ld_excl, n_excl, excl_offset;
    int excl_i64;
    int64_t ld_allow;                              // words between consecutive rows' allow words; 0 = one bitmap shared by the rows
};                                                 // (last: the fields the shared form reads keep their kernel-argument offsets)

// row g's allow words (m.allow != NULL).  ROWS is a compile-time copy of m.ld_allow > 0: the shared form never reads the stride,
// so its kernels are the code they were before the per-row form existed.
template <bool ROWS>
__device__ __forceinline__ const uint32_t* cand_allow_row(const CandMask& m, int64_t g) {
    if constexpr (ROWS) return m.allow + g * m.ld_allow;
    return m.allow;
}

__device__ __forceinline__ int64_t cand_excl_id(const CandMask& m, int64_t g, int64_t j) {
    return m.excl_i64 ? reinterpret_cast<const int64_t*>(m.excl)[g * m.ld_excl + j]
                      : (int64_t)reinterpret_cast<const int32_t*>(m.excl)[g * m.ld_excl + j];
}

// Block-wide (NT threads): s_ok[0, NW) <- the candidate bits of row g's columns [base, base + 32 NW), base a multiple of 32 --
// the row's allow words (0 past ceil(V / 32)), then the row's excluded ids that fall inside the range cleared.  Ends in a barrier;
// the caller puts another between its last read of s_ok and the next call.  An id outside [0, V) lands outside the range, or
// on a column >= V whose bit the caller never reads.
template <int NW, int NT, bool ROWS>
__device__ __forceinline__ void cand_bits(uint32_t* s_ok, const CandMask& m, int64_t g, int64_t base, int64_t V) {
    static_assert(NW <= NT, "one allow word per thread");
    int64_t p = 0;
    if (m.excl && (int64_t)threadIdx.x < m.n_excl) p = cand_excl_id(m, g, threadIdx.x);     // (in flight with the allow word)
    if (threadIdx.x < NW) {
        const int64_t wi = base / 32 + threadIdx.x;
        s_ok[threadIdx.x] = !m.allow ? ~0u : wi < (V + 31) / 32 ? cand_allow_row<ROWS>(m, g)[wi] : 0u;
    }
    __syncthreads();
    if (m.excl) {
        for (int64_t j = threadIdx.x; j < m.n_excl; j += NT) {
            if (j >= NT) p = cand_excl_id(m, g, j);
            const uint64_t r = (uint64_t)p - (uint64_t)m.excl_offset - (uint64_t)base;     // (unsigned: no overflow)
            if (p != 0 && r < (uint64_t)(32 * NW)) atomicAnd(&s_ok[r >> 5], ~(1u << (r & 31)));
        }
        __syncthreads();
    }
}
