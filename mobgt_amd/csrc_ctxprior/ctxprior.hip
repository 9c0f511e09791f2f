// include/mobgt_ctxprior.h: the category-transition and time-of-day prior -- one integer histogram over (slot, category), and the
// two fitted tables blended into a model's scores.  The rule is the docstring of mobgt_amd/ctxprior.py; the header repeats it in
// short.
//
// slot_hist_kernel -- the pairs (k - 1, k) of consecutive check-ins inside one train session, counted by (slot of k - 1,
// category of k).  The packed rows are ../csrc_universe/counts.hip's, but the sessions come as offsets, not as a session id per
// row, so the walk is by session: a wave per session, a lane per pair (as csr_hist_kernel of ../csrc_geoprior walks CSR rows), and
// an offsets pair is checked before it bounds a loop.  Every pair hits one of n_slots * n_cat cells, a few thousand addresses for
// millions of pairs: up to LDS_CELLS cells the workgroup counts in a 32-bit histogram of its own in LDS and flushes the cells that
// are not empty once, with 64-bit vector atomics; a workgroup takes SESSIONS sessions per step and walks the sessions in steps of
// the grid, so it clears and flushes once however many sessions it counts.  With more cells every add is a 64-bit atomic on
// global memory.
//
// blend_kernel -- ONE WORKGROUP PER (CHUNK OF COLUMNS, ROW): the anchor position (../csrc_prior/blend_rows.h), its category and
// slot, then the two rows of
// PRODUCTS w * T[.][k] staged in LDS, one f32 product per category -- the same bits as a product per element, and no multiply
// is left in the column loop.  A thread blends CHUNK / THREADS columns, each read and written by that thread only, so in place
// is safe: where both rows are 16-byte aligned four consecutive columns per lane (one 16-byte load and store), else one column
// per lane and step; both forms do the same arithmetic on the same elements.
//
// Built with -ffp-contract=off (Makefile): a term is one product and one sum, each rounded on its own.  No workgroup reads what
// another writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_ctxprior.h"
#include "../csrc_prior/blend_rows.h"

namespace {

constexpr int TPB = MOBGT_CTXPRIOR_THREADS;
constexpr int WAVES = TPB / WAVE;
constexpr int LDS_CELLS = MOBGT_CTXPRIOR_LDS_CELLS;
constexpr int SESSIONS = MOBGT_CTXPRIOR_SESSIONS;
constexpr int CHUNK = MOBGT_CTXPRIOR_CHUNK;
constexpr int PER_LANE = 4;                        // columns of one 16-byte load
constexpr size_t LDS_MAX = (size_t)LDS_CELLS * sizeof(unsigned);
static_assert(TPB % WAVE == 0 && SESSIONS % WAVES == 0 && CHUNK % (TPB * PER_LANE) == 0, "whole waves, whole steps");
static_assert(LDS_MAX <= 160 * 1024, "the histogram fits a CU's LDS");
static_assert(2 * sizeof(float) * MOBGT_CTXPRIOR_MAX_CAT <= 64 * 1024, "the blend's two rows of products fit the default LDS limit");
static_assert((int64_t)MOBGT_CTXPRIOR_MAX_SLOTS * MOBGT_CTXPRIOR_MAX_CAT > LDS_CELLS, "the global form is reachable");
static_assert((int64_t)MOBGT_CTXPRIOR_MAX_SLOTS * MOBGT_CTXPRIOR_MAX_CAT <= INT32_MAX, "a cell is an int");
static_assert(MOBGT_CTXPRIOR_I32 == ROWS_I32 && MOBGT_CTXPRIOR_I64 == ROWS_I64, "blend_rows.h's dtype codes are this header's");

// counts[slot * n_cat + b - 1] += 1 for every pair of a train session.  Dynamic LDS: IN_LDS only, n_slots * n_cat counts.
template <bool IN_LDS>
__global__ __launch_bounds__(TPB) void slot_hist_kernel(const int32_t* __restrict__ seq, int64_t M, const int64_t* __restrict__ offsets,
                                                        int64_t n_sessions, const uint8_t* __restrict__ train, int n_slots, int n_cat,
                                                        unsigned long long* __restrict__ counts, int32_t* __restrict__ status) {
    extern __shared__ unsigned s_hist[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int cells = n_slots * n_cat;
    if (IN_LDS) {
        for (int q = t; q < cells; q += TPB) s_hist[q] = 0u;
        __syncthreads();
    }
    int bad = 0;
    for (int64_t s0 = (int64_t)blockIdx.x * SESSIONS; s0 < n_sessions; s0 += (int64_t)gridDim.x * SESSIONS) {
        for (int r = wave; r < SESSIONS; r += WAVES) {
            const int64_t s = s0 + r;
            if (s >= n_sessions) break;                                 // (uniform in the wave)
            const int64_t o0 = offsets[s], o1 = offsets[s + 1];
            if (o0 < 0 || o1 < o0 || o1 > M) {                          // the session is skipped
                if (lane == 0) bad |= MOBGT_CTXPRIOR_SBADINDEX;
                continue;
            }
            if (train[s] == 0) continue;
            for (int64_t k = o0 + 1 + lane; k < o1; k += WAVE) {        // rows k - 1 and k, both in [o0, o1) and so in [0, M)
                const int64_t slot = seq[3 * (k - 1) + 1], b = seq[3 * k + 2];
                if (slot < 0 || slot >= n_slots || b < 1 || b > n_cat) {   // the pair is skipped
                    bad |= MOBGT_CTXPRIOR_SBADVALUE;
                    continue;
                }
                const int cell = (int)slot * n_cat + (int)b - 1;
                if (IN_LDS) atomicAdd(&s_hist[cell], 1u);
                else atomicAdd(&counts[cell], 1ull);
            }
        }
    }
    if (bad) atomicOr(status, bad);
    if (IN_LDS) {
        __syncthreads();
        for (int q = t; q < cells; q += TPB) {
            const unsigned v = s_hist[q];
            if (v != 0u) atomicAdd(&counts[q], (unsigned long long)v);
        }
    }
}

struct Rows : BlendRows {
    int hist64;
    const void* time;
    const void* cat;
    int64_t ld_ctx;
    int ctx64;
};

// Dynamic LDS: 2 * C floats, the category products then the time products.
__global__ __launch_bounds__(TPB) void blend_kernel(Rows in, const int32_t* __restrict__ poi_cat, int64_t P, const float* __restrict__ Tc,
                                                    const float* __restrict__ Tt, int C, int S, const float* __restrict__ weights) {
    extern __shared__ __attribute__((aligned(16))) float s_terms[];
    __shared__ int32_t last_of_wave[WAVES];
    float* s_c = s_terms;
    float* s_t = s_terms + C;
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.y;
    const int64_t c0 = (int64_t)blockIdx.x * CHUNK;                     // < V
    const int32_t width = (int32_t)(in.V - c0 < CHUNK ? in.V - c0 : CHUNK);

    // the anchor: the last entry of the history row that is not 0 (blend_rows.h)
    int32_t last = anchor_scan<TPB>(in, g, tid, last_of_wave);
    __syncthreads();
    last = anchor_max<TPB>(last, last_of_wave);

    // the same in every lane of the workgroup; an id, a category or a slot outside its range is never an index
    const int64_t a = last >= 0 ? load_id(in.hist, in.hist64, g * in.ld_hist + last) : 0;
    const bool anchored = a >= 1 && a <= P;
    const int64_t ca = anchored ? load_id(in.cat, in.ctx64, g * in.ld_ctx + last) : 0;
    const int64_t ta = anchored ? load_id(in.time, in.ctx64, g * in.ld_ctx + last) : -1;
    const bool by_cat = anchored && ca >= 1 && ca <= C, by_time = anchored && ta >= 0 && ta < S;
    if (by_cat) {
        const float w = weights[0];
        const float* row = Tc + (ca - 1) * C;
        for (int k = tid; k < C; k += TPB) s_c[k] = __fmul_rn(w, row[k]);
    }
    if (by_time) {
        const float w = weights[1];
        const float* row = Tt + ta * C;
        for (int k = tid; k < C; k += TPB) s_t[k] = __fmul_rn(w, row[k]);
    }
    __syncthreads();

    const float* src = in.scores + g * in.ld_scores + c0;
    float* dst = in.out + g * in.ld_out + c0;
    const int64_t p0 = c0 + in.label_offset;                            // the POI of the chunk's first column, 1-based
    auto blend = [&](float s, int32_t j) {
        const int64_t p = p0 + j;
        if (anchored && p >= 1 && p <= P) {
            const int32_t k = poi_cat[p - 1];
            if (k >= 1 && k <= C) {
                if (by_cat) s = __fadd_rn(s, s_c[k - 1]);
                if (by_time) s = __fadd_rn(s, s_t[k - 1]);
            }
        }
        return s;
    };
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const int32_t whole = width / PER_LANE * PER_LANE;
        for (int32_t j = tid * PER_LANE; j < whole; j += TPB * PER_LANE) {
            float4 v = *reinterpret_cast<const float4*>(src + j);
            v.x = blend(v.x, j);
            v.y = blend(v.y, j + 1);
            v.z = blend(v.z, j + 2);
            v.w = blend(v.w, j + 3);
            *reinterpret_cast<float4*>(dst + j) = v;
        }
        for (int32_t j = whole + tid; j < width; j += TPB) dst[j] = blend(src[j], j);
    } else {
        for (int32_t j = tid; j < width; j += TPB) dst[j] = blend(src[j], j);
    }
}

bool bad_tables(int n_slots, int n_cat) {
    return n_slots < 1 || n_slots > MOBGT_CTXPRIOR_MAX_SLOTS || n_cat < 1 || n_cat > MOBGT_CTXPRIOR_MAX_CAT;
}

// more than the default 64 KB of dynamic LDS needs the attribute once per function (not a stream operation)
int lds_opt_in() {
    static const int rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(slot_hist_kernel<true>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
    return rc;
}

}  // namespace

extern "C" int mobgt_ctxprior_abi_version(void) { return MOBGT_CTXPRIOR_ABI_VERSION; }

extern "C" int mobgt_ctxprior_slot_hist(const void* seq, int64_t M, const void* offsets, int64_t n_sessions, const void* train, int n_slots,
                                        int n_cat, void* counts, void* status, void* stream) {
    if (bad_size(M) || bad_size(n_sessions) || bad_tables(n_slots, n_cat)) return MOBGT_CTXPRIOR_EBADDIM;
    const int64_t cells = (int64_t)n_slots * n_cat;
    if (bad_ptr(seq, 4, M) || bad_ptr(offsets, 8, n_sessions + 1) || bad_ptr(train, 1, n_sessions) || bad_ptr(counts, 8, cells) ||
        bad_ptr(status, 4, 1))
        return MOBGT_CTXPRIOR_EALIGN;
    const bool in_lds = cells <= LDS_CELLS;
    if (in_lds) {
        const int rc = lds_opt_in();
        if (rc != 0) return rc;
    }
    const hipError_t rc = hipMemsetAsync(counts, 0, (size_t)cells * sizeof(unsigned long long), (hipStream_t)stream);
    if (rc != hipSuccess) return (int)rc;
    if (n_sessions == 0 || M == 0) return 0;
    const int64_t steps = (n_sessions + SESSIONS - 1) / SESSIONS;
    const dim3 grid((unsigned)(steps < MOBGT_CTXPRIOR_MAX_GRID ? steps : MOBGT_CTXPRIOR_MAX_GRID));
    if (in_lds)
        hipLaunchKernelGGL(slot_hist_kernel<true>, grid, dim3(TPB), (size_t)cells * sizeof(unsigned), (hipStream_t)stream, (const int32_t*)seq, M,
                           (const int64_t*)offsets, n_sessions, (const uint8_t*)train, n_slots, n_cat, (unsigned long long*)counts,
                           (int32_t*)status);
    else
        hipLaunchKernelGGL(slot_hist_kernel<false>, grid, dim3(TPB), 0, (hipStream_t)stream, (const int32_t*)seq, M, (const int64_t*)offsets,
                           n_sessions, (const uint8_t*)train, n_slots, n_cat, (unsigned long long*)counts, (int32_t*)status);
    return (int)hipGetLastError();
}

extern "C" int mobgt_ctxprior_blend_rows(const float* scores, int64_t ld_scores, float* out, int64_t ld_out, int64_t G, int64_t V,
                                         int64_t label_offset, const void* hist, int hist_dtype, int64_t ld_hist, int64_t n_hist_cols,
                                         const void* time, const void* cat, int ctx_dtype, int64_t ld_ctx, const int32_t* poi_cat, int64_t P,
                                         const float* cat_table, const float* slot_table, int n_cat, int n_slots, const float* weights,
                                         void* stream) {
    const Rows in = {{scores, out, ld_scores, ld_out, V, label_offset, hist, ld_hist, n_hist_cols}, hist_dtype == MOBGT_CTXPRIOR_I64,
                     time, cat, ld_ctx, ctx_dtype == MOBGT_CTXPRIOR_I64};
    if (bad_rows_dims(in, G, MOBGT_CTXPRIOR_MAX_G) || P < 1 || P > INT32_MAX || bad_tables(n_slots, n_cat) || ld_ctx < n_hist_cols)
        return MOBGT_CTXPRIOR_EBADDIM;
    if (bad_id_dtype(hist_dtype) || bad_id_dtype(ctx_dtype)) return MOBGT_CTXPRIOR_EDTYPE;
    const uintptr_t ctx_align = in.ctx64 ? 8 : 4;
    if (bad_rows_ptrs(in, in.hist64, G) || bad_ptr(time, ctx_align, G * n_hist_cols) || bad_ptr(cat, ctx_align, G * n_hist_cols) ||
        bad_ptr(poi_cat, 4, P) || bad_ptr(cat_table, 4, (int64_t)n_cat * n_cat) || bad_ptr(slot_table, 4, (int64_t)n_slots * n_cat) ||
        bad_ptr(weights, 4, 2))
        return MOBGT_CTXPRIOR_EALIGN;
    if (G == 0 || V == 0) return 0;
    const dim3 grid((unsigned)((V + CHUNK - 1) / CHUNK), (unsigned)G);
    hipLaunchKernelGGL(blend_kernel, grid, dim3(TPB), 2 * sizeof(float) * (size_t)n_cat, (hipStream_t)stream, in, poi_cat, P, cat_table,
                       slot_table, n_cat, n_slots, weights);
    const hipError_t err = hipGetLastError();
    return err != hipSuccess ? (int)err : 0;
}
