// libmobgt_tokscatter.so (include/mobgt_tokscatter.h): the backward of the encoder input's gathers for a few hundred positions.
//
// csrc/embed.hip's gather_multi_kernel<TI, true> gives one wave one position and lets it walk the jobs in order: fetch the job's
// parameters, load the index, wait; per 64 columns load the gradient piece, wait, issue one atomic -- and that wait also covers
// the atomics issued before it, because on gfx9 stores and atomics without a result count in vmcnt like loads.  At the fq widths
// (160 | 32 | 192 x 3, one job skipped) that is about twenty dependent round trips per wave and the whole of the launch's 11 us.
// Here the wave owns the same position and
//   1. requests the indices of all MAXJ job slots (slots past the job count repeat the last job: no branch between the loads),
//   2. requests every piece of every job's gradient row -- MAXJ x NPIECE floats per lane, column and slot clamped instead of
//      predicated, so the loads do not depend on the indices and nothing stands between them,
//   3. waits ONCE, then issues all its atomics back to back.
// An IDENTITY job (row r of the table is position r: the distance GCN's compact per-batch table) is not scattered at all: its
// rows are written with plain stores, zeros where the position is a pad, and its destination needs no zero-fill.
// Behind the row workgroups the launch may carry passenger workgroups that form gu = (scale[r] (g W^T))^T in bf16 from the
// identity job's gradient rows (csrc/sgemm_body.h sgemm_nk_tile_burst: four one-wave tiles per workgroup) -- the operand of the
// distance GCN's mask_rows_bwd, which used to be a launch of its own two launches later.  No workgroup waits for another.
#include "mobgt_tokscatter.h"
#include "sgemm_body.h"

namespace {

constexpr int MAXJ = MOBGT_TOKSCATTER_MAX_JOBS;
constexpr int NPIECE = MOBGT_TOKSCATTER_MAX_WIDTH / 64;
static_assert(MOBGT_TOKSCATTER_MAX_WIDTH % 64 == 0, "whole pieces");
static_assert(MOBGT_TOKSCATTER_RIDE_MAX_K == 16 * mobgt_sgemm::NK_MAXS, "the k-steps the ride's tile holds in flight");
static_assert(MOBGT_TOKSCATTER_EBADDIM == MOBGT_EBADDIM && MOBGT_TOKSCATTER_EALIGN == MOBGT_EALIGN &&
              MOBGT_TOKSCATTER_EDTYPE == MOBGT_EDTYPE && MOBGT_TOKSCATTER_I64 == MOBGT_I64 && MOBGT_TOKSCATTER_I32 == MOBGT_I32,
              "the codes of include/mobgt_hip.h");

struct ScatterParams {
    float* d_tables[MAXJ];                   // null: the slot issues nothing (a skipped job, a slot past the job count)
    const void* idx[MAXJ];
    int64_t skip[MAXJ];
    int width[MAXJ];                         // 0 in the slots past the job count (their loads repeat the last job's)
    const float* src[MAXJ];                  // buf + coff
    int64_t ld[MAXJ];
    int64_t R;
    const float* extra_src;                  // the row-0 vector, or (extra_dst null) any readable address: requested either way
    float* extra_dst;                        // row 0 of the extra job's table, null: nothing is added
    int extra_width, identity;
    const void* ride_idx;                    // the identity job's index and skip value: rows it skips count as zeros in the ride
    int64_t ride_skip;
    int row_blocks;                          // workgroups in front of the passengers
    int ride_tiles;
    mobgt_sgemm::SgemmParams ride;
};

template <typename TI>
__global__ __launch_bounds__(256) void scatter_burst_kernel(const ScatterParams p) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if ((int)blockIdx.x >= p.row_blocks) {
        // ---- passengers: one 16 x 16 tile of gu per wave, from the identity job's gradient rows
        const int tile = ((int)blockIdx.x - p.row_blocks) * 4 + wave;
        if (tile < p.ride_tiles)
            mobgt_sgemm::sgemm_nk_tile_burst(p.ride, tile, reinterpret_cast<const TI*>(p.ride_idx), p.ride_skip);
        return;
    }
    const int64_t r = (int64_t)blockIdx.x * 4 + wave;
    if (r >= p.R) return;
    // ---- 1. every index
    int64_t row[MAXJ];
#pragma unroll
    for (int t = 0; t < MAXJ; ++t) row[t] = (int64_t)reinterpret_cast<const TI*>(p.idx[t])[r];
    // ---- 2. every piece of every gradient row (column clamped into the row: an address of its own never depends on an index),
    //         and the row-0 vector (every wave requests it -- there always is an address, see the launcher -- one wave adds it)
    float v[MAXJ][NPIECE], ex[NPIECE];
#pragma unroll
    for (int t = 0; t < MAXJ; ++t) {
        const float* from = p.src[t] + r * p.ld[t];
#pragma unroll
        for (int k = 0; k < NPIECE; ++k) v[t][k] = from[max(min(lane + 64 * k, p.width[t] - 1), 0)];
    }
#pragma unroll
    for (int k = 0; k < NPIECE; ++k) ex[k] = p.extra_src[min(lane + 64 * k, p.extra_width - 1)];
    // ---- 3. one wait, then the stores and atomics with nothing between them (the jobs' destinations, skip values and widths are
    //         fetched into scalar registers in front of the wait: left to itself the compiler fetches them job by job, between
    //         the atomics)
    float* dt[MAXJ];
    int64_t sk[MAXJ];
    int wd[MAXJ];
#pragma unroll
    for (int t = 0; t < MAXJ; ++t) {
        dt[t] = p.d_tables[t]; sk[t] = p.skip[t]; wd[t] = p.width[t];
        asm volatile("" : "+s"(dt[t]), "+s"(sk[t]), "+s"(wd[t]));
    }
    // s_waitcnt's immediate in the gfx9 encoding (gfx950 is a gfx9 target; gfx10 and later moved the fields and count stores in a
    // counter of their own): vmcnt = bits 15:14 | 3:0, expcnt = bits 6:4, lgkmcnt = bits 11:8.  0x0F70 = vmcnt 0, expcnt 7 and
    // lgkmcnt 15 (their largest values: not waited for).  On another target these bits would name other counters: see the #error.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "scatter_burst_kernel: the s_waitcnt immediate below is the gfx9 encoding"
#endif
    __builtin_amdgcn_s_waitcnt(0x0F70);
    if (p.extra_dst && blockIdx.x == 0 && wave == 0) {
#pragma unroll
        for (int k = 0; k < NPIECE; ++k)
            if (lane + 64 * k < p.extra_width) atomicAdd(p.extra_dst + lane + 64 * k, ex[k]);
    }
#pragma unroll
    for (int t = 0; t < MAXJ; ++t) {
        if (!dt[t]) continue;
        const bool live = row[t] >= 0 && row[t] != sk[t];
        if (t == p.identity) {
            float* dst = dt[t] + r * wd[t];
#pragma unroll
            for (int k = 0; k < NPIECE; ++k)
                if (lane + 64 * k < wd[t]) dst[lane + 64 * k] = live ? v[t][k] : 0.f;
        } else if (live) {
            float* dst = dt[t] + row[t] * wd[t];
#pragma unroll
            for (int k = 0; k < NPIECE; ++k)
                if (lane + 64 * k < wd[t]) atomicAdd(dst + lane + 64 * k, v[t][k]);
        }
    }
}

}  // namespace

extern "C" int mobgt_tokscatter_abi_version(void) { return MOBGT_TOKSCATTER_ABI_VERSION; }

extern "C" int mobgt_tokscatter_bwd(int n, float* const* d_tables, const void* const* idx, const int64_t* skip, const int* width,
                                    const int* coff, const float* const* buf, const int64_t* ld, int64_t R, int idx_dtype,
                                    const float* extra_row0, int extra_job, int identity_job, const float* ride_w, int64_t ride_ldw,
                                    const float* ride_scale, void* ride_gut, int64_t ride_ldt, int ride_n, void* stream) {
    if (n < 1 || n > MAXJ || !d_tables || !idx || !width || !coff || !buf || !ld) return MOBGT_TOKSCATTER_EBADDIM;
    if (idx_dtype != MOBGT_TOKSCATTER_I64 && idx_dtype != MOBGT_TOKSCATTER_I32) return MOBGT_TOKSCATTER_EDTYPE;
    if (identity_job < -1 || identity_job >= n || (identity_job >= 0 && !d_tables[identity_job])) return MOBGT_TOKSCATTER_EBADDIM;
    if (extra_row0 && (extra_job < 0 || extra_job >= n || extra_job == identity_job)) return MOBGT_TOKSCATTER_EBADDIM;
    if (R > (int64_t)1 << 30) return MOBGT_TOKSCATTER_EBADDIM;
    ScatterParams p = {};
    for (int t = 0; t < n; ++t) {
        if (width[t] < 1 || width[t] > MOBGT_TOKSCATTER_MAX_WIDTH || coff[t] < 0 || ld[t] < (int64_t)coff[t] + width[t] || !buf[t] || !idx[t])
            return MOBGT_TOKSCATTER_EBADDIM;
        if (((uintptr_t)buf[t] | (uintptr_t)d_tables[t]) & 3) return MOBGT_TOKSCATTER_EALIGN;
        p.d_tables[t] = d_tables[t]; p.idx[t] = idx[t]; p.skip[t] = skip ? skip[t] : -1;
        p.width[t] = width[t]; p.src[t] = buf[t] + coff[t]; p.ld[t] = ld[t];
    }
    for (int t = n; t < MAXJ; ++t) {                              // (the slots past the job count: the last job's loads, nothing issued)
        p.idx[t] = p.idx[n - 1]; p.src[t] = p.src[n - 1]; p.ld[t] = p.ld[n - 1]; p.skip[t] = -1;
    }
    p.R = R; p.identity = identity_job;
    p.extra_src = p.src[0]; p.extra_width = 1;                    // (no row-0 vector: a readable float)
    if (extra_row0) {
        if ((uintptr_t)extra_row0 & 3) return MOBGT_TOKSCATTER_EALIGN;
        p.extra_src = extra_row0; p.extra_width = width[extra_job]; p.extra_dst = d_tables[extra_job];
    }
    p.row_blocks = (int)((R + 3) / 4);
    if (ride_gut) {
        const int j = identity_job;
        if (j < 0 || !ride_w || ride_n < 1 || ride_n > MOBGT_TOKSCATTER_RIDE_MAX_N || (width[j] & 15) ||
            width[j] > MOBGT_TOKSCATTER_RIDE_MAX_K || ride_ldw < width[j] || ride_ldt < R)
            return MOBGT_TOKSCATTER_EBADDIM;
        if ((((uintptr_t)p.src[j] | (uintptr_t)ride_w) & 15) || (ld[j] & 3) || (ride_ldw & 3) || ((uintptr_t)ride_gut & 1) ||
            ((uintptr_t)ride_scale & 3))
            return MOBGT_TOKSCATTER_EALIGN;
        mobgt_sgemm::SgemmParams& s = p.ride;
        s.A = p.src[j]; s.lda = ld[j]; s.B = ride_w; s.ldb = ride_ldw; s.M = (int)R; s.N = ride_n; s.K = width[j]; s.Kb = s.K;
        s.ct = reinterpret_cast<bf16_t*>(ride_gut); s.ldt = ride_ldt; s.ct_scale = ride_scale;
        p.ride_tiles = (int)((R + 15) / 16) * ((ride_n + 15) / 16);
        p.ride_idx = idx[j]; p.ride_skip = p.skip[j];
    }
    if (R <= 0) return 0;
    const dim3 grid((unsigned)(p.row_blocks + (p.ride_tiles + 3) / 4)), block(256);
    if (idx_dtype == MOBGT_TOKSCATTER_I64) hipLaunchKernelGGL(scatter_burst_kernel<int64_t>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(scatter_burst_kernel<int32_t>, grid, block, 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}
