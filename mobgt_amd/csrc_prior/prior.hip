// include/mobgt_prior.h: the fitted Markov tables blended into a model's scores.  The rule is the docstring of
// mobgt_amd/prior.py; the header repeats it in short.
//
// ONE WORKGROUP PER (CHUNK OF COLUMNS, ROW).  The anchor search is blend_rows.h's, shared with the other two priors; its one
// barrier is also the chunk's.  Whatever a workgroup indexes with -- the anchor, its rowptr pair, the part of the
// row inside the chunk, the (u, a) range of the keys -- is found with the same value in every lane and checked before it is used.
// The chunk lives in LDS between its one load and its one store: the entries of the CSR row are added there, a thread an entry,
// and a row's columns are distinct, so no two threads meet on one element.  A workgroup reads the tables and its chunk of
// `scores` and writes its chunk of `out` only: no workgroup waits for another, and in place is safe.
//
// Built with -ffp-contract=off (Makefile): a term is one product and one sum, each rounded on its own, as blend_host rounds them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_prior.h"
#include "blend_rows.h"

namespace {

constexpr int TPB = MOBGT_PRIOR_THREADS;
constexpr int CHUNK = MOBGT_PRIOR_CHUNK;
static_assert(TPB % WAVE == 0 && CHUNK % TPB == 0, "a workgroup is whole waves and takes CHUNK / THREADS columns a thread");
static_assert(MOBGT_PRIOR_I32 == ROWS_I32 && MOBGT_PRIOR_I64 == ROWS_I64, "blend_rows.h's dtype codes are this header's");

struct Rows : BlendRows {
    const void* user;
    int64_t ld_user, user_offset;
    int hist64, user64;
};

struct Tables {
    const int64_t* rowptr;
    const int32_t* col;
    const float* lg;
    int64_t nnz;
    const int64_t* ukey;
    const float* lu;
    int64_t nnzU, U;
    const float* lp;
    int64_t P;
};

// the first i in [lo, hi) with a[i] >= x, hi if there is none; a ascending.  One lane's search.
template <class T>
__device__ inline int32_t lower(const T* __restrict__ a, int32_t lo, int32_t hi, T x) {
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (a[mid] < x) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// (the same by a whole wave, six dependent loads for 2^31 elements where `lower` takes 31: wave_lower of blend_rows.h)

__global__ __launch_bounds__(TPB) void blend_kernel(Rows in, Tables tb, const float* __restrict__ weights, int32_t* __restrict__ status) {
    __shared__ float tile[CHUNK];
    __shared__ int32_t last_of_wave[TPB / WAVE];
    const int tid = threadIdx.x, lane = tid % WAVE;
    const int64_t g = blockIdx.y;
    const int64_t c0 = (int64_t)blockIdx.x * CHUNK;                     // < V
    const int32_t width = (int32_t)(in.V - c0 < CHUNK ? in.V - c0 : CHUNK);
    const float wu = weights[0], wg = weights[1], wp = weights[2];

    // the anchor: the last entry of the history row that is not 0 (blend_rows.h)
    int32_t last = anchor_scan<TPB>(in, g, tid, last_of_wave);

    // meanwhile the chunk with the popularity term
    const float* src = in.scores + g * in.ld_scores + c0;
    for (int32_t j = tid; j < width; j += TPB) {
        float s = src[j];
        const int64_t p = c0 + j + in.label_offset;                     // the column's POI, 1-based
        if (p >= 1 && p <= tb.P) {
            const float l = tb.lp[p - 1];
            if (l > 0.0f) s = __fadd_rn(s, __fmul_rn(wp, l));
        }
        tile[j] = s;
    }
    __syncthreads();
    last = anchor_max<TPB>(last, last_of_wave);

    // from here to the loop over the entries everything is the same in every lane of the workgroup
    int32_t e_lo = 0, e_hi = 0;
    int64_t a = 0;
    bool row_flag = false, flag = false;
    if (last >= 0) {
        a = load_id(in.hist, in.hist64, g * in.ld_hist + last);
        if (a >= 1 && a <= tb.P) {
            const int64_t r0 = tb.rowptr[a - 1], r1 = tb.rowptr[a];
            if (r0 < 0 || r1 < r0 || r1 > tb.nnz) {
                row_flag = true;                                        // the row counts as empty
            } else {
                // col ascends inside a row: entries outside [0, P) stand at its ends, and no chunk's part holds them
                if (r1 > r0 && (tb.col[r0] < 0 || tb.col[r1 - 1] >= tb.P)) row_flag = true;
                // POI (0-based) q is column q + 1 - label_offset: the chunk is the POIs [q0, q0 + width)
                const int64_t q0 = c0 + in.label_offset - 1;
                e_lo = wave_lower(tb.col, (int32_t)r0, (int32_t)r1, (int32_t)(q0 < 0 ? 0 : q0), lane);
                e_hi = wave_lower(tb.col, e_lo, (int32_t)r1, (int32_t)(q0 + width < tb.P ? q0 + width : tb.P), lane);
            }
        }
    }
    int64_t ubase = 0;
    int32_t u_lo = 0, u_hi = 0;
    if (e_hi > e_lo && tb.nnzU > 0) {
        const int64_t u = load_id(in.user, in.user64, g * in.ld_user) - in.user_offset;
        if (u >= 0 && u < tb.U) {                                       // (U * P * P < 2^63: no key overflows)
            ubase = (u * tb.P + (a - 1)) * tb.P;
            u_lo = wave_lower(tb.ukey, 0, (int32_t)tb.nnzU, ubase, lane);
            u_hi = wave_lower(tb.ukey, u_lo, (int32_t)tb.nnzU, ubase + tb.P, lane);
        }
    }
    for (int32_t e = e_lo + tid; e < e_hi; e += TPB) {
        const int64_t q = tb.col[e];
        if (q < 0 || q >= tb.P) {                                       // (possible only where col does not ascend)
            flag = true;
            continue;
        }
        const int64_t j = q + 1 - in.label_offset - c0;
        if (j < 0 || j >= width) continue;                              // not a column of this chunk, or of the scores at all
        const float l = tb.lg[e];
        if (!(l > 0.0f)) continue;                                      // cg(a, p) = 0: cu(u, a, p) is not looked up
        float s = __fadd_rn(tile[j], __fmul_rn(wg, l));
        if (u_hi > u_lo) {
            const int32_t at = lower(tb.ukey, u_lo, u_hi, ubase + q);
            if (at < u_hi && tb.ukey[at] == ubase + q) {
                const float m = tb.lu[at];
                if (m > 0.0f) s = __fadd_rn(s, __fmul_rn(wu, m));
            }
        }
        tile[j] = s;
    }
    if (flag || (row_flag && tid == 0)) atomicOr(status, MOBGT_PRIOR_SBADINDEX);
    __syncthreads();
    float* dst = in.out + g * in.ld_out + c0;
    for (int32_t j = tid; j < width; j += TPB) dst[j] = tile[j];
}

}  // namespace

extern "C" int mobgt_prior_abi_version(void) { return MOBGT_PRIOR_ABI_VERSION; }

extern "C" int mobgt_prior_blend_rows(const float* scores, int64_t ld_scores, float* out, int64_t ld_out, int64_t G, int64_t V,
                                      int64_t label_offset, const void* hist, int hist_dtype, int64_t ld_hist, int64_t n_hist_cols,
                                      const void* user, int user_dtype, int64_t ld_user, int64_t user_offset, const void* rowptr,
                                      const void* col, const float* lg, int64_t nnz, const void* ukey, const float* lu, int64_t nnzU,
                                      int64_t U, const float* lp, int64_t P, const float* weights, void* status, void* stream) {
    const Rows in = {{scores, out, ld_scores, ld_out, V, label_offset, hist, ld_hist, n_hist_cols}, user, ld_user, user_offset,
                     hist_dtype == MOBGT_PRIOR_I64, user_dtype == MOBGT_PRIOR_I64};
    if (bad_rows_dims(in, G, MOBGT_PRIOR_MAX_G) || bad_size(nnz) || bad_size(nnzU) || P < 1 || P > INT32_MAX || U < 0 ||
        U > INT64_MAX / (P * P) || ld_user < 1 || user_offset < 0 || user_offset > 1)
        return MOBGT_PRIOR_EBADDIM;
    if (bad_id_dtype(hist_dtype) || bad_id_dtype(user_dtype)) return MOBGT_PRIOR_EDTYPE;
    if (bad_rows_ptrs(in, in.hist64, G) || bad_ptr(user, in.user64 ? 8 : 4, G) || bad_ptr(rowptr, 8, P + 1) || bad_ptr(col, 4, nnz) ||
        bad_ptr(lg, 4, nnz) || bad_ptr(ukey, 8, nnzU) || bad_ptr(lu, 4, nnzU) || bad_ptr(lp, 4, P) || bad_ptr(weights, 4, 3) ||
        bad_ptr(status, 4, 1))
        return MOBGT_PRIOR_EALIGN;
    if (G == 0 || V == 0) return 0;
    const Tables tb = {(const int64_t*)rowptr, (const int32_t*)col, lg, nnz, (const int64_t*)ukey, lu, nnzU, U, lp, P};
    const dim3 grid((unsigned)((V + CHUNK - 1) / CHUNK), (unsigned)G);
    hipLaunchKernelGGL(blend_kernel, grid, dim3(TPB), 0, (hipStream_t)stream, in, tb, weights, (int32_t*)status);
    const hipError_t err = hipGetLastError();
    return err != hipSuccess ? (int)err : 0;
}
