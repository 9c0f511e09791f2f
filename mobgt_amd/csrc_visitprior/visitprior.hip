// include/mobgt_visitprior.h: the per-user visit-frequency and recency prior -- the two launches of its fit around torch's sort and
// cumsum, and the two fitted tables blended into a model's scores.  The rule is the docstring of mobgt_amd/visitprior.py; the
// header repeats it in short.
//
// keys_kernel -- a thread per packed check-in: the 64-bit key u * P + (p - 1) and the row's number among its user's train rows,
// written to the slot the host's cumsum gave the row's session.  fill_kernel -- over the sorted keys, a thread per key and per
// user: the first key of a run writes the run's col, cnt (the run's length, by a bisection for its end) and age (from the last
// number of the run: the sort is stable, so the numbers ascend inside a run), and thread u writes rowptr[u].  Both are
// ../csrc_universe/counts.hip's scheme with a 64-bit key by user and one more column.  Integers and plain stores only.
//
// blend_kernel -- ONE WORKGROUP PER (CHUNK OF COLUMNS, ROW), and the work is sparse: a user has tens to hundreds of entries
// among up to 100 001 columns.  So the columns are not looked up one by one.  Out of place the workgroup copies its chunk at full
// width (16-byte loads and stores where both rows allow it); then it takes the user's CSR row -- all of it where it has at most
// THREADS entries, as most users' have: a thread an entry, no search to wait for; of a longer row the part that falls into the
// chunk, which every wave finds with two searches in the ascending col (wave_lower of ../csrc_prior/blend_rows.h) -- and after
// one barrier -- the copy's stores come before the entries' -- a thread per entry checks that the entry is one of the chunk's,
// reads the SCORE (never the copy), adds the two terms and stores.  A chunk without entries is a plain copy; in place nothing
// is copied, so such a chunk writes nothing and a chunk with entries writes those elements only.  Every element is read and written by its own workgroup only, so in place is safe.
//
// Built with -ffp-contract=off (Makefile): a term is one product and one sum, each rounded on its own.  No workgroup reads what
// another writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_visitprior.h"
#include "../csrc_prior/blend_rows.h"

namespace {

constexpr int TPB = MOBGT_VISITPRIOR_THREADS;
constexpr int CHUNK = MOBGT_VISITPRIOR_CHUNK;
constexpr int PER_LANE = 4;                        // columns of one 16-byte load
constexpr int64_t KEY_LIMIT = (int64_t)1 << MOBGT_VISITPRIOR_KEY_BITS;
static_assert(TPB % WAVE == 0 && CHUNK % PER_LANE == 0, "whole waves; a chunk starts 16-byte aligned where its row does");
static_assert(MOBGT_VISITPRIOR_I32 == ROWS_I32 && MOBGT_VISITPRIOR_I64 == ROWS_I64, "blend_rows.h's dtype codes are this header's");

__global__ __launch_bounds__(TPB) void keys_kernel(const int32_t* __restrict__ seq, const int32_t* __restrict__ sid, int64_t M,
                                                   const int64_t* __restrict__ first, const int64_t* __restrict__ slot0,
                                                   const int64_t* __restrict__ ord0, const int64_t* __restrict__ users, int64_t S, int64_t P,
                                                   int64_t U, int64_t* __restrict__ keys, int32_t* __restrict__ ord, int64_t T,
                                                   int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= M) return;
    int bad = 0;
    const int64_t s = sid[i];
    if (s < 0 || s >= S) {
        bad = MOBGT_VISITPRIOR_SBADINDEX;
    } else if (slot0[s] >= 0) {                                         // a train session
        const int64_t at = first[s], base = slot0[s];
        if (at < 0 || at > i || base >= T || i - at >= T - base) {      // (checked before a sum: no sum overflows)
            bad = MOBGT_VISITPRIOR_SBADINDEX;
        } else {
            const int64_t k = i - at, slot = base + k;                  // 0 <= k < M, 0 <= slot < T
            const int64_t p = seq[3 * i], u = users[s], n0 = ord0[s];
            if (p < 1 || p > P || u < 0 || u >= U || n0 < 0 || n0 > INT32_MAX - k) {
                bad = MOBGT_VISITPRIOR_SBADVALUE;                       // the key stays -1
            } else {
                keys[slot] = u * P + (p - 1);                           // (U * P < 2^62)
                ord[slot] = (int32_t)(n0 + k);
            }
        }
    }
    if (bad) atomicOr(status, bad);
}

// thread i: key i (its run's col, cnt and age, if it is the first of its run) and user i (rowptr[i])
__global__ __launch_bounds__(TPB) void fill_kernel(const int64_t* __restrict__ keys, const int32_t* __restrict__ ord, const int64_t* __restrict__ pos,
                                                   int64_t T, int64_t P, int64_t U, int64_t nnz, const int32_t* __restrict__ tot,
                                                   int64_t* __restrict__ rowptr, int32_t* __restrict__ col, int32_t* __restrict__ cnt,
                                                   int32_t* __restrict__ age, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < T) {
        const int64_t k = keys[i];
        if (i == 0 || keys[i - 1] != k) {
            const int64_t r = pos[i] - 1;
            bool ok = r >= 0 && r < nnz && k >= 0 && k < U * P;         // (a run index from elsewhere is never an index)
            if (ok) {
                int64_t lo = i + 1, hi = T;                             // the first key above k
                while (lo < hi) {
                    const int64_t mid = lo + (hi - lo) / 2;
                    if (keys[mid] <= k) lo = mid + 1; else hi = mid;
                }
                const int64_t u = k / P;
                const int64_t n = tot[u], a = n - 1 - ord[lo - 1];      // lo - 1 in [i, T)
                ok = a >= 0 && a < n;
                if (ok) {
                    col[r] = (int32_t)(k - u * P);
                    cnt[r] = (int32_t)(lo - i);
                    age[r] = (int32_t)a;
                }
            }
            if (!ok) atomicOr(status, MOBGT_VISITPRIOR_SBADVALUE);
        }
    }
    if (i <= U) {
        const int64_t target = i * P;
        int64_t lo = 0, hi = T;                                         // the first key at or above user i's first
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < target) lo = mid + 1; else hi = mid;
        }
        rowptr[i] = lo == 0 ? 0 : pos[lo - 1];
    }
}

struct Rows : BlendRows {
    int hist64;
    const void* user;
    int64_t ld_user, user_offset;
    int user64;
};

struct Tables {
    const int64_t* rowptr;
    const int32_t* col;
    const float* freq;
    const float* rec;
    int64_t nnz, U, P;
};

__global__ __launch_bounds__(TPB) void blend_kernel(Rows in, Tables tb, const float* __restrict__ weights, int32_t* __restrict__ status) {
    const int tid = threadIdx.x, lane = tid % WAVE;
    const int64_t g = blockIdx.y;
    const int64_t c0 = (int64_t)blockIdx.x * CHUNK;                     // < V
    const int32_t width = (int32_t)(in.V - c0 < CHUNK ? in.V - c0 : CHUNK);
    const float* src = in.scores + g * in.ld_scores + c0;
    float* dst = in.out + g * in.ld_out + c0;
    const bool in_place = src == dst;                                   // (out is scores, and then with one row stride)

    if (!in_place) {                                                    // the chunk as it is, bit for bit
        if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
            const int32_t whole = width / PER_LANE * PER_LANE;
            for (int32_t j = tid * PER_LANE; j < whole; j += TPB * PER_LANE)
                *reinterpret_cast<float4*>(dst + j) = *reinterpret_cast<const float4*>(src + j);
            for (int32_t j = whole + tid; j < width; j += TPB) dst[j] = src[j];
        } else {
            for (int32_t j = tid; j < width; j += TPB) dst[j] = src[j];
        }
    }

    // the user's entries inside this chunk: the same values in every lane of the workgroup, each checked before it is used
    int32_t e_lo = 0, e_hi = 0;
    bool row_flag = false, flag = false;
    const int64_t u = load_id(in.user, in.user64, g * in.ld_user) - in.user_offset;
    if (u >= 0 && u < tb.U) {
        const int64_t r0 = tb.rowptr[u], r1 = tb.rowptr[u + 1];
        if (r0 < 0 || r1 < r0 || r1 > tb.nnz) {
            row_flag = true;                                            // the row counts as empty
        } else if (r1 - r0 <= TPB) {
            // a short row, as most users': a thread an entry, and the checks below keep the chunk's -- no search to wait for
            e_lo = (int32_t)r0;
            e_hi = (int32_t)r1;
        } else {
            // col ascends inside a row: entries outside [0, P) stand at its ends, and no chunk's part holds them
            if (tb.col[r0] < 0 || tb.col[r1 - 1] >= tb.P) row_flag = true;
            // POI (0-based) q is column q + 1 - label_offset: the chunk is the POIs [q0, q0 + width)
            const int64_t q0 = c0 + in.label_offset - 1;
            e_lo = wave_lower(tb.col, (int32_t)r0, (int32_t)r1, (int32_t)(q0 < 0 ? 0 : q0), lane);
            e_hi = wave_lower(tb.col, e_lo, (int32_t)r1, (int32_t)(q0 + width < tb.P ? q0 + width : tb.P), lane);
        }
    }
    if (e_hi > e_lo) {                                                  // (the same in every lane: the barrier is met by all or by none)
        if (!in_place) __syncthreads();                                 // the copy's stores, then the entries'
        const float wv = weights[0], wr = weights[1];
        for (int32_t e = e_lo + tid; e < e_hi; e += TPB) {
            const int64_t q = tb.col[e];
            if (q < 0 || q >= tb.P) {                                   // (in a short row, or where col does not ascend)
                flag = true;
                continue;
            }
            const int64_t j = q + 1 - in.label_offset - c0;
            if (j < 0 || j >= width) continue;                          // not a column of this chunk, or of the scores at all
            float v = src[j];
            v = __fadd_rn(v, __fmul_rn(wv, tb.freq[e]));
            v = __fadd_rn(v, __fmul_rn(wr, tb.rec[e]));
            dst[j] = v;
        }
    }
    if (flag || (row_flag && tid == 0)) atomicOr(status, MOBGT_VISITPRIOR_SBADINDEX);
}

bool bad_universe(int64_t P, int64_t U) { return P < 1 || P > INT32_MAX || U < 0 || U > INT32_MAX || U > (KEY_LIMIT - 1) / P; }

unsigned blocks(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

}  // namespace

extern "C" int mobgt_visitprior_abi_version(void) { return MOBGT_VISITPRIOR_ABI_VERSION; }

extern "C" int mobgt_visitprior_keys(const void* seq, const void* sid, int64_t M, const void* first, const void* slot0, const void* ord0,
                                     const void* users, int64_t S, int64_t P, int64_t U, void* keys, void* ord, int64_t T, void* status,
                                     void* stream) {
    if (bad_size(M) || bad_size(S) || bad_size(T) || bad_universe(P, U)) return MOBGT_VISITPRIOR_EBADDIM;
    if (bad_ptr(seq, 4, M) || bad_ptr(sid, 4, M) || bad_ptr(first, 8, S) || bad_ptr(slot0, 8, S) || bad_ptr(ord0, 8, S) ||
        bad_ptr(users, 8, S) || bad_ptr(keys, 8, T) || bad_ptr(ord, 4, T) || bad_ptr(status, 4, 1))
        return MOBGT_VISITPRIOR_EALIGN;
    if (M == 0 || T == 0) return 0;
    const hipError_t rc = hipMemsetAsync(keys, 0xFF, (size_t)T * sizeof(int64_t), (hipStream_t)stream);    // every key -1
    if (rc != hipSuccess) return (int)rc;
    hipLaunchKernelGGL(keys_kernel, dim3(blocks(M)), dim3(TPB), 0, (hipStream_t)stream, (const int32_t*)seq, (const int32_t*)sid, M,
                       (const int64_t*)first, (const int64_t*)slot0, (const int64_t*)ord0, (const int64_t*)users, S, P, U, (int64_t*)keys,
                       (int32_t*)ord, T, (int32_t*)status);
    return (int)hipGetLastError();
}

extern "C" int mobgt_visitprior_fill(const void* keys, const void* ord, const void* pos, int64_t T, int64_t P, int64_t U, int64_t nnz,
                                     const void* tot, void* rowptr, void* col, void* cnt, void* age, void* status, void* stream) {
    if (bad_size(T) || nnz < 0 || nnz > T || bad_universe(P, U)) return MOBGT_VISITPRIOR_EBADDIM;
    if (bad_ptr(keys, 8, T) || bad_ptr(ord, 4, T) || bad_ptr(pos, 8, T) || bad_ptr(tot, 4, U) || bad_ptr(rowptr, 8, U + 1) ||
        bad_ptr(col, 4, nnz) || bad_ptr(cnt, 4, nnz) || bad_ptr(age, 4, nnz) || bad_ptr(status, 4, 1))
        return MOBGT_VISITPRIOR_EALIGN;
    hipLaunchKernelGGL(fill_kernel, dim3(blocks(T > U + 1 ? T : U + 1)), dim3(TPB), 0, (hipStream_t)stream, (const int64_t*)keys,
                       (const int32_t*)ord, (const int64_t*)pos, T, P, U, nnz, (const int32_t*)tot, (int64_t*)rowptr, (int32_t*)col,
                       (int32_t*)cnt, (int32_t*)age, (int32_t*)status);
    return (int)hipGetLastError();
}

extern "C" int mobgt_visitprior_blend_rows(const float* scores, int64_t ld_scores, float* out, int64_t ld_out, int64_t G, int64_t V,
                                           int64_t label_offset, const void* hist, int hist_dtype, int64_t ld_hist, int64_t n_hist_cols,
                                           const void* user, int user_dtype, int64_t ld_user, int64_t user_offset, const void* rowptr,
                                           const void* col, const float* freq, const float* rec, int64_t nnz, int64_t U, int64_t P,
                                           const float* weights, void* status, void* stream) {
    const Rows in = {{scores, out, ld_scores, ld_out, V, label_offset, hist, ld_hist, n_hist_cols}, hist_dtype == MOBGT_VISITPRIOR_I64,
                     user, ld_user, user_offset, user_dtype == MOBGT_VISITPRIOR_I64};
    if (bad_rows_dims(in, G, MOBGT_VISITPRIOR_MAX_G) || bad_size(nnz) || bad_universe(P, U) || ld_user < 1 || user_offset < 0 ||
        user_offset > 1)
        return MOBGT_VISITPRIOR_EBADDIM;
    if (bad_id_dtype(hist_dtype) || bad_id_dtype(user_dtype)) return MOBGT_VISITPRIOR_EDTYPE;
    if (bad_rows_ptrs(in, in.hist64, G) || bad_ptr(user, in.user64 ? 8 : 4, G) || bad_ptr(rowptr, 8, U + 1) || bad_ptr(col, 4, nnz) ||
        bad_ptr(freq, 4, nnz) || bad_ptr(rec, 4, nnz) || bad_ptr(weights, 4, 2) || bad_ptr(status, 4, 1))
        return MOBGT_VISITPRIOR_EALIGN;
    if (G == 0 || V == 0) return 0;
    const Tables tb = {(const int64_t*)rowptr, (const int32_t*)col, freq, rec, nnz, U, P};
    const dim3 grid((unsigned)((V + CHUNK - 1) / CHUNK), (unsigned)G);
    hipLaunchKernelGGL(blend_kernel, grid, dim3(TPB), 0, (hipStream_t)stream, in, tb, weights, (int32_t*)status);
    const hipError_t err = hipGetLastError();
    return err != hipSuccess ? (int)err : 0;
}
