// include/mobgt_baseline.h: the Markov baseline's exact target ranks and top-k lists.  The rule is the docstring of
// mobgt_amd/baseline.py; the header repeats it in short.
//
// Candidate p of a sample (user u, previous POI a, target t) has the key K(p) = (cu(u, a, p), cg(a, p), -pop_rank(p)), larger
// first.  Only the entries of row a of the cg CSR (G_a) have a key that is not (0, 0, -pop_rank): the kernels walk that row and
// settle the rest by popularity -- no array over all P candidates exists.
//
// ONE WAVE PER SAMPLE.  `inspect` checks everything a sample indexes with before anything of it is used, with the same values in
// every lane, so a sample that fails leaves its wave as a whole; what fails is reported in status[0].  The loops over a row, over
// the history and over pop_order stride 64 a step, a lane an element; whatever crosses lanes (shuffles, ballots) stands outside the
// loops whose bounds differ between lanes, or inside loops whose bounds are the same in every lane.  A wave reads the tables and
// writes its own sample's outputs only: no wave waits for another, no LDS, no __syncthreads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_baseline.h"

namespace {

constexpr int WAVE = MOBGT_BASELINE_WAVE;
constexpr int WAVES = MOBGT_BASELINE_SAMPLES_PER_BLOCK;
constexpr int TPB = WAVE * WAVES;
constexpr int MAX_L = MOBGT_BASELINE_MAX_L;
constexpr int MAX_BLOCKS = 1 << 20;                                     // (grid x block stays below 2^32 threads)

struct Samples {
    const int32_t* seq;
    const int64_t* offsets;
    const int64_t* users;
    int64_t S, M;
    const int32_t* session;
    const int32_t* cut;
    int64_t Q;
};

struct Tables {
    const int64_t* rowptr;
    const int32_t* col;
    const int32_t* val;
    int64_t nnz;
    const int64_t* ukey;
    const int32_t* uval;
    int64_t nnzU, U;
    const int32_t* pop_rank;
    int64_t P;
    int order;
};

// larger first: cu, then cg, then the smaller popularity rank
struct Key {
    int32_t cu, cg, pr;
};

__device__ inline bool above(const Key& x, const Key& y) {
    return x.cu != y.cu ? x.cu > y.cu : x.cg != y.cg ? x.cg > y.cg : x.pr < y.pr;
}

// a checked sample (everything below 2^31: M, nnz and nnzU are).  bad: its status bits
struct Sample {
    int64_t first;                                                      // the session's first row
    int64_t ubase;                                                      // the cu key of (u, a, POI 1)
    int32_t c, t;                                                       // history rows; the target, 1-based
    int32_t r0, n;                                                      // row a of the CSR: first entry, entries (0 under order 2)
    int32_t ulo, un;                                                    // the (u, a) range of the cu table: first entry, entries
    Key kt;                                                             // K(t)
    int32_t bad;
};

// the first i in [lo, hi) with a[i] >= x, hi if there is none; a ascending
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

// the count stored for x among the ascending keys a[lo .. hi), 0 where x is not one of them
template <class T>
__device__ inline int32_t count_of(const T* __restrict__ a, const int32_t* __restrict__ cnt, int32_t lo, int32_t hi, T x) {
    const int32_t i = lower(a, lo, hi, x);
    return i < hi && a[i] == x ? cnt[i] : 0;
}

__device__ inline Sample inspect(const Samples& in, const Tables& tb, int64_t q) {
    Sample r = {};
    r.bad = MOBGT_BASELINE_SBADINDEX;
    const int64_t s = in.session[q];
    if (s < 0 || s >= in.S) return r;
    const int64_t a0 = in.offsets[s], b0 = in.offsets[s + 1];
    if (a0 < 0 || b0 < a0 || b0 > in.M) return r;
    const int64_t c = in.cut[q];
    if (c < 1 || c > b0 - a0 - 1) return r;
    if (c > MAX_L) {
        r.bad = MOBGT_BASELINE_STOOLONG;
        return r;
    }
    const int64_t a = in.seq[3 * (a0 + c - 1)], t = in.seq[3 * (a0 + c)];
    if (a < 1 || a > tb.P || t < 1 || t > tb.P) return r;
    const int64_t r0 = tb.rowptr[a - 1], r1 = tb.rowptr[a];
    if (r0 < 0 || r1 < r0 || r1 > tb.nnz) return r;
    r.bad = 0;
    r.first = a0;
    r.c = (int32_t)c;
    r.t = (int32_t)t;
    r.r0 = (int32_t)r0;
    r.n = tb.order == MOBGT_BASELINE_ORDER_POPULARITY ? 0 : (int32_t)(r1 - r0);
    r.kt.pr = tb.pop_rank[t - 1];
    r.kt.cg = count_of(tb.col, tb.val, r.r0, r.r0 + r.n, (int32_t)(t - 1));
    if (tb.order == MOBGT_BASELINE_ORDER_USER && tb.nnzU > 0) {
        const int64_t u = in.users[s];
        if (u >= 0 && u < tb.U) {                                       // (U * P * P < 2^63: no key overflows)
            r.ubase = (u * tb.P + (a - 1)) * tb.P;
            r.ulo = lower(tb.ukey, 0, (int32_t)tb.nnzU, r.ubase);
            r.un = lower(tb.ukey, r.ulo, (int32_t)tb.nnzU, r.ubase + tb.P) - r.ulo;
            r.kt.cu = count_of(tb.ukey, tb.uval, r.ulo, r.ulo + r.un, r.ubase + (t - 1));
        }
    }
    return r;
}

// Entry i < r.n of the sample's row: its 0-based POI and its key.  false: col is outside [0, P) and nothing was looked up with it.
__device__ inline bool entry(const Tables& tb, const Sample& r, int32_t i, Key& k, int32_t& poi) {
    const int64_t e = (int64_t)r.r0 + i;
    poi = tb.col[e];
    if (poi < 0 || poi >= tb.P) return false;
    k.cg = tb.val[e];
    k.pr = tb.pop_rank[poi];
    k.cu = r.un ? count_of(tb.ukey, tb.uval, r.ulo, r.ulo + r.un, r.ubase + poi) : 0;
    return true;
}

__device__ inline int wave_sum(int v) {
#pragma unroll
    for (int d = WAVE / 2; d; d /= 2) v += __shfl_xor(v, d, WAVE);
    return v;
}

__global__ __launch_bounds__(WAVE) void clear_kernel(int32_t* __restrict__ status) {
    if (threadIdx.x == 0) status[0] = 0;
}

__global__ __launch_bounds__(TPB) void ranks_kernel(Samples in, Tables tb, int32_t* __restrict__ rank, uint8_t* __restrict__ revisit,
                                                    int32_t* __restrict__ status) {
    const int lane = threadIdx.x % WAVE;
    for (int64_t q = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE; q < in.Q; q += (int64_t)gridDim.x * WAVES) {
        const Sample r = inspect(in, tb, q);                            // (the same in every lane)
        if (r.bad) {
            if (lane == 0) {
                rank[q] = -1;
                revisit[q] = 0;
                atomicOr(status, r.bad);
            }
            continue;
        }
        int before = 0, more_popular = 0, flag = 0;
        for (int32_t i = lane; i < r.n; i += WAVE) {
            Key k;
            int32_t poi;
            if (entry(tb, r, i, k, poi)) {
                before += above(k, r.kt);
                more_popular += k.pr < r.kt.pr;
            } else {
                flag = 1;
            }
        }
        int hit = 0;
        for (int32_t j = lane; j < r.c; j += WAVE) hit |= in.seq[3 * (r.first + j)] == r.t;
        before = wave_sum(before);
        more_popular = wave_sum(more_popular);
        hit = __any(hit);
        flag = __any(flag);
        if (lane == 0) {
            // the POIs outside the row have the key (0, 0, -pop_rank): they precede t only where t's key is of that form too
            rank[q] = before + (r.kt.cu == 0 && r.kt.cg == 0 ? r.kt.pr - more_popular : 0);
            revisit[q] = hit ? 1 : 0;
            if (flag) atomicOr(status, MOBGT_BASELINE_SBADINDEX);
        }
    }
}

__global__ __launch_bounds__(TPB) void topk_kernel(Samples in, Tables tb, const int32_t* __restrict__ pop_order, int k,
                                                   int32_t* __restrict__ ids, int32_t* __restrict__ status) {
    const int lane = threadIdx.x % WAVE;
    for (int64_t q = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE; q < in.Q; q += (int64_t)gridDim.x * WAVES) {
        int32_t* __restrict__ out = ids + q * k;
        const Sample r = inspect(in, tb, q);                            // (the same in every lane)
        if (r.bad) {
            if (lane < k) out[lane] = -1;
            if (lane == 0) atomicOr(status, r.bad);
            continue;
        }
        int flag = 0;
        Key mine = {0, 0, 0};
        int32_t mine_poi = -1;                                          // (-1: this lane holds no entry)
        if (lane < r.n && !entry(tb, r, lane, mine, mine_poi)) {
            mine_poi = -1;
            flag = 1;
        }
        // the best entries of the row, best first: round j takes the largest key below the one round j - 1 took
        const int rounds = r.n < k ? r.n : k;
        Key prev = {0, 0, 0};
        int pos = 0;
        for (; pos < rounds; ++pos) {                                   // (every bound and the break are the same in every lane)
            Key best = {0, 0, 0};
            int32_t best_poi = -1;
            if (mine_poi >= 0 && (pos == 0 || above(prev, mine))) {
                best = mine;
                best_poi = mine_poi;
            }
            for (int32_t i = WAVE + lane; i < r.n; i += WAVE) {
                Key kk;
                int32_t poi;
                if (!entry(tb, r, i, kk, poi)) {
                    flag = 1;
                } else if ((pos == 0 || above(prev, kk)) && (best_poi < 0 || above(kk, best))) {
                    best = kk;
                    best_poi = poi;
                }
            }
#pragma unroll
            for (int d = WAVE / 2; d; d /= 2) {
                const Key o = {__shfl_xor(best.cu, d, WAVE), __shfl_xor(best.cg, d, WAVE), __shfl_xor(best.pr, d, WAVE)};
                const int32_t o_poi = __shfl_xor(best_poi, d, WAVE);
                if (o_poi >= 0 && (best_poi < 0 || above(o, best))) {
                    best = o;
                    best_poi = o_poi;
                }
            }
            // (equal keys exist only in tables that are no strict order; lane 0's choice then holds for the wave)
            prev = {__shfl(best.cu, 0, WAVE), __shfl(best.cg, 0, WAVE), __shfl(best.pr, 0, WAVE)};
            best_poi = __shfl(best_poi, 0, WAVE);
            if (best_poi < 0) break;                                    // (entries were skipped: the row has fewer than `rounds`)
            if (lane == 0) out[pos] = best_poi + 1;
        }
        // the rest by popularity, without the row's own POIs: all of them are in the list already (pos < k only where pos = n)
        for (int64_t base = 0; base < tb.P && pos < k; base += WAVE) {
            const int64_t j = base + lane;
            bool keep = false;
            int32_t poi = 0;
            if (j < tb.P) {
                poi = pop_order[j];
                if (poi < 0 || poi >= tb.P) {
                    flag = 1;
                } else {
                    const int32_t at = lower(tb.col, r.r0, r.r0 + r.n, poi);
                    keep = !(at < r.r0 + r.n && tb.col[at] == poi);
                }
            }
            const unsigned long long kept = __ballot(keep);
            const int slot = pos + __popcll(kept & ((1ull << lane) - 1));
            if (keep && slot < k) out[slot] = poi + 1;
            pos += __popcll(kept);
        }
        if (lane >= pos && lane < k) out[lane] = -1;                    // (P < k)
        if (__any(flag) && lane == 0) atomicOr(status, MOBGT_BASELINE_SBADINDEX);
    }
}

// null only where the buffer has no element
bool bad_ptr(const void* p, uintptr_t align, int64_t n) {
    return (p == nullptr && n > 0) || (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0;
}

bool bad_size(int64_t v) { return v < 0 || v > INT32_MAX; }

unsigned grid(int64_t Q) {
    const int64_t b = (Q + WAVES - 1) / WAVES;
    return (unsigned)(b < 1 ? 1 : b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

// the limits and pointers the two entry points share
int check(const void* seq, const void* offsets, const void* users, int64_t S, int64_t M, const void* session, const void* cut, int64_t Q,
          const void* rowptr, const void* col, const void* val, int64_t nnz, const void* ukey, const void* uval, int64_t nnzU, int64_t U,
          const void* pop_rank, int64_t P, int64_t order, const void* status) {
    if (bad_size(Q) || bad_size(S) || bad_size(M) || bad_size(nnz) || bad_size(nnzU) || P < 1 || P > INT32_MAX || U < 0 ||
        U > INT64_MAX / (P * P) || order < MOBGT_BASELINE_ORDER_USER || order > MOBGT_BASELINE_ORDER_POPULARITY)
        return MOBGT_BASELINE_EBADDIM;
    if (bad_ptr(seq, 4, M) || bad_ptr(offsets, 8, S + 1) || bad_ptr(users, 8, S) || bad_ptr(session, 4, Q) || bad_ptr(cut, 4, Q) ||
        bad_ptr(rowptr, 8, P + 1) || bad_ptr(col, 4, nnz) || bad_ptr(val, 4, nnz) || bad_ptr(ukey, 8, nnzU) || bad_ptr(uval, 4, nnzU) ||
        bad_ptr(pop_rank, 4, P) || bad_ptr(status, 4, 1))
        return MOBGT_BASELINE_EALIGN;
    return 0;
}

}  // namespace

#define LAUNCH(kernel, grid, block, ...)                                                            \
    do {                                                                                            \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);   \
        const hipError_t err_ = hipGetLastError();                                                  \
        if (err_ != hipSuccess) return (int)err_;                                                   \
    } while (0)

extern "C" int mobgt_baseline_abi_version(void) { return MOBGT_BASELINE_ABI_VERSION; }

extern "C" int mobgt_baseline_ranks(const void* seq, const void* offsets, const void* users, int64_t S, int64_t M, const void* session,
                                    const void* cut, int64_t Q, const void* rowptr, const void* col, const void* val, int64_t nnz,
                                    const void* ukey, const void* uval, int64_t nnzU, int64_t U, const void* pop_rank, int64_t P,
                                    int64_t order, void* rank, void* revisit, void* status, void* stream) {
    const int rc = check(seq, offsets, users, S, M, session, cut, Q, rowptr, col, val, nnz, ukey, uval, nnzU, U, pop_rank, P, order, status);
    if (rc) return rc;
    if (bad_ptr(rank, 4, Q) || bad_ptr(revisit, 1, Q)) return MOBGT_BASELINE_EALIGN;
    const Samples in = {(const int32_t*)seq, (const int64_t*)offsets, (const int64_t*)users, S, M, (const int32_t*)session,
                        (const int32_t*)cut, Q};
    const Tables tb = {(const int64_t*)rowptr, (const int32_t*)col, (const int32_t*)val, nnz, (const int64_t*)ukey, (const int32_t*)uval,
                       nnzU, U, (const int32_t*)pop_rank, P, (int)order};
    LAUNCH(clear_kernel, 1, WAVE, (int32_t*)status);
    if (Q > 0) LAUNCH(ranks_kernel, grid(Q), TPB, in, tb, (int32_t*)rank, (uint8_t*)revisit, (int32_t*)status);
    return 0;
}

extern "C" int mobgt_baseline_topk(const void* seq, const void* offsets, const void* users, int64_t S, int64_t M, const void* session,
                                   const void* cut, int64_t Q, const void* rowptr, const void* col, const void* val, int64_t nnz,
                                   const void* ukey, const void* uval, int64_t nnzU, int64_t U, const void* pop_rank, const void* pop_order,
                                   int64_t P, int64_t order, int64_t k, void* ids, void* status, void* stream) {
    const int rc = check(seq, offsets, users, S, M, session, cut, Q, rowptr, col, val, nnz, ukey, uval, nnzU, U, pop_rank, P, order, status);
    if (rc) return rc;
    if (k < 1 || k > MOBGT_BASELINE_MAX_K) return MOBGT_BASELINE_EBADDIM;
    if (bad_ptr(pop_order, 4, P) || bad_ptr(ids, 4, Q * k)) return MOBGT_BASELINE_EALIGN;
    const Samples in = {(const int32_t*)seq, (const int64_t*)offsets, (const int64_t*)users, S, M, (const int32_t*)session,
                        (const int32_t*)cut, Q};
    const Tables tb = {(const int64_t*)rowptr, (const int32_t*)col, (const int32_t*)val, nnz, (const int64_t*)ukey, (const int32_t*)uval,
                       nnzU, U, (const int32_t*)pop_rank, P, (int)order};
    LAUNCH(clear_kernel, 1, WAVE, (int32_t*)status);
    if (Q > 0) LAUNCH(topk_kernel, grid(Q), TPB, in, tb, (const int32_t*)pop_order, (int)k, (int32_t*)ids, (int32_t*)status);
    return 0;
}
