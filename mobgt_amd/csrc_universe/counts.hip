// include/mobgt_universe.h: the POI table's counts, Graph_cat and the keys of Graph_adj from packed check-in sessions, and the
// CSR of Graph_adj from the sorted keys.
//
// counts_kernel -- one thread per check-in, a workgroup owns CHUNK contiguous check-ins.  The POI-sized counters (checkin_cnt,
// poi_cat_min / max) are scattered over P addresses: global integer atomics.  The category counters are the opposite case, every
// check-in hits one of a few hundred addresses: they are kept in the workgroup's LDS (integer atomics there) and flushed once,
// non-zero counters only: cat_cnt always, graph_cat while it fits (the header's threshold), beyond that global integer atomics.  The P^2 space of POI pairs
// is never counted into: every train transition stores its 64-bit key at a slot the host fixed, the caller sorts the keys, and
// run_heads_kernel / run_fill_kernel read the runs of equal keys off the sorted array.
//
// Every id is checked before it is an index; what fails is skipped and reported in status[0].  Integer atomics and plain
// stores only: exact, and independent of the order the workgroups run in.  No workgroup reads what another writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_universe.h"

namespace {

constexpr int TPB = 256;
constexpr int CHUNK = MOBGT_UNIVERSE_CHUNK;
constexpr int FILL_BLOCKS = 2048;

// every output of mobgt_universe_counts at its start value: n = max(P, n_cat^2, T, 1) indices, grid-stride
__global__ __launch_bounds__(TPB) void start_kernel(int64_t n, int64_t P, int64_t n_cat, int64_t T, int32_t* __restrict__ checkin_cnt,
                                                    int32_t* __restrict__ cat_cnt, int32_t* __restrict__ poi_cat_min,
                                                    int32_t* __restrict__ poi_cat_max, int32_t* __restrict__ graph_cat,
                                                    int64_t* __restrict__ keys, int32_t* __restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        if (i < P) {
            checkin_cnt[i] = 0;
            poi_cat_min[i] = INT32_MAX;
            poi_cat_max[i] = 0;
        }
        if (i < n_cat) cat_cnt[i] = 0;
        if (i < n_cat * n_cat) graph_cat[i] = 0;
        if (i < T) keys[i] = -1;
        if (i == 0) status[0] = 0;
    }
}

// Workgroup blockIdx.x owns check-ins blockIdx.x * CHUNK .. + CHUNK - 1.  s_mem: [cat_cnt][graph_cat if lds_gc].
__global__ __launch_bounds__(TPB) void counts_kernel(const int32_t* __restrict__ seq, const int32_t* __restrict__ sid, int64_t M,
                                                     const int32_t* __restrict__ first, const int32_t* __restrict__ slot0, int64_t S,
                                                     int64_t P, int n_cat, int lds_gc, int32_t* __restrict__ checkin_cnt,
                                                     int32_t* __restrict__ cat_cnt, int32_t* __restrict__ poi_cat_min,
                                                     int32_t* __restrict__ poi_cat_max, int32_t* __restrict__ graph_cat,
                                                     int64_t* __restrict__ keys, int64_t T, int32_t* __restrict__ status) {
    extern __shared__ int32_t s_mem[];
    int32_t* s_cnt = s_mem;
    int32_t* s_gc = s_mem + n_cat;
    const int t = threadIdx.x;
    const int n_lds = n_cat + (lds_gc ? n_cat * n_cat : 0);
    for (int k = t; k < n_lds; k += TPB) s_mem[k] = 0;
    __syncthreads();

    const int64_t base = (int64_t)blockIdx.x * CHUNK;
    const int64_t end = base + CHUNK < M ? base + CHUNK : M;
    for (int64_t i = base + t; i < end; i += TPB) {
        const int64_t p = seq[3 * i], c = seq[3 * i + 2], s = sid[i];
        const bool okp = p >= 1 && p <= P, okc = c >= 1 && c <= n_cat, oks = s >= 0 && s < S;
        int bad = (okp ? 0 : MOBGT_UNIVERSE_SBADPOI) | (okc ? 0 : MOBGT_UNIVERSE_SBADCAT) | (oks ? 0 : MOBGT_UNIVERSE_SBADSESSION);
        if (okp && okc) {
            atomicAdd(&checkin_cnt[p - 1], 1);
            atomicMin(&poi_cat_min[p - 1], (int32_t)c);
            atomicMax(&poi_cat_max[p - 1], (int32_t)c);
            atomicAdd(&s_cnt[c - 1], 1);
            if (oks && i > 0 && sid[i - 1] == s && slot0[s] >= 0) {                 // a transition inside one train session
                const int64_t p0 = seq[3 * (i - 1)], c0 = seq[3 * (i - 1) + 2];
                if (p0 >= 1 && p0 <= P && c0 >= 1 && c0 <= n_cat) {                 // (else: check-in i - 1 reports itself)
                    const int64_t pair = (c0 - 1) * n_cat + (c - 1);
                    if (lds_gc) atomicAdd(&s_gc[pair], 1); else atomicAdd(&graph_cat[pair], 1);
                    const int64_t k = i - first[s] - 1, slot = slot0[s] + k;
                    if (k >= 0 && slot < T)
                        keys[slot] = (p0 - 1) * P + (p - 1);
                    else
                        bad |= MOBGT_UNIVERSE_SBADSESSION;
                }
            }
        }
        if (bad) atomicOr(status, bad);
    }
    __syncthreads();

    // the flush: a counter this workgroup never touched costs no atomic
    for (int k = t; k < n_cat; k += TPB)
        if (s_cnt[k]) atomicAdd(&cat_cnt[k], s_cnt[k]);
    if (lds_gc)
        for (int k = t; k < n_cat * n_cat; k += TPB)
            if (s_gc[k]) atomicAdd(&graph_cat[k], s_gc[k]);
}

__global__ __launch_bounds__(TPB) void run_heads_kernel(const int64_t* __restrict__ keys, int64_t T, int32_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < T) head[i] = i == 0 || keys[i] != keys[i - 1];
}

// thread i: key i (the run's col and val, if it is the first of its run) and row i (rowptr[i])
__global__ __launch_bounds__(TPB) void run_fill_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ pos, int64_t T, int64_t P,
                                                       int64_t nnz, int64_t* __restrict__ rowptr, int32_t* __restrict__ col,
                                                       int32_t* __restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < T) {
        const int64_t k = keys[i];
        if (i == 0 || keys[i - 1] != k) {
            const int64_t r = pos[i] - 1;
            if (r >= 0 && r < nnz && k >= 0 && k < P * P) {                         // (a run index from elsewhere is never an index)
                int64_t lo = i + 1, hi = T;                                         // the first key above k
                while (lo < hi) {
                    const int64_t mid = lo + (hi - lo) / 2;
                    if (keys[mid] <= k) lo = mid + 1; else hi = mid;
                }
                col[r] = (int32_t)(k % P);
                val[r] = (int32_t)(lo - i);
            }
        }
    }
    if (i <= P) {
        const int64_t target = i * P;
        int64_t lo = 0, hi = T;                                                     // the first key at or above row i's first
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < target) lo = mid + 1; else hi = mid;
        }
        rowptr[i] = lo == 0 ? 0 : pos[lo - 1];
    }
}

// null only where the buffer has no element
bool bad_ptr(const void* p, uintptr_t align, int64_t n) {
    return (p == nullptr && n > 0) || (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0;
}

}  // namespace

extern "C" int mobgt_universe_abi_version(void) { return MOBGT_UNIVERSE_ABI_VERSION; }

extern "C" int mobgt_universe_counts(const void* seq, const void* sid, int64_t M, const void* first, const void* slot0, int64_t S, int64_t P,
                                     int n_cat, void* checkin_cnt, void* cat_cnt, void* poi_cat_min, void* poi_cat_max, void* graph_cat,
                                     void* keys, int64_t T, void* status, void* stream) {
    if (M < 0 || M > INT32_MAX || S < 0 || T < 0 || T > INT32_MAX || P < 1 || P > MOBGT_UNIVERSE_MAX_P || n_cat < 1 ||
        n_cat > MOBGT_UNIVERSE_MAX_CAT)
        return MOBGT_UNIVERSE_EBADDIM;
    const int64_t ncat2 = (int64_t)n_cat * n_cat;
    if (bad_ptr(seq, 4, M) || bad_ptr(sid, 4, M) || bad_ptr(first, 4, S) || bad_ptr(slot0, 4, S) || bad_ptr(checkin_cnt, 4, P) ||
        bad_ptr(cat_cnt, 4, n_cat) || bad_ptr(poi_cat_min, 4, P) || bad_ptr(poi_cat_max, 4, P) || bad_ptr(graph_cat, 4, ncat2) ||
        bad_ptr(keys, 8, T) || bad_ptr(status, 4, 1))
        return MOBGT_UNIVERSE_EALIGN;
    int64_t n = P > ncat2 ? P : ncat2;
    n = T > n ? T : n;
    const int64_t fill_blocks = (n + TPB - 1) / TPB;
    hipLaunchKernelGGL(start_kernel, dim3((unsigned)(fill_blocks < FILL_BLOCKS ? fill_blocks : FILL_BLOCKS)), dim3(TPB), 0, (hipStream_t)stream,
                       n, P, (int64_t)n_cat, T, (int32_t*)checkin_cnt, (int32_t*)cat_cnt, (int32_t*)poi_cat_min, (int32_t*)poi_cat_max,
                       (int32_t*)graph_cat, (int64_t*)keys, (int32_t*)status);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || M == 0) return (int)err;
    const int lds_gc = n_cat <= MOBGT_UNIVERSE_LDS_MAX_CAT;
    const size_t lds = sizeof(int32_t) * ((size_t)n_cat + (lds_gc ? (size_t)ncat2 : 0));
    hipLaunchKernelGGL(counts_kernel, dim3((unsigned)((M + CHUNK - 1) / CHUNK)), dim3(TPB), lds, (hipStream_t)stream, (const int32_t*)seq,
                       (const int32_t*)sid, M, (const int32_t*)first, (const int32_t*)slot0, S, P, n_cat, lds_gc,
                       (int32_t*)checkin_cnt, (int32_t*)cat_cnt, (int32_t*)poi_cat_min, (int32_t*)poi_cat_max, (int32_t*)graph_cat,
                       (int64_t*)keys, T, (int32_t*)status);
    return (int)hipGetLastError();
}

extern "C" int mobgt_universe_run_heads(const void* keys, int64_t T, void* head, void* stream) {
    if (T < 1 || T > INT32_MAX) return MOBGT_UNIVERSE_EBADDIM;
    if (bad_ptr(keys, 8, T) || bad_ptr(head, 4, T)) return MOBGT_UNIVERSE_EALIGN;
    hipLaunchKernelGGL(run_heads_kernel, dim3((unsigned)((T + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, (const int64_t*)keys, T,
                       (int32_t*)head);
    return (int)hipGetLastError();
}

extern "C" int mobgt_universe_run_fill(const void* keys, const void* pos, int64_t T, int64_t P, int64_t nnz, void* rowptr, void* col, void* val,
                                       void* stream) {
    if (T < 0 || T > INT32_MAX || nnz < 0 || nnz > T || P < 1 || P > MOBGT_UNIVERSE_MAX_P) return MOBGT_UNIVERSE_EBADDIM;
    if (bad_ptr(keys, 8, T) || bad_ptr(pos, 8, T) || bad_ptr(rowptr, 8, P + 1) || bad_ptr(col, 4, nnz) || bad_ptr(val, 4, nnz))
        return MOBGT_UNIVERSE_EALIGN;
    const int64_t n = T > P + 1 ? T : P + 1;
    hipLaunchKernelGGL(run_fill_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, (const int64_t*)keys,
                       (const int64_t*)pos, T, P, nnz, (int64_t*)rowptr, (int32_t*)col, (int32_t*)val);
    return (int)hipGetLastError();
}
