// mobgt_sessions_to_raw (include/mobgt_data.h): check-in sessions -> the raw trajectory-graph arrays of a padded batch, the
// device form of graphormer/gen_pickles.py:755-832.  One workgroup per session:
//
//   1. the history's POIs go to LDS; every check-in i finds the LAST position of its POI by scanning back from the end
//      (O(L^2) compares in the worst case, all on LDS; neighbouring threads read the same word, a broadcast);
//   2. a check-in that is its own last occurrence is a node; its node index is the number of such check-ins in front of it
//      (drop_duplicates(keep='last') keeps visit order): a workgroup prefix sum over the flags;
//   3. the workgroup writes every element of its outputs: the node arrays, zeros beyond n, a zero fill of its counts tile
//      (16-byte stores);
//   4. after a barrier it counts the L - 1 transitions: in LDS (ds_add) when n <= 64 -- few cells, many increments, the
//      case where a global atomic would serialise on one address -- and copies the n x n block out with plain stores;
//      otherwise global integer atomics on its own tile, which nobody else touches.
//
// Integer counts: the result does not depend on the order of the increments.  No workgroup reads what another writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_data.h"

namespace {

constexpr int TPB = 1024;                          // threads per workgroup
constexpr int MAXL = MOBGT_DATA_MAX_LP;
constexpr int PER = MAXL / TPB;                    // consecutive check-ins a thread owns in the prefix sum
constexpr int SMALL_N = 64;                        // up to this many nodes the transitions are counted in LDS
static_assert(MAXL % TPB == 0 && MAXL <= 65536, "positions are kept as 16-bit words");

__device__ __forceinline__ void zero_fill(int* p, size_t count, int t) {
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4;           // (p is 4-byte aligned: checked at entry)
    if (head > count) head = count;
    if ((size_t)t < head) p[t] = 0;
    int4* v = reinterpret_cast<int4*>(p + head);
    const size_t nv = (count - head) / 4;
    for (size_t q = t; q < nv; q += TPB) v[q] = make_int4(0, 0, 0, 0);
    const size_t tail0 = head + nv * 4;
    if ((size_t)t < count - tail0) p[tail0 + t] = 0;
}

__global__ __launch_bounds__(TPB) void sessions_kernel(const int* __restrict__ seq, const int* __restrict__ len, int* __restrict__ counts,
                                                       int* __restrict__ x, int* __restrict__ time, int* __restrict__ cat,
                                                       float* __restrict__ time_normal, int* __restrict__ n_nodes,
                                                       int* __restrict__ status, int Lp, int N) {
    __shared__ int s_poi[MAXL];
    __shared__ unsigned short s_last[MAXL];        // position of the last occurrence of check-in i's POI
    __shared__ unsigned short s_rk[MAXL];          // node index, at positions that are a last occurrence
    __shared__ int s_scan[TPB];
    __shared__ int s_cnt[SMALL_N * SMALL_N];
    const int g = blockIdx.x, t = threadIdx.x;
    const int L0 = len[g];
    const bool len_ok = L0 >= 1 && L0 <= Lp;
    const int L = len_ok ? L0 : 0;
    const int* sq = seq + (size_t)g * Lp * 3;

    for (int i = t; i < L; i += TPB) s_poi[i] = sq[3 * i];
    __syncthreads();
    for (int i = t; i < L; i += TPB) {
        const int p = s_poi[i];
        int j = L - 1;
        while (s_poi[j] != p) --j;                 // (stops at j = i at the latest)
        s_last[i] = (unsigned short)j;
    }
    __syncthreads();

    int flag[PER], mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = t * PER + k;
        flag[k] = (i < L && s_last[i] == i) ? 1 : 0;
        mine += flag[k];
    }
    s_scan[t] = mine;
    __syncthreads();
    for (int off = 1; off < TPB; off <<= 1) {      // inclusive prefix sum over the threads' flag counts
        const int v = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    const int n_all = s_scan[TPB - 1];
    const bool ok = len_ok && n_all <= N;          // (the same in every thread of the workgroup)
    const int n = ok ? n_all : 0;
    int rank = s_scan[t] - mine;
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (flag[k]) s_rk[t * PER + k] = (unsigned short)rank++;

    // ---- every output element of graph g: node arrays, padding, the zeroed counts tile
    int* xg = x + (size_t)g * N;
    int* tg = time + (size_t)g * N;
    int* cg = cat + (size_t)g * N;
    float* ng = time_normal + (size_t)g * N;
    for (int a = n + t; a < N; a += TPB) {
        xg[a] = 0; tg[a] = 0; cg[a] = 0; ng[a] = 0.0f;
    }
    if (ok) {
        rank = s_scan[t] - mine;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (!flag[k]) continue;
            const int i = t * PER + k, a = rank++;
            const int tm = sq[3 * i + 1];
            xg[a] = s_poi[i];
            tg[a] = tm;
            cg[a] = sq[3 * i + 2];
            ng[a] = tm == 0 ? 0.0f : (float)((double)tm / 48.0);      // gen_pickles.py:805-809: a double quotient, then float
        }
    }
    if (t == 0) {
        n_nodes[g] = n;
        status[g] = !len_ok ? MOBGT_DATA_SBADLEN : (n_all > N ? MOBGT_DATA_SNODES : MOBGT_DATA_SOK);
    }
    int* tile = counts + (size_t)g * N * N;
    zero_fill(tile, (size_t)N * N, t);
    if (!ok) return;
    if (n <= SMALL_N) {
        for (int c = t; c < n * n; c += TPB) s_cnt[c] = 0;
        __syncthreads();                           // (also: s_rk complete, the tile's zeros ordered before the stores below)
        for (int i = 1 + t; i < L; i += TPB)
            atomicAdd(&s_cnt[(int)s_rk[s_last[i - 1]] * n + (int)s_rk[s_last[i]]], 1);
        __syncthreads();
        for (int c = t; c < n * n; c += TPB) tile[(size_t)(c / n) * N + c % n] = s_cnt[c];
    } else {
        __syncthreads();                           // s_rk complete; the tile's zeros are visible to the workgroup's atomics
        for (int i = 1 + t; i < L; i += TPB)
            atomicAdd(&tile[(size_t)s_rk[s_last[i - 1]] * N + s_rk[s_last[i]]], 1);
    }
}

bool bad_ptr(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

}  // namespace

extern "C" int mobgt_data_abi_version(void) { return MOBGT_DATA_ABI_VERSION; }

extern "C" int mobgt_sessions_to_raw(const void* seq, const void* len, void* counts, void* x, void* time, void* cat, void* time_normal,
                                     void* n_nodes, void* status, int G, int Lp, int N, void* stream) {
    if (G < 0 || Lp < 1 || Lp > MOBGT_DATA_MAX_LP || N < 1 || N > MOBGT_DATA_MAX_N) return MOBGT_DATA_EBADDIM;
    if (G == 0) return 0;
    if (bad_ptr(seq) || bad_ptr(len) || bad_ptr(counts) || bad_ptr(x) || bad_ptr(time) || bad_ptr(cat) || bad_ptr(time_normal) ||
        bad_ptr(n_nodes) || bad_ptr(status))
        return MOBGT_DATA_EALIGN;
    hipLaunchKernelGGL(sessions_kernel, dim3(G), dim3(TPB), 0, (hipStream_t)stream, (const int*)seq, (const int*)len, (int*)counts,
                       (int*)x, (int*)time, (int*)cat, (float*)time_normal, (int*)n_nodes, (int*)status, Lp, N);
    return (int)hipGetLastError();
}
