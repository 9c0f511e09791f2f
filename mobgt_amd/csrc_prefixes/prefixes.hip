// include/mobgt_prefixes.h: every prefix of a check-in session as a sample, with its n (distinct POIs of the history) and mult (the
// largest multiplicity there).
//
// occ_j = the number of rows i <= j of the session with the POI of row j.  n_c counts the j < c with occ_j == 1, mult_c is the
// largest occ_j with j < c: two inclusive scans along the session.  A wave takes 64 rows at a time, one row per lane.  The rows of
// its own chunk reach a lane by shuffle; the rows of the chunks before (the long form only) by broadcast reads of the session's
// POI column in LDS.
//
// A session's offsets and pcum entries are checked before anything of it is used (inspect); what fails is skipped and reported in
// status[0].  A wave reads and writes only its own session's rows and samples: no wave waits for another, and the two forms share
// no session (the short form takes L <= 64, the long form the rest).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_prefixes.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVE = MOBGT_PREFIXES_WAVE;
constexpr int WAVES = TPB / WAVE;
constexpr int MAX_L = MOBGT_PREFIXES_MAX_L;
constexpr int FILL_BLOCKS = 2048;
constexpr int SHORT_BLOCKS = 1 << 20;                                   // (grid x block stays below 2^32 threads)
constexpr int LONG_BLOCKS = 2048;

// a checked session: first row, history rows, first output position, samples (all below 2^31: M is); bad: its status bits
struct Session {
    int32_t a, L, p0, cnt, bad;
};

__device__ inline Session inspect(const int64_t* __restrict__ offsets, const int64_t* __restrict__ pcum, const uint8_t* __restrict__ keep,
                                  int64_t s, int64_t M, int64_t Q, int64_t h) {
    Session r = {0, 0, 0, 0, 0};
    const int64_t a = offsets[s], b = offsets[s + 1], p0 = pcum[s], p1 = pcum[s + 1];
    if (a < 0 || b < a || b > M || p0 < 0 || p1 < p0 || p1 > Q) {
        r.bad = MOBGT_PREFIXES_SBADINDEX;
        return r;
    }
    const int64_t L = b - a - 1;                                        // (-1: a session without a row)
    const int64_t cnt = (keep == nullptr || keep[s]) && L >= h ? L - h + 1 : 0;
    if (p1 - p0 != cnt) {
        r.bad = MOBGT_PREFIXES_SBADINDEX;
        return r;
    }
    if (cnt > 0 && L > MAX_L) {
        r.bad = MOBGT_PREFIXES_STOOLONG;
        return r;
    }
    r.a = (int32_t)a;
    r.L = (int32_t)L;
    r.p0 = (int32_t)p0;
    r.cnt = (int32_t)cnt;
    return r;
}

// How many of the chunk's rows 0 .. lane hold this lane's POI; `rows` (wave-uniform): the rows the chunk has.  Lanes beyond them
// take the shuffles and return a number nobody reads.
__device__ inline int chunk_occ(int32_t poi, int lane, int rows) {
    int occ = 0;
    for (int i = 0; i < rows; ++i) {
        const int32_t other = __shfl(poi, i, WAVE);
        occ += i <= lane && other == poi;
    }
    return occ;
}

// inclusive sum-scan and max-scan over the wave: six shuffle steps each
__device__ inline void scan(int& sum, int& most, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d *= 2) {
        const int s = __shfl_up(sum, d, WAVE), m = __shfl_up(most, d, WAVE);
        if (lane >= d) {
            sum += s;
            most = most > m ? most : m;
        }
    }
}

__device__ inline void store(int64_t q, int64_t s, int64_t c, int n, int most, int32_t* __restrict__ session, int32_t* __restrict__ cut,
                             int32_t* __restrict__ nn, int32_t* __restrict__ mult) {
    session[q] = (int32_t)s;
    cut[q] = (int32_t)c;
    nn[q] = n;
    mult[q] = most;
}

__global__ __launch_bounds__(TPB) void fill_kernel(int64_t Q, int32_t* __restrict__ session, int32_t* __restrict__ cut,
                                                   int32_t* __restrict__ nn, int32_t* __restrict__ mult, int32_t* __restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    const int64_t first = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (first == 0) status[0] = 0;
    for (int64_t q = first; q < Q; q += stride) {
        session[q] = -1;
        cut[q] = nn[q] = mult[q] = 0;
    }
}

// The short form.  Wave w of workgroup b takes sessions b * WAVES + w, + gridDim.x * WAVES, ...: every bound of the loop and every
// return inside it is wave-uniform, so every lane takes every shuffle.  No __syncthreads: the waves of a workgroup share nothing.
__global__ __launch_bounds__(TPB) void short_kernel(const int32_t* __restrict__ seq, const int64_t* __restrict__ offsets,
                                                    const int64_t* __restrict__ pcum, const uint8_t* __restrict__ keep, int64_t S, int64_t M,
                                                    int64_t Q, int64_t h, int32_t* __restrict__ session, int32_t* __restrict__ cut,
                                                    int32_t* __restrict__ nn, int32_t* __restrict__ mult, int32_t* __restrict__ status) {
    const int lane = threadIdx.x % WAVE;
    for (int64_t s = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE; s < S; s += (int64_t)gridDim.x * WAVES) {
        const Session r = inspect(offsets, pcum, keep, s, M, Q, h);
        if (r.bad) {                                                    // (reported here for both forms: this one sees every session)
            if (lane == 0) atomicOr(status, r.bad);
            continue;
        }
        if (r.cnt == 0 || r.L > WAVE) continue;
        const bool valid = lane < r.L;
        const int32_t poi = valid ? seq[3 * ((int64_t)r.a + lane)] : 0;
        const int occ = chunk_occ(poi, lane, r.L);
        int sum = valid && occ == 1, most = valid ? occ : 0;
        scan(sum, most, lane);
        const int64_t c = lane + 1;                                     // lane j closes the history r_0 .. r_j of sample j + 1
        if (valid && c >= h) store(r.p0 + (c - h), s, c, sum, most, session, cut, nn, mult);
    }
}

// The long form, one wave per workgroup.  The wave looks through 64 sessions at a time, a lane each, and takes those with more than
// 64 history rows one after the other.  The POI column of a session is staged in LDS; in chunk k a lane counts its POI among the
// 64 k rows before the chunk (16-byte reads, every lane the same address: a broadcast) and among the chunk's own rows by shuffle.
// Per session of L rows that is about L^2 / 512 LDS reads per wave and L^2 / 128 compares per lane.
__global__ __launch_bounds__(WAVE) void long_kernel(const int32_t* __restrict__ seq, const int64_t* __restrict__ offsets,
                                                    const int64_t* __restrict__ pcum, const uint8_t* __restrict__ keep, int64_t S, int64_t M,
                                                    int64_t Q, int64_t h, int32_t* __restrict__ session, int32_t* __restrict__ cut,
                                                    int32_t* __restrict__ nn, int32_t* __restrict__ mult) {
    __shared__ __attribute__((aligned(16))) int32_t col[MAX_L];
    const int lane = threadIdx.x;
    for (int64_t s0 = (int64_t)blockIdx.x * WAVE; s0 < S; s0 += (int64_t)gridDim.x * WAVE) {
        Session r = {0, 0, 0, 0, 0};
        if (s0 + lane < S) r = inspect(offsets, pcum, keep, s0 + lane, M, Q, h);
        unsigned long long todo = __ballot(!r.bad && r.cnt > 0 && r.L > WAVE);
        while (todo) {                                                  // (wave-uniform)
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1;
            const int a = __shfl(r.a, k, WAVE), L = __shfl(r.L, k, WAVE), p0 = __shfl(r.p0, k, WAVE);
            __syncthreads();                                            // the session before has been read
            for (int j = lane; j < L; j += WAVE) col[j] = seq[3 * ((int64_t)a + j)];          // (L <= MAX_L: inspect)
            __syncthreads();
            int carry_n = 0, carry_m = 0;
            for (int base = 0; base < L; base += WAVE) {
                const int j = base + lane;
                const bool valid = j < L;
                const int32_t poi = valid ? col[j] : 0;
                int occ = 0;
                for (int i = 0; i < base; i += 4) {                     // rows before the chunk: all of them before row j
                    const int4 v = *reinterpret_cast<const int4*>(&col[i]);
                    occ += (v.x == poi) + (v.y == poi) + (v.z == poi) + (v.w == poi);
                }
                occ += chunk_occ(poi, lane, L - base < WAVE ? L - base : WAVE);
                int sum = valid && occ == 1, most = valid ? occ : 0;
                scan(sum, most, lane);
                sum += carry_n;
                most = most > carry_m ? most : carry_m;
                const int64_t c = j + 1;
                if (valid && c >= h) store(p0 + (c - h), s0 + k, c, sum, most, session, cut, nn, mult);
                carry_n = __shfl(sum, WAVE - 1, WAVE);                  // (lanes beyond the last row add nothing: the last row's)
                carry_m = __shfl(most, WAVE - 1, WAVE);
            }
        }
    }
}

// null only where the buffer has no element
bool bad_ptr(const void* p, uintptr_t align, int64_t n) {
    return (p == nullptr && n > 0) || (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0;
}

unsigned grid(int64_t work, int64_t per_block, int64_t most) {
    const int64_t b = (work + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b < most ? b : most);
}

}  // namespace

#define LAUNCH(kernel, grid, block, ...)                                                            \
    do {                                                                                            \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);   \
        const hipError_t err_ = hipGetLastError();                                                  \
        if (err_ != hipSuccess) return (int)err_;                                                   \
    } while (0)

extern "C" int mobgt_prefixes_abi_version(void) { return MOBGT_PREFIXES_ABI_VERSION; }

extern "C" int mobgt_prefixes_stats(const void* seq, const void* offsets, const void* pcum, const void* keep, int64_t S, int64_t M,
                                    int64_t Q, int64_t min_history, void* session, void* cut, void* n, void* mult, void* status,
                                    void* stream) {
    if (S < 0 || S > INT32_MAX || M < 0 || M > INT32_MAX || Q < 0 || Q > M || min_history < 1) return MOBGT_PREFIXES_EBADDIM;
    if (bad_ptr(seq, 4, M) || bad_ptr(offsets, 8, S + 1) || bad_ptr(pcum, 8, S + 1) || bad_ptr(session, 4, Q) || bad_ptr(cut, 4, Q) ||
        bad_ptr(n, 4, Q) || bad_ptr(mult, 4, Q) || bad_ptr(status, 4, 1))
        return MOBGT_PREFIXES_EALIGN;
    LAUNCH(fill_kernel, grid(Q, TPB, FILL_BLOCKS), TPB, Q, (int32_t*)session, (int32_t*)cut, (int32_t*)n, (int32_t*)mult, (int32_t*)status);
    if (S > 0) {
        LAUNCH(short_kernel, grid(S, WAVES, SHORT_BLOCKS), TPB, (const int32_t*)seq, (const int64_t*)offsets, (const int64_t*)pcum,
               (const uint8_t*)keep, S, M, Q, min_history, (int32_t*)session, (int32_t*)cut, (int32_t*)n, (int32_t*)mult, (int32_t*)status);
        LAUNCH(long_kernel, grid(S, WAVE, LONG_BLOCKS), WAVE, (const int32_t*)seq, (const int64_t*)offsets, (const int64_t*)pcum,
               (const uint8_t*)keep, S, M, Q, min_history, (int32_t*)session, (int32_t*)cut, (int32_t*)n, (int32_t*)mult);
    }
    return 0;
}
