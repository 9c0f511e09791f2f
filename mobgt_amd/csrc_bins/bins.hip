// include/mobgt_bins.h: the distance-bin edges and table from coordinates (graphormer/collator.py:301-308, :429-437).
//
// digits_kernel -- one level of the radix select over the squared chords of all pairs, nothing of size P^2 stored:
//
//   * radius.hip's walk: a workgroup of 4 waves owns 16 consecutive rows, 4 per wave, a row's unit vector in registers; the
//     columns' unit vectors pass through LDS in tiles of MOBGT_BINS_TILE columns, lane l of a wave takes column 64 b + l;
//   * c2 is exactly symmetric, so only the pairs i < j are walked (tiles left of the workgroup's rows and steps left of the
//     wave's rows are skipped) and counted twice; the P diagonal zeros are added by workgroup 0;
//   * in a city nearly all pairs share the sign, the exponent and the first mantissa bits, so in the first levels a whole wave
//     lands in a handful of buckets: the lanes that hold the digit of the first remaining lane add once, with the popcount of
//     their ballot, up to PEEL times; what is left after that is spread out and goes to LDS one atomic per lane.  Each wave
//     has a histogram of its own in LDS; a workgroup's 16 x P pairs fit its 32-bit counts;
//   * one flush per workgroup: 64-bit vector atomics to global memory for the buckets that are not empty.
//
// table_kernel -- np.searchsorted(thresholds, c2, side="right") for every pair: a workgroup owns 8 table rows and keeps every
// `stride`-th threshold in LDS (at most COARSE of them: all of them up to 2048 thresholds); a pair searches those, then the
// stride - 1 thresholds between two of them in global memory (they stay in L2: 256 KB at most).  A lane owns four int16 that
// share an aligned 8-byte word of the table and stores them at once if the row holds all four, one by one at the row's head
// and tail.  chord2, the search and the store are bins_search.h's, shared with csrc_pairbins/batch.hip.
//
// Built with -ffp-contract=off (Makefile): c2 is the header's bit-exact expression.  No workgroup reads what another writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_bins.h"
#include "bins_search.h"

namespace {

constexpr int WAVES = 4;                           // waves per workgroup
constexpr int RPW = 4;                             // rows per wave (digits_kernel)
constexpr int TPB = WAVES * 64;
constexpr int ROWS = WAVES * RPW;                  // rows per workgroup (digits_kernel)
constexpr int TILE = MOBGT_BINS_TILE;              // columns per LDS tile
constexpr int RADIX = MOBGT_BINS_RADIX;
constexpr int PEEL = 4;                            // digits a wave adds with one lane each before the per-lane atomics
constexpr int TROWS = 8;                           // table rows per workgroup (table_kernel)
static_assert(RADIX == 1 << MOBGT_BINS_DIGIT_BITS && 64 % MOBGT_BINS_DIGIT_BITS == 0, "whole digits");
static_assert(TILE % 64 == 0 && RADIX == TPB, "a step is one wave wide; the flush takes one bucket per thread");
static_assert((uint64_t)ROWS * MOBGT_BINS_MAX_P < (1ull << 32), "a workgroup's pairs fit a 32-bit count");

__global__ __launch_bounds__(TPB) void digits_kernel(const double* __restrict__ unit, int64_t P, uint64_t prefix, int prefix_bits,
                                                     unsigned long long* __restrict__ counts) {
    __shared__ double s_u[TILE * 3];
    __shared__ unsigned s_hist[WAVES][RADIX];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS + wave * RPW;
    const int shift = 64 - prefix_bits - MOBGT_BINS_DIGIT_BITS;        // of the digit; the prefix lies above it

    for (int q = t; q < WAVES * RADIX; q += TPB) (&s_hist[0][0])[q] = 0u;
    int64_t row[RPW];
    double xi[RPW], yi[RPW], zi[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        row[r] = row0 + r;
        const int64_t ld = row[r] < P ? row[r] : P - 1;
        xi[r] = unit[3 * ld]; yi[r] = unit[3 * ld + 1]; zi[r] = unit[3 * ld + 2];
    }
    unsigned* hist = s_hist[wave];

    // (the first tile that holds a column right of the workgroup's first row)
    for (int64_t c0 = (int64_t)blockIdx.x * ROWS / TILE * TILE; c0 < P; c0 += TILE) {
        const int64_t n_tile = (P - c0 < TILE ? P - c0 : TILE) * 3;     // doubles of this tile
        __syncthreads();                                                // (the previous tile has been read; s_hist is clear)
        for (int64_t q = t; q < n_tile; q += TPB) s_u[q] = unit[c0 * 3 + q];
        __syncthreads();

        for (int b = 0; b < TILE / 64; ++b) {
            if (c0 + 64 * b >= P) break;                                // (uniform)
            if (c0 + 64 * b + 63 <= row0) continue;                     // (uniform in the wave: no column right of any of its rows)
            const int64_t j = c0 + 64 * b + lane;
            const bool in = j < P;
            const int jl = in ? 64 * b + lane : 0;                      // (never read LDS words the tile did not fill)
            const double xj = s_u[3 * jl], yj = s_u[3 * jl + 1], zj = s_u[3 * jl + 2];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const uint64_t key = (uint64_t)__double_as_longlong(chord2(xi[r], yi[r], zi[r], xj, yj, zj));
                const uint64_t head = (key >> 1) >> (shift + MOBGT_BINS_DIGIT_BITS - 1);     // (a shift by 64 when prefix_bits = 0)
                const int digit = (int)((key >> shift) & (RADIX - 1));
                const bool mine = in && j > row[r] && row[r] < P && head == prefix;
                unsigned long long rem = __ballot(mine);
                for (int it = 0; it < PEEL && rem != 0ull; ++it) {      // (uniform in the wave)
                    const int leader = __ffsll((long long)rem) - 1;
                    const int d0 = __builtin_amdgcn_readlane(digit, leader);
                    const unsigned long long m = __ballot(mine && digit == d0) & rem;
                    if (lane == leader) atomicAdd(&hist[d0], (unsigned)__popcll(m));
                    rem &= ~m;
                }
                if ((rem >> lane) & 1ull) atomicAdd(&hist[digit], 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long sum = 0ull;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) sum += s_hist[w][t];
    sum *= 2ull;                                                        // (i, j) and (j, i)
    if (blockIdx.x == 0 && t == 0 && prefix == 0ull) sum += (unsigned long long)P;          // c2(i, i) = +0.0: pattern 0
    if (sum != 0ull) atomicAdd(&counts[t], sum);
}

__global__ __launch_bounds__(TPB) void table_kernel(const double* __restrict__ unit, int64_t P, const double* __restrict__ thr, int nthr,
                                                    int stride, int ncoarse, int16_t* __restrict__ table) {
    __shared__ double s_c[COARSE];
    const int t = threadIdx.x;
    for (int q = t; q < ncoarse; q += TPB) s_c[q] = thr[(int64_t)q * stride];
    __syncthreads();

    auto count = [&](double c2) -> int { return count_thresholds(s_c, ncoarse, thr, nthr, stride, c2); };
    const int16_t pad = (int16_t)count(0.0);

    const int64_t ld = P + 1;
    const int64_t skew = (int64_t)((reinterpret_cast<uintptr_t>(table) & 7u) >> 1);         // elements from an 8-byte boundary to table[0]
    for (int ar = 0; ar < TROWS; ++ar) {
        const int64_t a = (int64_t)blockIdx.x * TROWS + ar;
        if (a >= ld) break;                                             // (uniform)
        const int64_t f0 = a * ld + skew, f1 = f0 + P;                  // the row's first and last element, counted from the boundary
        double xa = 0.0, ya = 0.0, za = 0.0;
        if (a > 0) { xa = unit[3 * (a - 1)]; ya = unit[3 * (a - 1) + 1]; za = unit[3 * (a - 1) + 2]; }
        for (int64_t g = f0 / VEC + t; g <= f1 / VEC; g += TPB) {
            int16_t v[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int64_t e = g * VEC + k, col = e - f0;
                v[k] = pad;
                if (a > 0 && col >= 1 && col <= P)
                    v[k] = (int16_t)count(chord2(xa, ya, za, unit[3 * (col - 1)], unit[3 * (col - 1) + 1], unit[3 * (col - 1) + 2]));
            }
            store_vec(table + (g * VEC - skew), v, g * VEC, f0, f1);                 // (the word's address: 8-byte aligned)
        }
    }
}

bool bad_ptr(const void* p, uintptr_t align) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0; }
bool bad_p(int64_t P) { return P < 1 || P > MOBGT_BINS_MAX_P; }

}  // namespace

extern "C" int mobgt_bins_abi_version(void) { return MOBGT_BINS_ABI_VERSION; }

extern "C" int mobgt_bins_chord2_digits(const void* unit, int64_t P, uint64_t prefix, int prefix_bits, void* counts, void* stream) {
    if (bad_p(P)) return MOBGT_BINS_EBADDIM;
    if (prefix_bits < 0 || prefix_bits > 64 - MOBGT_BINS_DIGIT_BITS || prefix_bits % MOBGT_BINS_DIGIT_BITS != 0) return MOBGT_BINS_EBADDIM;
    if ((prefix_bits == 0 && prefix != 0) || (prefix_bits > 0 && (prefix >> prefix_bits) != 0)) return MOBGT_BINS_EBADDIM;
    if (bad_ptr(unit, 8) || bad_ptr(counts, 8)) return MOBGT_BINS_EALIGN;
    const hipError_t rc = hipMemsetAsync(counts, 0, RADIX * sizeof(unsigned long long), (hipStream_t)stream);
    if (rc != hipSuccess) return (int)rc;
    hipLaunchKernelGGL(digits_kernel, dim3((unsigned)((P + ROWS - 1) / ROWS)), dim3(TPB), 0, (hipStream_t)stream, (const double*)unit, P,
                       prefix, prefix_bits, (unsigned long long*)counts);
    return (int)hipGetLastError();
}

extern "C" int mobgt_bins_table(const void* unit, int64_t P, const void* thresholds, int nthr, void* table, void* stream) {
    if (bad_p(P) || nthr < MOBGT_BINS_MIN_THRESHOLDS || nthr > MOBGT_BINS_MAX_THRESHOLDS) return MOBGT_BINS_EBADDIM;
    if (bad_ptr(unit, 8) || bad_ptr(thresholds, 8) || bad_ptr(table, 2)) return MOBGT_BINS_EALIGN;
    const int stride = (nthr + COARSE - 1) / COARSE, ncoarse = (nthr + stride - 1) / stride;
    hipLaunchKernelGGL(table_kernel, dim3((unsigned)((P + 1 + TROWS - 1) / TROWS)), dim3(TPB), 0, (hipStream_t)stream, (const double*)unit, P,
                       (const double*)thresholds, nthr, stride, ncoarse, (int16_t*)table);
    return (int)hipGetLastError();
}
