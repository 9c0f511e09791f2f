// include/mobgt_geo.h: the within-radius POI graph from coordinates (graphormer/foursquare_process.py:15-23, :689-702).
//
// One kernel body, three outputs (bit words + degrees, degrees only, CSR fill):
//
//   * a workgroup of 4 waves owns 16 consecutive rows, 4 per wave; a row's unit vector lives in registers;
//   * the columns' unit vectors pass through LDS in tiles of MOBGT_GEO_TILE = 2048 columns (48 KB, a straight coalesced copy
//     of the [P, 3] array: lane l of a wave reads column 64 b + l at step b, a 24-byte stride over ds_read_b64 -- 32 lanes
//     on 64 distinct banks);
//   * per step and row one __ballot of the membership test: 64 columns as a 64-bit mask, uniform in the wave.  Words: lanes
//     2 b and 2 b + 1 keep its halves, so after the tile's 32 steps lane l holds word l of the tile and the wave stores 256
//     contiguous bytes per row.  Degrees: popcounts of the masks.  Fill: a set lane stores its column at the row's running
//     base + the popcount of the mask below it, so columns come out ascending without a sort.
//
// The test is f64 and exactly symmetric (see the header); every wave of a workgroup runs every tile (the tile barrier), rows
// at and beyond P compute on row P - 1 and store nothing.  No workgroup reads what another writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_geo.h"

namespace {

constexpr int WAVES = 4;                           // waves per workgroup
constexpr int RPW = 4;                             // rows per wave
constexpr int TPB = WAVES * 64;
constexpr int ROWS = WAVES * RPW;                  // rows per workgroup
constexpr int TILE = MOBGT_GEO_TILE;               // columns per LDS tile = 64 lanes x 32 bits
static_assert(TILE == 64 * 32, "a lane keeps one 32-bit word per tile");

enum Mode { WORDS, COUNT, FILL };

__global__ __launch_bounds__(256) void unit_kernel(const double* __restrict__ coords, double* __restrict__ unit, int64_t P) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    constexpr double kPi = 3.141592653589793;      // math.pi
    const double lat = coords[2 * i] * kPi / 180.0, lon = coords[2 * i + 1] * kPi / 180.0;    // foursquare_process.py:17-20
    double sl, cl, so, co;
    sincos(lat, &sl, &cl);
    sincos(lon, &so, &co);
    unit[3 * i] = cl * co;
    unit[3 * i + 1] = cl * so;
    unit[3 * i + 2] = sl;
}

template <int MODE>
__global__ __launch_bounds__(TPB) void radius_kernel(const double* __restrict__ unit, int64_t P, double chord2_max,
                                                     int* __restrict__ words, int64_t W, int* __restrict__ deg,
                                                     const int64_t* __restrict__ rowptr, int* __restrict__ col,
                                                     float* __restrict__ val) {
    __shared__ double s_u[TILE * 3];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS + wave * RPW;

    int64_t row[RPW];
    double xi[RPW], yi[RPW], zi[RPW];
    int cnt[RPW];                                  // set bits so far, the diagonal included (uniform in the wave)
    int64_t base[RPW], end[RPW];                   // FILL: where the row's next column goes, and where the row ends
    float inv[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        row[r] = row0 + r;
        const int64_t ld = row[r] < P ? row[r] : P - 1;
        xi[r] = unit[3 * ld]; yi[r] = unit[3 * ld + 1]; zi[r] = unit[3 * ld + 2];
        cnt[r] = 0;
        base[r] = end[r] = 0;
        inv[r] = 0.0f;
        if (MODE == FILL && row[r] < P) {
            base[r] = rowptr[row[r]];
            end[r] = rowptr[row[r] + 1];
            inv[r] = (float)(1.0 / (double)(end[r] - base[r]));
        }
    }

    for (int64_t c0 = 0; c0 < P; c0 += TILE) {
        const int64_t n_tile = (P - c0 < TILE ? P - c0 : TILE) * 3;     // doubles of this tile
        __syncthreads();                                                // (the previous tile has been read)
        for (int64_t q = t; q < n_tile; q += TPB) s_u[q] = unit[c0 * 3 + q];
        __syncthreads();

        int word[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) word[r] = 0;
        for (int b = 0; b < 32; ++b) {
            if (c0 + 64 * b >= P) break;                                // (uniform)
            const int64_t j = c0 + 64 * b + lane;
            const bool in = j < P;
            const int jl = in ? 64 * b + lane : 0;                      // (never read LDS words the tile did not fill)
            const double xj = s_u[3 * jl], yj = s_u[3 * jl + 1], zj = s_u[3 * jl + 2];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const double dx = xi[r] - xj, dy = yi[r] - yj, dz = zi[r] - zj;
                const double c2 = dx * dx + dy * dy + dz * dz;
                const bool bit = in && ((c2 > 0.0 && c2 <= chord2_max) || j == row[r]);
                const unsigned long long m = __ballot(bit);
                cnt[r] += __popcll(m);
                if (MODE == WORDS) {
                    if ((lane >> 1) == b) word[r] = (int)(unsigned)((lane & 1) ? (m >> 32) : (m & 0xffffffffull));
                }
                if (MODE == FILL) {
                    if (m != 0 && row[r] < P) {
                        const int64_t pos = base[r] + __popcll(m & ((1ull << lane) - 1ull));
                        if (bit && pos < end[r]) {
                            col[pos] = (int)j;
                            val[pos] = inv[r];
                        }
                        base[r] += __popcll(m);
                    }
                }
            }
        }
        if (MODE == WORDS) {
            const int64_t w = c0 / 32 + lane;                           // this lane's word of the row
#pragma unroll
            for (int r = 0; r < RPW; ++r)
                if (row[r] < P && w < W) words[row[r] * W + w] = word[r];
        }
    }
    if (MODE != FILL && lane == 0) {
#pragma unroll
        for (int r = 0; r < RPW; ++r)
            if (row[r] < P) deg[row[r]] = cnt[r] - 1;                   // (the diagonal bit is set exactly once)
    }
}

bool bad_ptr(const void* p, uintptr_t align) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0; }
bool bad_p(int64_t P) { return P < 1 || P > MOBGT_GEO_MAX_P; }
unsigned grid_rows(int64_t P) { return (unsigned)((P + ROWS - 1) / ROWS); }

}  // namespace

extern "C" int mobgt_geo_abi_version(void) { return MOBGT_GEO_ABI_VERSION; }

extern "C" int mobgt_geo_unit_vectors(const void* coords_deg, void* unit, int64_t P, void* stream) {
    if (bad_p(P)) return MOBGT_GEO_EBADDIM;
    if (bad_ptr(coords_deg, 8) || bad_ptr(unit, 8)) return MOBGT_GEO_EALIGN;
    hipLaunchKernelGGL(unit_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)coords_deg,
                       (double*)unit, P);
    return (int)hipGetLastError();
}

extern "C" int mobgt_geo_radius_words(const void* unit, int64_t P, double chord2_max, void* words, void* deg, void* stream) {
    if (bad_p(P)) return MOBGT_GEO_EBADDIM;
    if (bad_ptr(unit, 8) || bad_ptr(words, 4) || bad_ptr(deg, 4)) return MOBGT_GEO_EALIGN;
    const int64_t W = (P + 127) / 128 * 4;
    hipLaunchKernelGGL(radius_kernel<WORDS>, dim3(grid_rows(P)), dim3(TPB), 0, (hipStream_t)stream, (const double*)unit, P, chord2_max,
                       (int*)words, W, (int*)deg, (const int64_t*)nullptr, (int*)nullptr, (float*)nullptr);
    return (int)hipGetLastError();
}

extern "C" int mobgt_geo_radius_count(const void* unit, int64_t P, double chord2_max, void* deg, void* stream) {
    if (bad_p(P)) return MOBGT_GEO_EBADDIM;
    if (bad_ptr(unit, 8) || bad_ptr(deg, 4)) return MOBGT_GEO_EALIGN;
    hipLaunchKernelGGL(radius_kernel<COUNT>, dim3(grid_rows(P)), dim3(TPB), 0, (hipStream_t)stream, (const double*)unit, P, chord2_max,
                       (int*)nullptr, (int64_t)0, (int*)deg, (const int64_t*)nullptr, (int*)nullptr, (float*)nullptr);
    return (int)hipGetLastError();
}

extern "C" int mobgt_geo_radius_fill(const void* unit, int64_t P, double chord2_max, const void* rowptr, void* col, void* val,
                                     void* stream) {
    if (bad_p(P)) return MOBGT_GEO_EBADDIM;
    if (bad_ptr(unit, 8) || bad_ptr(rowptr, 8) || bad_ptr(col, 4) || bad_ptr(val, 4)) return MOBGT_GEO_EALIGN;
    hipLaunchKernelGGL(radius_kernel<FILL>, dim3(grid_rows(P)), dim3(TPB), 0, (hipStream_t)stream, (const double*)unit, P, chord2_max,
                       (int*)nullptr, (int64_t)0, (int*)nullptr, (const int64_t*)rowptr, (int*)col, (float*)val);
    return (int)hipGetLastError();
}
