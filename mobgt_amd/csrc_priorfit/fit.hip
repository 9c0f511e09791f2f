// include/mobgt_priorfit.h: the per-batch terms of a maximum-likelihood fit of the priors' weights -- n, nll, gradient and Hessian
// of the log-likelihood of the targets under softmax(base + sum_k W[l, k] feats[k]), for L weight rows at once.  The rule is the
// docstring of mobgt_amd/priorfit.py; the header repeats it in short.
//
// partials_kernel<K> -- ONE WORKGROUP PER (CHUNK OF COLUMNS, ROW).  Thread t owns the COLS consecutive columns c0 + COLS t ..: it
// loads them of base and of the K planes once, as f32 in registers (one 16-byte load each where the address allows it, guarded
// scalar loads at a row's end and on rows that are not 16-byte aligned; the columns a thread owns do not depend on which).
// First pass, every l: z of its columns, their maximum reduced over the wave, into LDS; one barrier.  Second pass, l by l: the
// chunk's maximum m from LDS, e = exp(z - m) (0 for a masked column: -inf never meets -inf in a subtraction), the 1 + K +
// K (K + 1) / 2 sums Z, A_k, B_kj in registers, a butterfly over the wave, the four waves' sums through LDS (two buffers, so one
// barrier per l), added in wave order and stored.  z is evaluated twice from the same expression; the library is built with
// -ffp-contract=off, so both evaluations -- and terms_host's -- round alike, and the sums name their FMAs themselves.
//
// combine_kernel -- ONE WAVE PER (l, g), lane j the j-th sum.  It ORs the flags of every l' of the row (a row counts for all
// weight rows or for none), takes the maximum M of the chunks' m, adds the records in chunk order scaled by exp(m_c - M),
// skipping a chunk whose m is -inf, reads the target column and writes the NT terms -- zeros for a row that does not count.
//
// No workgroup reads what another of the same launch writes; the only atomic is the OR into the status word.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mobgt_priorfit.h"

namespace {

constexpr int WAVE = MOBGT_PRIORFIT_WAVE;
constexpr int TPB = MOBGT_PRIORFIT_THREADS;
constexpr int WAVES = TPB / WAVE;
constexpr int CHUNK = MOBGT_PRIORFIT_CHUNK;
constexpr int COLS = MOBGT_PRIORFIT_COLS;
constexpr int MAX_K = MOBGT_PRIORFIT_MAX_K;
constexpr int MAX_L = MOBGT_PRIORFIT_MAX_L;
constexpr int sums_of(int K) { return 1 + K + K * (K + 1) / 2; }       // Z, A_k, B_kj
static_assert(TPB % WAVE == 0 && CHUNK == TPB * COLS && COLS == 4, "a thread's columns are one 16-byte load");
static_assert(sums_of(MAX_K) + 1 == MOBGT_PRIORFIT_MAX_NT && sums_of(MAX_K) <= WAVE, "a lane per sum in the combine");
static_assert(sums_of(MAX_K) + 2 <= TPB, "a thread per double of a record");

struct Args {
    const float* base;                   // may be null
    const float* feats;
    int64_t ld_base, ld_feats, plane_feats, G, V, ld_y, target_offset;
    const void* y;
    int y64, K, L;
    const double* W;
    double* work;
    int64_t nchunks;
};

__device__ inline double wave_max(double v) {
#pragma unroll
    for (int d = WAVE / 2; d; d /= 2) v = fmax(v, __shfl_xor(v, d, WAVE));
    return v;
}

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int d = WAVE / 2; d; d /= 2) v += __shfl_xor(v, d, WAVE);
    return v;
}

__device__ inline bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// out[j] = row[c + j] for the columns below V, `fill` for the others; nothing from V on is read
__device__ inline void load_cols(const float* __restrict__ row, int64_t c, int64_t V, float fill, float (&out)[COLS]) {
    if (c + COLS <= V && (reinterpret_cast<uintptr_t>(row + c) & 15u) == 0) {
        const float4 v = *reinterpret_cast<const float4*>(row + c);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < COLS; ++j) out[j] = c + j < V ? row[c + j] : fill;
    }
}

template <int K>
__global__ __launch_bounds__(TPB) void partials_kernel(Args a) {
    constexpr int NS = sums_of(K), REC = NS + 2;
    __shared__ double s_max[MAX_L][WAVES];
    __shared__ int s_bad[MAX_L][WAVES];
    __shared__ double s_part[2][WAVES][NS];
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const int64_t g = blockIdx.y, chunk = blockIdx.x;
    const int64_t c = chunk * CHUNK + (int64_t)tid * COLS;
    const int L = a.L;
    const double NEG = -INFINITY;

    float b[COLS], f[K][COLS];
    if (a.base != nullptr) load_cols(a.base + g * a.ld_base, c, a.V, -INFINITY, b);
    else {
#pragma unroll
        for (int j = 0; j < COLS; ++j) b[j] = 0.0f;
    }
    bool bad_f = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        load_cols(a.feats + k * a.plane_feats + g * a.ld_feats, c, a.V, 0.0f, f[k]);
#pragma unroll
        for (int j = 0; j < COLS; ++j) bad_f = bad_f || !finite32(f[k][j]);
    }
    bool in[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) in[j] = c + j < a.V;

    // z of column j under weight row l: the rule's order, no FMA (-ffp-contract=off); a column from V on is masked
    auto z_of = [&](const double (&w)[K], int j) {
        double z = (double)b[j];
#pragma unroll
        for (int k = 0; k < K; ++k) z = z + w[k] * (double)f[k][j];
        return in[j] ? z : NEG;
    };

    for (int l = 0; l < L; ++l) {
        double w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = a.W[l * K + k];
        double m = NEG;
        bool bad = bad_f;
#pragma unroll
        for (int j = 0; j < COLS; ++j) {
            const double z = z_of(w, j);
            bad = bad || z != z || z == INFINITY;
            m = fmax(m, z);
        }
        m = wave_max(m);
        const int any_bad = __any(bad);
        if (lane == 0) {
            s_max[l][wave] = m;
            s_bad[l][wave] = any_bad;
        }
    }
    __syncthreads();

    for (int l = 0; l < L; ++l) {
        double w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = a.W[l * K + k];
        double m = s_max[l][0];
        int flag = s_bad[l][0];
#pragma unroll
        for (int v = 1; v < WAVES; ++v) {
            m = fmax(m, s_max[l][v]);
            flag |= s_bad[l][v];
        }
        double acc[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) acc[i] = 0.0;
#pragma unroll
        for (int j = 0; j < COLS; ++j) {
            const double z = z_of(w, j);
            const double e = z == NEG ? 0.0 : exp(z - m);               // (m = -inf only where every z is)
            acc[0] += e;
            int p = 1 + K;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double fk = (double)f[k][j], ef = e * fk;
                acc[1 + k] += ef;
#pragma unroll
                for (int q = k; q < K; ++q, ++p) acc[p] = fma(ef, (double)f[q][j], acc[p]);
            }
        }
        double* part = s_part[l & 1][wave];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const double s = wave_sum(acc[i]);
            if (lane == 0) part[i] = s;
        }
        __syncthreads();
        double* rec = a.work + ((g * L + l) * a.nchunks + chunk) * REC;
        if (tid < NS) {
            const double (*sp)[NS] = s_part[l & 1];
            double s = sp[0][tid];
#pragma unroll
            for (int v = 1; v < WAVES; ++v) s += sp[v][tid];
            rec[2 + tid] = s;
        } else if (tid == NS) {
            rec[0] = flag ? 1.0 : 0.0;
        } else if (tid == NS + 1) {
            rec[1] = m;
        }
    }
}

__device__ inline int64_t load_y(const void* p, int wide, int64_t i) {
    return wide ? static_cast<const int64_t*>(p)[i] : static_cast<const int32_t*>(p)[i];
}

__global__ __launch_bounds__(TPB) void combine_kernel(Args a, double* __restrict__ terms, int32_t* __restrict__ status) {
    const int lane = threadIdx.x % WAVE;
    const int64_t wv = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
    if (wv >= a.G * a.L) return;                                        // (uniform in the wave; the kernel has no barrier)
    const int K = a.K, L = a.L;
    const int l = (int)(wv / a.G);
    const int64_t g = wv % a.G;
    const int NS = 1 + K + K * (K + 1) / 2, REC = NS + 2, NT = NS + 1;
    const int64_t nch = a.nchunks;
    const double* rows = a.work + g * L * nch * REC;
    const double NEG = -INFINITY;

    // the flags and the emptiness of every weight row of g; the maximum of this one
    bool bad = false;
    double M = NEG;
    for (int lp = 0; lp < L; ++lp) {
        bool some = false;
        for (int64_t c = lane; c < nch; c += WAVE) {
            const double* r = rows + (lp * nch + c) * REC;
            const double m = r[1];
            bad = bad || r[0] != 0.0;
            some = some || m > NEG;
            if (lp == l) M = fmax(M, m);
        }
        if (!__any(some)) bad = true;                                   // every z[lp, g, :] is -inf
    }
    M = wave_max(M);

    // the target column: z[lp, g, t] of every weight row must be finite
    const int64_t t = load_y(a.y, a.y64, g * a.ld_y) + a.target_offset;
    const bool in_range = t >= 0 && t < a.V;
    double zt = 0.0, ft_mine = 0.0;
    if (in_range) {
        double ft[MAX_K];
#pragma unroll
        for (int k = 0; k < MAX_K; ++k) ft[k] = k < K ? (double)a.feats[k * a.plane_feats + g * a.ld_feats + t] : 0.0;
        const double bt = a.base != nullptr ? (double)a.base[g * a.ld_base + t] : 0.0;
        for (int lp = 0; lp < L; ++lp) {
            double z = bt;
#pragma unroll
            for (int k = 0; k < MAX_K; ++k)
                if (k < K) z = z + a.W[lp * K + k] * ft[k];
            bad = bad || !(fabs(z) < INFINITY);
            if (lp == l) zt = z;
        }
        if (lane >= 1 && lane <= K) ft_mine = (double)a.feats[(int64_t)(lane - 1) * a.plane_feats + g * a.ld_feats + t];
    }
    bad = __any(bad);

    // lane j < NS: sum j of the records, in chunk order
    double acc = 0.0;
    if (lane < NS) {
        for (int64_t c = 0; c < nch; ++c) {
            const double* r = rows + (l * nch + c) * REC;
            const double m = r[1];
            if (m == NEG) continue;                                     // skipped, not rescaled: (-inf) - (-inf) is NaN
            acc = fma(r[2 + lane], exp(m - M), acc);
        }
    }
    // B_kj sits in lane 1 + K + p, p counting the pairs k <= j row-major
    int pk = 0, pj = 0;
    if (lane > K) {
        int p = lane - 1 - K;
        for (pk = 0; pk < K - 1 && p >= K - pk; ++pk) p -= K - pk;
        pj = pk + p;
        if (pj >= K) pk = pj = 0;                                       // (lanes from NS on: any lane that exists)
    }
    const double Z = __shfl(acc, 0, WAVE);
    const double Ak = __shfl(acc, 1 + pk, WAVE), Aj = __shfl(acc, 1 + pj, WAVE);
    const bool counts = in_range && !bad;
    double* out = terms + (l * a.G + g) * NT;
    if (lane == 0) {
        out[0] = counts ? 1.0 : 0.0;
        out[1] = counts ? (M + log(Z)) - zt : 0.0;
        if (bad) atomicOr(status, MOBGT_PRIORFIT_SNONFINITE);
    } else if (lane <= K) {
        out[lane + 1] = counts ? acc / Z - ft_mine : 0.0;
    } else if (lane < NS) {
        out[lane + 1] = counts ? acc / Z - (Ak / Z) * (Aj / Z) : 0.0;
    }
}

// null only where the buffer has no element
bool bad_ptr(const void* p, uintptr_t align, int64_t n) {
    return (p == nullptr && n > 0) || (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0;
}

bool bad_sizes(int K, int64_t G, int64_t V, int L) {
    return K < 1 || K > MAX_K || L < 1 || L > MAX_L || G < 0 || G > MOBGT_PRIORFIT_MAX_G || V < 0 || V > INT32_MAX;
}

int64_t chunks_of(int64_t V) { return (V + CHUNK - 1) / CHUNK; }

template <int K>
void launch_partials(const Args& a, hipStream_t stream) {
    hipLaunchKernelGGL(partials_kernel<K>, dim3((unsigned)a.nchunks, (unsigned)a.G), dim3(TPB), 0, stream, a);
}

}  // namespace

extern "C" int mobgt_priorfit_abi_version(void) { return MOBGT_PRIORFIT_ABI_VERSION; }

extern "C" int mobgt_priorfit_nt(int K) { return K < 1 || K > MAX_K ? MOBGT_PRIORFIT_EBADDIM : sums_of(K) + 1; }

extern "C" int64_t mobgt_priorfit_work_bytes(int K, int64_t G, int64_t V, int L) {
    if (bad_sizes(K, G, V, L)) return MOBGT_PRIORFIT_EBADDIM;
    return G * L * chunks_of(V) * (sums_of(K) + 2) * (int64_t)sizeof(double);
}

extern "C" int mobgt_priorfit_terms(const float* base, int64_t ld_base, const float* feats, int64_t ld_feats, int64_t plane_feats, int K,
                                    int64_t G, int64_t V, const void* y, int y_dtype, int64_t ld_y, int64_t target_offset,
                                    const double* W, int L, void* work, double* terms, void* status, void* stream) {
    if (bad_sizes(K, G, V, L) || ld_feats < V || plane_feats < V || (base != nullptr && ld_base < V) || ld_y < 1)
        return MOBGT_PRIORFIT_EBADDIM;
    if (y_dtype != MOBGT_PRIORFIT_I32 && y_dtype != MOBGT_PRIORFIT_I64) return MOBGT_PRIORFIT_EDTYPE;
    const int64_t nchunks = chunks_of(V), NT = sums_of(K) + 1;
    if (bad_ptr(base, 4, 0) || bad_ptr(feats, 4, G * V) || bad_ptr(y, y_dtype == MOBGT_PRIORFIT_I64 ? 8 : 4, G) || bad_ptr(W, 8, 1) ||
        bad_ptr(work, 8, G * V) || bad_ptr(terms, 8, G * L * NT) || bad_ptr(status, 4, 1))
        return MOBGT_PRIORFIT_EALIGN;
    if (G == 0 || V == 0) return 0;
    const Args a = {base, feats, ld_base, ld_feats, plane_feats, G, V, ld_y, target_offset, y, y_dtype == MOBGT_PRIORFIT_I64, K, L, W,
                    static_cast<double*>(work), nchunks};
    const hipStream_t s = (hipStream_t)stream;
    switch (K) {
        case 1: launch_partials<1>(a, s); break;
        case 2: launch_partials<2>(a, s); break;
        case 3: launch_partials<3>(a, s); break;
        case 4: launch_partials<4>(a, s); break;
        case 5: launch_partials<5>(a, s); break;
        case 6: launch_partials<6>(a, s); break;
        case 7: launch_partials<7>(a, s); break;
        default: launch_partials<8>(a, s); break;
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((G * L + WAVES - 1) / WAVES)), dim3(TPB), 0, s, a, terms, (int32_t*)status);
    err = hipGetLastError();
    return err != hipSuccess ? (int)err : 0;
}
