// Backward of the encoder input from d(tokens) down to the gathered rows, one launch (model_fqandtoyo.py:1264-1298, 1338-1347;
// FuseEmbeddings :444-456):
//
//     d        = input_dropout'( pos_dropout'( d(out)[g, 1 + n, :] ) )          mobgt_assemble_tokens_bwd
//     d_add    = d;    d_nf = d * real[g, n]
//     g4       = d_nf * LeakyReLU'(nf)                                           FuseEmbeddings-4's activation (from its OUTPUT nf)
//     dx4      = g4 W4                    [.., :W2] = d(f2), [.., W2:] = d(category rows)
//     g2       = dx4[:, :W2] * LeakyReLU'(f2)
//     d_pt     = g2 W2                                                           FuseEmbeddings-2
//     d_token += column sums of the graph-token rows' d
//
// As launches these were assemble_tokens<true> (5 us), two small f32 GEMMs with a masked operand (10 + 9 us): three ramps and
// two round trips through global memory for 20 MFLOP on a few hundred rows.  Here a workgroup of 12 waves owns 16 node rows and
// walks the chain with its rows in LDS.  Products: full-f32 v_mfma_f32_16x16x4_f32, the weight ([out, in] row-major = the
// [K, N] operand of dX = g W) read as 16-byte runs ALONG a row -- 4 adjacent columns serve 4 MFMAs whose output column for lane j
// is n0 + 4 j + n -- so a wave instruction touches 4 rows x 256 contiguous bytes; 64-column blocks x K quarters over the 12
// waves, the quarters meet in an LDS tile (ds_add_f32).  d_nf and dx4 are written out because the two weight gradients
// (g4^T x4, g2^T pt -- leaves of the step's grouped weight-gradient launch) load them with the same activation masks.
//
// This header holds both kernels and their host-side parameter fill; csrc/tokbwd.hip (libmobgt_hip: mobgt_token_bwd_chain) and
// csrc_tokhost/tokhost.hip (libmobgt_tokhost: the hosting entry) each compile it.
//
// The hosting form (mobgt_tokhost_token_bwd_chain): the first encoder layer has no layer below it to finish its backward the way
// chain.hip's backward chain finishes the upper layers'; this launch is the next one on the device and leaves ~215 compute
// units idle.  So a row workgroup first FORMS its rows of d(out) = dx1 + dqkv Wqkv (bf16 MFMA on the packed Wqkv^T, written
// back in place: it is the encoder input's gradient), the graph-token rows likewise, 16 graphs per workgroup; and the layer's four
// weight gradients ride as extra workgroups (blockIdx >= n_chain), one 32 x 32 tile each.  No workgroup waits for another.
// Both are computed in the order of the launch they replace (mobgt_layer_backward_tail: K over eight waves, their partial sums
// added in wave order, then dx1), so every written result and weight gradient of the two forms agrees bit for bit; d_token, a sum
// over the graphs by atomics in the old form, is here the float64 sum of a workgroup's graphs rounded once.
#pragma once
#include "common.h"
#include "mobgt_hip.h"
#include "wgrad_body.h"

namespace mobgt_tokbwd {
namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int TNW = 12, TNT = TNW * 64, TBM = 16;
constexpr int TAIL_NW = 8;           // waves of the launch the hosting form replaces (wgrad.hip: wgrad_group_kernel<8>)
constexpr int HOST_MAX_WG = 4;       // weight-gradient problems a launch hosts (include/mobgt_tokhost.h: MOBGT_TOKHOST_MAX_WG)

struct TokBwdParams {
    const float* dout;                       // [G, N+1, C]
    const float* real;                       // [G*N]
    const float* y4;                         // nf = FuseEmbeddings-4's output [G*N, C]
    const float* y2; int64_t ld2;            // f2 = FuseEmbeddings-2's output [G*N, W2], row stride ld2 (the leading columns of x4)
    const float *w4, *w2;                    // [C, C], [W2, W2] row-major (out, in)
    float *d_nf, *d_add;                     // [G*N, C]
    float* dx4; int64_t ldx4;                // [G*N, C]
    float* d_pt;                             // [G*N, W2]
    float* d_token;                          // [C], accumulated
    int G, N;
    float slope4, slope2;
    uint32_t thr_pos, thr_in;
    float keep_pos, keep_in;
    uint64_t seed;
    const uint64_t* seed_dev;
    uint32_t salt_nf, salt_tok, salt_in;
    int n_node_blocks;
};

// what the first encoder layer left to this launch (the hosting form)
struct TokHost {
    const uint16_t *t_dqkv, *t_wqt;          // [G*T, 3C] bf16, Wqkv^T packed by mobgt_pack_mfma_b; both null: no tail
    float* dx1;                              // [G*T, C] f32 = dout: dx1 on entry, dx1 + dqkv Wqkv behind the launch
    mobgt_wgrad::WgradParams wg[HOST_MAX_WG];
    int wg_first[HOST_MAX_WG + 1], wg_tiles[HOST_MAX_WG], wg_splits[HOST_MAX_WG];
    int n_wg, n_chain;                       // weight-gradient problems; first passenger workgroup
};

__device__ __forceinline__ float leaky_grad(float y, float slope) { return y > 0.f ? 1.f : slope; }

#ifdef TB_STAMP
__device__ int* g_tb_dbg = nullptr;
#define TSTAMP_DECL int st_[8] = {}
#define TSTAMP(i) st_[i] = (int)wall_clock64()
#define TSTAMP_DUMP() do { if (g_tb_dbg && threadIdx.x == 0) for (int q_ = 0; q_ < 8; ++q_) g_tb_dbg[blockIdx.x * 8 + q_] = st_[q_]; } while (0)
#else
#define TSTAMP_DECL
#define TSTAMP(i)
#define TSTAMP_DUMP()
#endif

// out[ks] [TBM][N] (LDS partial tiles, one per K split ks < gemm_ks<N>(): the caller adds them up) = A [TBM][K] (LDS, row stride
// LDA) x rows [K range ks] of W [K][N] (global, row-major, row stride N).  Plain stores: ds_add_f32 into ONE tile measured 13 us
// per product (64 lanes on 8 banks, a read-modify-write each) against 3 us for the whole product without it.
template <int N> constexpr int gemm_ks() { return TNW / ((N + 63) / 64); }
template <int K, int N, int LDA, int LDO>
__device__ __forceinline__ void gemm_kn(const float* __restrict__ A, const float* __restrict__ W, float* __restrict__ out) {
    constexpr int NB = (N + 63) / 64, KS = TNW / NB, NT16 = K / 16, TMAX = (NT16 + KS - 1) / KS;
    static_assert(K % 16 == 0 && N % 32 == 0 && KS >= 1, "shape");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    if (wave >= NB * KS) return;
    const int blk = wave / KS, ks = wave % KS;
    const int t_lo = ks * NT16 / KS, t_hi = (ks + 1) * NT16 / KS;
    const int n0 = 64 * blk;
    const bool col_ok = n0 + 4 * j < N;                       // (the last block of a width that is not a multiple of 64)
    const int cl = col_ok ? n0 + 4 * j : 0;
    f32x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 bw[TMAX][4];
#pragma unroll
    for (int tt = 0; tt < TMAX; ++tt) {
        const int t = min(t_lo + tt, t_hi - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) bw[tt][i] = *reinterpret_cast<const f32x4*>(W + (int64_t)(16 * t + 4 * q + i) * N + cl);
    }
#pragma unroll
    for (int tt = 0; tt < TMAX; ++tt) {
        if (t_lo + tt < t_hi) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(A + j * LDA + 16 * (t_lo + tt) + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bw[tt][i][n], acc[n], 0, 0, 0);
        }
    }
    if (col_ok) {
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int v = 0; v < 4; ++v) out[(ks * TBM + 4 * q + v) * LDO + n0 + 4 * j + n] = acc[n][v];
    }
}

// The hosted tail for the workgroup's TBM token rows row_of(r): dst[r][:] (f32, LDS, row stride LDA) = dx1[row] + dqkv[row] Wqkv.
// Wave w owns the output columns 16 w .. 16 w + 15 and requests ALL of its share of the packed weight (K / 32 k-steps of one KB)
// before anything else -- call this first in the kernel; `tq` (LDS, TBM x (3C + 8) bf16) receives the rows of dqkv.  K is summed as
// mobgt_layer_backward_tail sums it (gemm_body.h, 8 waves): partial p_i = the k-steps i, i + 8, i + 16 in turn from zero, then
// ((p_0 + p_1) + ... + p_7) + dx1.
template <int C, int LDA, typename ROWOF>
__device__ __forceinline__ void host_tail(const TokHost& h, float* __restrict__ dst, uint16_t* __restrict__ tq, ROWOF&& row_of) {
    constexpr int K = 3 * C, S = K / 32, LDQ = K + 8;
    static_assert(C == 16 * TNW && K % 32 == 0, "one 16-column group per wave");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    uint4 b[S];
    const uint16_t* wp = h.t_wqt + ((int64_t)wave * S * 64 + lane) * 8;      // (packed: one contiguous KB per (group, k-step))
#pragma unroll
    for (int s = 0; s < S; ++s) b[s] = *reinterpret_cast<const uint4*>(wp + 512 * s);
    for (int e = threadIdx.x; e < TBM * (C / 4); e += TNT) {
        const int r = e / (C / 4), c = (e % (C / 4)) * 4;
        *reinterpret_cast<float4*>(dst + r * LDA + c) = *reinterpret_cast<const float4*>(h.dx1 + row_of(r) * C + c);
    }
    for (int e = threadIdx.x; e < TBM * (K / 8); e += TNT) {
        const int r = e / (K / 8), c = (e % (K / 8)) * 8;
        *reinterpret_cast<uint4*>(tq + r * LDQ + c) = *reinterpret_cast<const uint4*>(h.t_dqkv + row_of(r) * K + c);
    }
    __syncthreads();
    f32x4 acc[TAIL_NW];
#pragma unroll
    for (int i = 0; i < TAIL_NW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint16_t* a0 = tq + j * LDQ + 8 * q;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(a0 + 32 * s);
        acc[s % TAIL_NW] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, __builtin_bit_cast(bf16x8, b[s]), acc[s % TAIL_NW], 0, 0, 0);
    }
    f32x4 sum = acc[0];
#pragma unroll
    for (int i = 1; i < TAIL_NW; ++i) sum += acc[i];
#pragma unroll
    for (int v = 0; v < 4; ++v) {            // (register v of lane (j, q): row 4 q + v, column j of the wave's group)
        float* o = dst + (4 * q + v) * LDA + 16 * wave + j;
        *o = sum[v] + *o;
    }
    __syncthreads();
}

template <int C, int W2, bool HOST>
__device__ __forceinline__ void token_bwd_body(const TokBwdParams& p, const TokHost* hp, float* __restrict__ a4, float* __restrict__ t4) {
    constexpr int LDA = C + 4, LD2 = W2 + 4;
    constexpr int KS4 = gemm_ks<C>(), KS2 = gemm_ks<W2>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = p.N + 1;
    const uint64_t seed = (p.thr_pos || p.thr_in) ? p.seed + (p.seed_dev ? *p.seed_dev : 0ull) : 0ull;
    bool tail = false;
    if constexpr (HOST) {
        const TokHost& h = *hp;
        static_assert(mobgt_wgrad::wgrad_lds_floats<TAIL_NW>() <= (KS4 > KS2 ? KS4 : KS2) * TBM * LDA, "the passenger's LDS");
        static_assert(TBM * (3 * C + 8) * 2 <= (KS4 > KS2 ? KS4 : KS2) * TBM * LDA * 4, "the rows of dqkv");
        if ((int)blockIdx.x >= h.n_chain) {      // passenger: one 32 x 32 tile of one of the first layer's weight gradients
            const int bid = (int)blockIdx.x - h.n_chain;
            int qn = 0;
#pragma unroll
            for (int t = 1; t < HOST_MAX_WG; ++t)
                if (t < h.n_wg && bid >= h.wg_first[t]) qn = t;
            const int local = bid - h.wg_first[qn];
            mobgt_wgrad::wgrad_body<false, TAIL_NW, false, TNW>(h.wg[qn], local % h.wg_tiles[qn], local / h.wg_tiles[qn],
                                                                h.wg_splits[qn], t4);
            return;
        }
        tail = h.t_dqkv != nullptr;
        if ((int)blockIdx.x >= p.n_node_blocks) {
            // ---- the graph-token rows, TBM graphs per workgroup: d(token) (= d(pe[0])) += d of the finished rows
            const int g0 = ((int)blockIdx.x - p.n_node_blocks) * TBM;
            if (tail)
                host_tail<C, LDA>(h, a4, reinterpret_cast<uint16_t*>(t4), [&](int r) { return (int64_t)min(g0 + r, p.G - 1) * T; });
            for (int e = threadIdx.x; e < TBM * C; e += TNT) {
                const int r = e / C, c = e % C, g = min(g0 + r, p.G - 1);
                const int64_t row = (int64_t)g * T;
                float x;
                if (tail) x = a4[r * LDA + c];
                else x = p.dout[row * C + c];
                if (tail && g0 + r < p.G) h.dx1[row * C + c] = x;
                float scale = 1.f;
                if (p.thr_pos) scale = dropout_bits16(seed, dropout_row_hash(seed, (uint32_t)g ^ p.salt_tok), (uint32_t)c) >= p.thr_pos ? p.keep_pos : 0.f;
                if (p.thr_in) scale *= dropout_bits16(seed, dropout_row_hash(seed, (uint32_t)row ^ p.salt_in), (uint32_t)c) >= p.thr_in ? p.keep_in : 0.f;
                a4[r * LDA + c] = g0 + r < p.G ? x * scale : 0.f;          // (the element this thread alone read)
            }
            __syncthreads();
            // the block's graphs are added up in float64 and rounded once: up to TBM graphs, d_token receives the correctly rounded
            // column sums (one f32 add onto the zeroed accumulator), whatever order the old form's per-row atomics land in
            if (threadIdx.x < C) {
                double s = 0.0;
#pragma unroll
                for (int r = 0; r < TBM; ++r) s += (double)a4[r * LDA + threadIdx.x];
                if (s != 0.0) atomicAdd(&p.d_token[threadIdx.x], (float)s);
            }
            return;
        }
    }
    if (!HOST && (int)blockIdx.x >= p.n_node_blocks) {
        // ---- the graph-token rows: d(token) (= d(pe[0])) += d, one wave per graph
        const int g = ((int)blockIdx.x - p.n_node_blocks) * TNW + wave;
        if (g >= p.G) return;
        const int64_t row = (int64_t)g * T;
        const uint32_t h1 = p.thr_pos ? dropout_row_hash(seed, (uint32_t)g ^ p.salt_tok) : 0u;
        const uint32_t h2 = p.thr_in ? dropout_row_hash(seed, (uint32_t)row ^ p.salt_in) : 0u;
        for (int c = lane; c < C; c += 64) {
            float scale = 1.f;
            if (p.thr_pos) scale = dropout_bits16(seed, h1, (uint32_t)c) >= p.thr_pos ? p.keep_pos : 0.f;
            if (p.thr_in) scale *= dropout_bits16(seed, h2, (uint32_t)c) >= p.thr_in ? p.keep_in : 0.f;
            const float d = p.dout[row * C + c] * scale;
            if (d != 0.f) atomicAdd(&p.d_token[c], d);
        }
        return;
    }
    const int64_t R = (int64_t)p.G * p.N;
    const int64_t j0 = (int64_t)blockIdx.x * TBM;
    TSTAMP_DECL;
    TSTAMP(0);
    if constexpr (HOST) {
        // ---- the first layer's input gradient for this block's rows, before they are read: a4 <- dx1 + dqkv Wqkv
        if (tail)
            host_tail<C, LDA>(*hp, a4, reinterpret_cast<uint16_t*>(t4), [&](int r) {
                const int64_t jc = min(j0 + r, R - 1);
                return jc + jc / p.N + 1;                      // (node row (g, n) is token row g T + n + 1)
            });
    }
    // ---- token assembly backwards + FuseEmbeddings-4's activation derivative: TBM x C elements dealt out flat, every load of a
    //      thread requested before the first is used (a wave per row took two dependent passes: 3.6 us)
    constexpr int EPT = TBM * C / TNT;
    static_assert(TBM * C % TNT == 0, "flat split");
    float dv[EPT], yv[EPT], rl[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int e = threadIdx.x + k * TNT, r = e / C, c = e % C;
        const int64_t jc = min(j0 + r, R - 1);
        const int g = (int)(jc / p.N), n = (int)(jc - (int64_t)g * p.N);
        if (HOST && tail) dv[k] = a4[r * LDA + c];            // (this thread alone reads and, below, rewrites the element)
        else dv[k] = p.dout[((int64_t)g * T + n + 1) * C + c];
        yv[k] = p.y4[jc * C + c];
        rl[k] = p.real[jc];
    }
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int e = threadIdx.x + k * TNT, r = e / C, c = e % C;
        const int64_t jn = j0 + r;
        const bool on = jn < R;
        const int64_t jc = on ? jn : R - 1;
        const int g = (int)(jc / p.N), n = (int)(jc - (int64_t)g * p.N);
        const int64_t row = (int64_t)g * T + n + 1;
        float scale = 1.f;
        if (p.thr_pos) scale = dropout_bits16(seed, dropout_row_hash(seed, (uint32_t)jc ^ p.salt_nf), (uint32_t)c) >= p.thr_pos ? p.keep_pos : 0.f;
        if (p.thr_in) scale *= dropout_bits16(seed, dropout_row_hash(seed, (uint32_t)row ^ p.salt_in), (uint32_t)c) >= p.thr_in ? p.keep_in : 0.f;
        const float d = on ? dv[k] * scale : 0.f;
        const float dnf = d * rl[k];
        a4[r * LDA + c] = dnf * leaky_grad(yv[k], p.slope4);
        if (on) {
            if constexpr (HOST) {
                if (tail) hp->dx1[row * C + c] = dv[k];
            }
            p.d_add[jn * C + c] = d;
            p.d_nf[jn * C + c] = dnf;
        }
    }
    __syncthreads();
    TSTAMP(1);
    // ---- dx4 = g4 W4
    gemm_kn<C, C, LDA, LDA>(a4, p.w4, t4);
    __syncthreads();
    TSTAMP(2);
    // dx4 out; g2 = dx4[:, :W2] * LeakyReLU'(f2) -> the next A operand
    for (int e = threadIdx.x; e < TBM * C; e += TNT) {
        const int r = e / C, c = e % C;
        const int64_t jn = j0 + r;
        float v = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS4; ++ks) v += t4[(ks * TBM + r) * LDA + c];
        if (jn < R) p.dx4[jn * p.ldx4 + c] = v;
        if (c < W2) a4[r * LD2 + c] = jn < R ? v * leaky_grad(p.y2[jn * p.ld2 + c], p.slope2) : 0.f;
    }
    __syncthreads();
    TSTAMP(3);
    // ---- d_pt = g2 W2
    gemm_kn<W2, W2, LD2, LD2>(a4, p.w2, t4);
    __syncthreads();
    TSTAMP(4);
    for (int e = threadIdx.x; e < TBM * W2; e += TNT) {
        const int r = e / W2, c = e % W2;
        const int64_t jn = j0 + r;
        float v = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) v += t4[(ks * TBM + r) * LD2 + c];
        if (jn < R) p.d_pt[jn * W2 + c] = v;
    }
    TSTAMP(5);
    TSTAMP_DUMP();
}

// LDS of both kernels (static: 61 KB): a4 = the g4 rows, later the g2 rows (the A operands) -- hosting: first the finished rows
// of d(out); t4 = the partial tiles of dx4, later of d_pt -- hosting: first the rows of dqkv, and the whole of a passenger's LDS
#define TOKBWD_LDS(C, W2)                                                                                                          \
    __shared__ __attribute__((aligned(16))) float a4[TBM * (C + 4)];                                                               \
    __shared__ __attribute__((aligned(16))) float t4[(gemm_ks<C>() > gemm_ks<W2>() ? gemm_ks<C>() : gemm_ks<W2>()) * TBM * (C + 4)]

template <int C, int W2>
__global__ __launch_bounds__(TNT) void token_bwd_chain_kernel(const TokBwdParams p) {
    TOKBWD_LDS(C, W2);
    token_bwd_body<C, W2, false>(p, nullptr, a4, t4);
}

template <int C, int W2>
__global__ __launch_bounds__(TNT) void token_bwd_chain_host_kernel(const TokBwdParams p, const TokHost h) {
    TOKBWD_LDS(C, W2);
    token_bwd_body<C, W2, true>(p, &h, a4, t4);
}

inline int fill_params(TokBwdParams& p, const float* dout, const float* real, const float* y4, const float* y2, int64_t ld_y2, const float* w4,
                const float* w2, float* d_nf, float* d_add, float* dx4, int64_t ld_dx4, float* d_pt, float* d_token, int G, int N,
                int C, int W2, float slope4, float slope2, float p_pos, float p_in, uint64_t seed, const uint64_t* seed_dev,
                uint32_t salt_nf, uint32_t salt_tok, uint32_t salt_in) {
    if (G <= 0 || N <= 0) return MOBGT_EBADDIM;
    if (!(C == 192 && W2 == 160)) return MOBGT_EBADDIM;          // the instantiated widths (MobGT's hidden 128: C = 192, [poi ; time] = 160)
    if (!dout || !real || !y4 || !y2 || !w4 || !w2 || !d_nf || !d_add || !dx4 || !d_pt || !d_token || ld_y2 < W2 || ld_dx4 < C)
        return MOBGT_EBADDIM;
    if (((uintptr_t)w4 | (uintptr_t)w2) & 15) return MOBGT_EALIGN;
    p = {};
    p.dout = dout; p.real = real; p.y4 = y4; p.y2 = y2; p.ld2 = ld_y2; p.w4 = w4; p.w2 = w2; p.d_nf = d_nf; p.d_add = d_add;
    p.dx4 = dx4; p.ldx4 = ld_dx4; p.d_pt = d_pt; p.d_token = d_token; p.G = G; p.N = N; p.slope4 = slope4; p.slope2 = slope2;
    p.thr_pos = p_pos > 0.f ? dropout_threshold(p_pos) : 0u;
    p.thr_in = p_in > 0.f ? dropout_threshold(p_in) : 0u;
    p.keep_pos = p.thr_pos ? 1.f / (1.f - (float)p.thr_pos / 65536.f) : 1.f;
    p.keep_in = p.thr_in ? 1.f / (1.f - (float)p.thr_in / 65536.f) : 1.f;
    p.seed = seed; p.seed_dev = seed_dev; p.salt_nf = salt_nf; p.salt_tok = salt_tok; p.salt_in = salt_in;
    p.n_node_blocks = (int)(((int64_t)G * N + TBM - 1) / TBM);
    return 0;
}

inline int launch_plain(const TokBwdParams& p, void* stream) {
    const dim3 grid(p.n_node_blocks + (p.G + TNW - 1) / TNW), block(TNT);
    hipLaunchKernelGGL((token_bwd_chain_kernel<192, 160>), grid, block, 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

}  // namespace
}  // namespace mobgt_tokbwd
