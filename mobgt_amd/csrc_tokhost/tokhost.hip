// libmobgt_tokhost.so (include/mobgt_tokhost.h): the encoder input's backward launch hosting what the first encoder layer's
// backward left undone.  The kernels and their design notes are ../csrc/tokbwd_body.h's -- one source for this launch and for
// libmobgt_hip's mobgt_token_bwd_chain; only the entry point and its argument checks live here.
#include "mobgt_tokhost.h"
#include "tokbwd_body.h"

using namespace mobgt_tokbwd;

static_assert(MOBGT_TOKHOST_MAX_WG == HOST_MAX_WG, "the kernel's problem slots");
static_assert(MOBGT_TOKHOST_MAX_ROWS == mobgt_wgrad::SHORT_R, "the rows of the 8-wave weight-gradient launch");
static_assert(MOBGT_TOKHOST_EBADDIM == MOBGT_EBADDIM && MOBGT_TOKHOST_EALIGN == MOBGT_EALIGN, "the shared fill's status codes");

extern "C" int mobgt_tokhost_abi_version(void) { return MOBGT_TOKHOST_ABI_VERSION; }

extern "C" int mobgt_tokhost_token_bwd_chain(const float* dout, const float* real, const float* y4, const float* y2, int64_t ld_y2,
                                             const float* w4, const float* w2, float* d_nf, float* d_add, float* dx4, int64_t ld_dx4,
                                             float* d_pt, float* d_token, int G, int N, int C, int W2, float slope4, float slope2,
                                             float p_pos, float p_in, uint64_t seed, const uint64_t* seed_dev, uint32_t salt_nf,
                                             uint32_t salt_tok, uint32_t salt_in, const void* tail_dqkv, const void* tail_wqkv_t,
                                             float* dx1, int n_wg, const void* const* wg_g, const int64_t* wg_ldg,
                                             const void* const* wg_x, const int64_t* wg_ldx, float* const* wg_dw,
                                             const int64_t* wg_ldw, float* const* wg_db, const int* wg_M, const int* wg_N,
                                             void* stream) {
    TokBwdParams p;
    int rc = fill_params(p, dout, real, y4, y2, ld_y2, w4, w2, d_nf, d_add, dx4, ld_dx4, d_pt, d_token, G, N, C, W2, slope4, slope2,
                         p_pos, p_in, seed, seed_dev, salt_nf, salt_tok, salt_in);
    if (rc) return rc;
    if ((tail_dqkv == nullptr) != (tail_wqkv_t == nullptr) || n_wg < 0 || n_wg > MOBGT_TOKHOST_MAX_WG) return MOBGT_TOKHOST_EBADDIM;
    if (tail_dqkv && dx1 != dout) return MOBGT_TOKHOST_EBADDIM;          // (the rows are finished in place: dout IS the layer's dx1)
    if (n_wg && (!wg_g || !wg_ldg || !wg_x || !wg_ldx || !wg_dw || !wg_ldw || !wg_M || !wg_N)) return MOBGT_TOKHOST_EBADDIM;
    if (((uintptr_t)tail_dqkv | (uintptr_t)tail_wqkv_t | (uintptr_t)(tail_dqkv ? dx1 : nullptr)) & 15) return MOBGT_TOKHOST_EALIGN;
    if (!tail_dqkv && n_wg == 0) return launch_plain(p, stream);          // nothing to host: the plain kernel
    if ((int64_t)G * (N + 1) > MOBGT_TOKHOST_MAX_ROWS) return MOBGT_TOKHOST_EBADDIM;
    TokHost h = {};
    h.t_dqkv = reinterpret_cast<const uint16_t*>(tail_dqkv); h.t_wqt = reinterpret_cast<const uint16_t*>(tail_wqkv_t); h.dx1 = dx1;
    h.n_wg = n_wg;
    h.n_chain = p.n_node_blocks + (G + TBM - 1) / TBM;
    int total = 0;
    for (int i = 0; i < n_wg; ++i) {
        // (tiles and splits of mobgt_layer_backward_tail: ~256 workgroups shared by the problems, 8 waves each)
        rc = mobgt_wgrad::fill_problem(h.wg[i], wg_g[i], wg_ldg[i], wg_x[i], wg_ldx[i], wg_dw[i], wg_ldw[i], wg_db ? wg_db[i] : nullptr,
                                       (int64_t)G * (N + 1), wg_M[i], wg_N[i], 256 / n_wg, &h.wg_tiles[i], &h.wg_splits[i], 0, TAIL_NW);
        if (rc) return rc;
        h.wg_first[i] = total;
        total += h.wg_tiles[i] * h.wg_splits[i];
    }
    for (int i = n_wg; i <= MOBGT_TOKHOST_MAX_WG; ++i) h.wg_first[i] = total;
    hipLaunchKernelGGL((token_bwd_chain_host_kernel<192, 160>), dim3(h.n_chain + total), dim3(TNT), 0, (hipStream_t)stream, p, h);
    return (int)hipGetLastError();
}
