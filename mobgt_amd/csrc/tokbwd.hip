// mobgt_token_bwd_chain: the encoder input's backward as one launch.  The kernel, its design notes and the parameter fill are in
// tokbwd_body.h, which csrc_tokhost/tokhost.hip compiles as well (the form of this launch that hosts the first layer's tail).
#include "tokbwd_body.h"

using namespace mobgt_tokbwd;

#ifdef TB_STAMP
extern "C" int mobgt_tokbwd_debug_buffer(int* buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_tb_dbg), &buf, sizeof(buf)); }
#endif

extern "C" int mobgt_token_bwd_chain(const float* dout, const float* real, const float* y4, const float* y2, int64_t ld_y2,
                                     const float* w4, const float* w2, float* d_nf, float* d_add, float* dx4, int64_t ld_dx4,
                                     float* d_pt, float* d_token, int G, int N, int C, int W2, float slope4, float slope2,
                                     float p_pos, float p_in, uint64_t seed, const uint64_t* seed_dev, uint32_t salt_nf,
                                     uint32_t salt_tok, uint32_t salt_in, void* stream) {
    TokBwdParams p;
    const int rc = fill_params(p, dout, real, y4, y2, ld_y2, w4, w2, d_nf, d_add, dx4, ld_dx4, d_pt, d_token, G, N, C, W2, slope4, slope2,
                               p_pos, p_in, seed, seed_dev, salt_nf, salt_tok, salt_in);
    return rc ? rc : launch_plain(p, stream);
}
