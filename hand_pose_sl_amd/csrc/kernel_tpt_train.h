// The training kernels of TextPoseTransformer (HandPoseModels.py:201-222 under autograd; torch.nn.Transformer,
// post-norm, ReLU) that TransformerEnc has no use for, in the style of kernel_tenc_train.h:
//
//   b2h_tptt_embed_bwd  the gradient of token_embedding.weight, every row summed in ascending token order
//   b2h_embed_dwords    the forward gather for a caller's table that starts off the 16-byte grid
//
// The Linears and LayerNorms of the model are kernel_tenc_train.h's, its attentions -- the encoder's, the decoder's
// self- and cross-attention -- kernel_train_attn.h's b2h_tt_sdpa / b2h_tt_sdpa_bwd up to 128 frames and the blocked
// kernels beyond (b2h_api.hip: b2h_tpt_train_forward / b2h_tpt_backward have the launch lists); the forward gather
// is b2h_tpt_embed (b2h_embed_dwords below for a table off the 16-byte grid).
#pragma once
#include "kernel_tenc_train.h"

namespace b2h {

// b2h_tpt_embed for a table off the 16-byte grid: the training calls read the caller's token_embedding.weight, which
// they promise 4-byte aligned only, so each thread takes its four words as dwords.  Same grid, same rows, same NaN
// rule; `out` is the saved buffer (16-byte checked).  A table on the grid runs b2h_tpt_embed itself (b2h_api.hip).
__global__ __launch_bounds__(256) void b2h_embed_dwords(const int64_t* __restrict__ tokens, const float* __restrict__ table,
                                                      float* __restrict__ out, int64_t n, int n_tokens) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = i >> 5;
    const int c = (int)(i & 31);
    if (row >= n) return;
    const int64_t id = tokens[row];
    float4 v = make_float4(NAN, NAN, NAN, NAN);
    if (id >= 0 && id < n_tokens) {
        const float* src = table + id * kTtD + 4 * c;
        v = make_float4(src[0], src[1], src[2], src[3]);
    }
    reinterpret_cast<float4*>(out + row * kTtD)[c] = v;
}

// dTable[v][c] = sum of dE[n][c] over the token rows n < N with tokens[n] == v, in ascending n; a row no token
// hits becomes +0.  grid n_tokens (workgroup v owns table row v), 128 threads (a thread per column).  Every
// workgroup scans all N ids (the same address in every lane: scalar loads), so the order of the additions
// depends on the ids alone: no atomics.  An id outside [0, n_tokens) equals no v: it is skipped and indexes nothing.
__global__ __launch_bounds__(128) void b2h_tptt_embed_bwd(const int64_t* __restrict__ tokens, const float* __restrict__ dE,
                                                          float* __restrict__ dTable, int64_t N) {
    const int64_t v = blockIdx.x;
    float acc = 0.f;
    for (int64_t n = 0; n < N; ++n)
        if (tokens[n] == v) acc += dE[n * kTtD + threadIdx.x];
    dTable[v * kTtD + threadIdx.x] = acc;
}

} // namespace b2h
