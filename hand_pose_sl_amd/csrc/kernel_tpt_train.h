// Training kernels of TextPoseTransformer (HandPoseModels.py:201-222 under autograd; torch.nn.Transformer,
// post-norm, ReLU) beyond TransformerEnc's (kernel_tenc_train.h), in the same style: exact fp32 on the vector
// ALU, one kernel per operation, keep-masks (uint8, 1 = keep) as inputs, `scale` = 1 / (1 - p), a NULL mask
// means p = 0.
//
//   b2h_tptt_xsdpa      the decoder's multihead_attn: O = drop(softmax(Q K^T / sqrt(32))) V between the Tq
//                       target frames of a sequence and the Tk rows of its encoder memory
//   b2h_tptt_xsdpa_bwd  recomputes the probabilities; dQ for the frame rows, [dK | dV] for the memory rows
//   b2h_tptt_embed_bwd  the gradient of token_embedding.weight, every row summed in ascending token order
//
// The Linears, LayerNorms and both self-attentions of the model are b2h_tt_* launches (b2h_api.hip:
// b2h_tpt_train_forward / b2h_tpt_backward have the launch lists); the forward gather is b2h_tpt_embed.
// b2h_tt_sdpa's helpers are used where the two row sets do not matter (tt_load_head, the wave reductions);
// the softmax over two row counts is restated here so that kernel_tenc_train.h stays as it is.
#pragma once
#include "kernel_tenc_train.h"

namespace b2h {

// Dynamic LDS of the two cross-attention kernels: Q (and dO) at stride 33 over Tq rows, K and V at stride 33
// over Tk rows, the (Tq, Tk) probabilities at stride Tk | 1, and (backward) the mask bytes.
// Tq = Tk = 128: 116 736 B forward, 150 016 B backward.
__host__ __device__ inline size_t tptt_xsdpa_lds_bytes(int Tq, int Tk, bool bwd) {
    return (size_t)4 * (((bwd ? 2 : 1) * Tq + 2 * Tk) * kTtQs + Tq * tt_ps(Tk)) + (bwd ? (size_t)(Tq * Tk + 3) / 4 * 4 : 0);
}

// P[i][j] = softmax_j(Q_i . K_j / sqrt(32)), i < Tq, j < Tk <= 128, one wave per row, PRE-dropout:
// tt_softmax_rows's arithmetic with the two ranges kept apart.
__device__ inline void tptt_softmax_rows(const float* Q, const float* K, float* P, int Tq, int Tk) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6, ps = tt_ps(Tk);
    for (int i = w; i < Tq; i += nw) {
        float s[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = lane + 64 * u;
            float a = 0.f;
            if (j < Tk)
#pragma unroll
                for (int d = 0; d < kTtHd; ++d) a = fmaf(Q[i * kTtQs + d], K[j * kTtQs + d], a);
            s[u] = j < Tk ? a * kTtQkScale : -INFINITY;
        }
        const float mx = tt_wave_max(fmaxf(s[0], s[1]));
        const float e0 = expf(s[0] - mx), e1 = lane + 64 < Tk ? expf(s[1] - mx) : 0.f; // lane 0 < Tk always; e0 = 0 past Tk
        const float sum = tt_wave_sum((lane < Tk ? e0 : 0.f) + e1);
        if (lane < Tk) P[i * ps + lane] = e0 / sum;
        if (lane + 64 < Tk) P[i * ps + lane + 64] = e1 / sum;
    }
}

// Where the operands of one cross-attention live: q rows (B*Tq, ldq), the head's 32 columns from colq + 32 h;
// kv rows (B*Tk, ldkv) of the memory, K from colk + 32 h and V from colv + 32 h.
struct XsdpaSrc {
    const float* q;
    int ldq, colq;
    const float* kv;
    int ldkv, colk, colv;
};

// O[i][32 h + d] = sum_j drop(P)[i][j] V[j][d], O (B*Tq, 128); mask (B, 4, Tq, Tk).
// grid B * 4, 256 threads, tptt_xsdpa_lds_bytes(Tq, Tk, false) of dynamic LDS.  1 <= Tq, Tk <= 128.
__global__ __launch_bounds__(256) void b2h_tptt_xsdpa(XsdpaSrc src, const uint8_t* __restrict__ mask, float scale,
                                                      float* __restrict__ O, int Tq, int Tk) {
    extern __shared__ __attribute__((aligned(16))) float smem_tptt[];
    float* Q = smem_tptt;
    float* K = Q + Tq * kTtQs;
    float* V = K + Tk * kTtQs;
    float* P = V + Tk * kTtQs;
    const int64_t b = blockIdx.x / kTtHeads;
    const int h = blockIdx.x % kTtHeads, ps = tt_ps(Tk);
    const float* kv = src.kv + b * Tk * src.ldkv + h * kTtHd;
    tt_load_head(src.q + b * Tq * src.ldq + src.colq + h * kTtHd, src.ldq, Q, Tq);
    tt_load_head(kv + src.colk, src.ldkv, K, Tk);
    tt_load_head(kv + src.colv, src.ldkv, V, Tk);
    __syncthreads();
    tptt_softmax_rows(Q, K, P, Tq, Tk);
    __syncthreads();
    if (mask) {
        const uint8_t* mk = mask + (int64_t)blockIdx.x * Tq * Tk;
        for (int e = threadIdx.x; e < Tq * Tk; e += 256) {
            const int i = e / Tk, j = e % Tk;
            P[i * ps + j] = mk[e] ? P[i * ps + j] * scale : 0.f;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < Tq * kTtHd; e += 256) {
        const int i = e >> 5, d = e & 31;
        float a = 0.f;
        for (int j = 0; j < Tk; ++j) a = fmaf(P[i * ps + j], V[j * kTtQs + d], a);
        O[(b * Tq + i) * kTtD + h * kTtHd + d] = a;
    }
}

// Backward of b2h_tptt_xsdpa for one (sequence, head): b2h_tt_sdpa_bwd's formulas with i < Tq, j < Tk.
// S = softmax (recomputed), Pd = drop(S):
//   dV[j] = sum_i Pd[i][j] dO[i];  dP = dO V^T;  dSd = keep ? dP * scale : 0;  dZ = S o (dSd - rowsum(dSd o S));
//   dQ[i] = sum_j dZ[i][j] K[j] / sqrt(32);  dK[j] = sum_i dZ[i][j] Q[i] / sqrt(32).
// dO (B*Tq, 128) is the gradient of the concatenated heads; dq (B*Tq, 128) receives dQ, dkv (B*Tk, 256)
// receives [dK | dV].  tptt_xsdpa_lds_bytes(Tq, Tk, true) of dynamic LDS.
__global__ __launch_bounds__(256) void b2h_tptt_xsdpa_bwd(XsdpaSrc src, const float* __restrict__ dO,
                                                          const uint8_t* __restrict__ mask, float scale,
                                                          float* __restrict__ dq, float* __restrict__ dkv, int Tq, int Tk) {
    extern __shared__ __attribute__((aligned(16))) float smem_tptt[];
    float* Q = smem_tptt;
    float* G = Q + Tq * kTtQs;
    float* K = G + Tq * kTtQs;
    float* V = K + Tk * kTtQs;
    float* P = V + Tk * kTtQs;
    uint8_t* Mk = reinterpret_cast<uint8_t*>(P + Tq * tt_ps(Tk));
    const int64_t b = blockIdx.x / kTtHeads;
    const int h = blockIdx.x % kTtHeads, ps = tt_ps(Tk);
    const float* kv = src.kv + b * Tk * src.ldkv + h * kTtHd;
    tt_load_head(src.q + b * Tq * src.ldq + src.colq + h * kTtHd, src.ldq, Q, Tq);
    tt_load_head(dO + b * Tq * kTtD + h * kTtHd, kTtD, G, Tq);
    tt_load_head(kv + src.colk, src.ldkv, K, Tk);
    tt_load_head(kv + src.colv, src.ldkv, V, Tk);
    if (mask) {
        const uint8_t* mk = mask + (int64_t)blockIdx.x * Tq * Tk;
        for (int e = threadIdx.x; e < Tq * Tk; e += 256) Mk[e] = mk[e];
    }
    __syncthreads();
    tptt_softmax_rows(Q, K, P, Tq, Tk);
    __syncthreads();
    float* outq = dq + b * Tq * kTtD + h * kTtHd;
    float* outkv = dkv + b * Tk * (2 * kTtD) + h * kTtHd;
    for (int e = threadIdx.x; e < Tk * kTtHd; e += 256) { // dV[j][d] = sum_i Pd[i][j] dO[i][d]
        const int j = e >> 5, d = e & 31;
        float a = 0.f;
        for (int i = 0; i < Tq; ++i) {
            float pd = P[i * ps + j];
            if (mask) pd = Mk[i * Tk + j] ? pd * scale : 0.f;
            a = fmaf(pd, G[i * kTtQs + d], a);
        }
        outkv[(int64_t)j * (2 * kTtD) + kTtD + d] = a;
    }
    __syncthreads();
    {   // P <- dZ / sqrt(32), one wave per query row
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        for (int i = w; i < Tq; i += 4) {
            float sv[2], dsd[2];
            float rs = 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                sv[u] = 0.f;
                dsd[u] = 0.f;
                if (j < Tk) {
                    float a = 0.f;
#pragma unroll
                    for (int d = 0; d < kTtHd; ++d) a = fmaf(G[i * kTtQs + d], V[j * kTtQs + d], a);
                    if (mask) a = Mk[i * Tk + j] ? a * scale : 0.f;
                    sv[u] = P[i * ps + j];
                    dsd[u] = a;
                    rs = fmaf(a, sv[u], rs);
                }
            }
            rs = tt_wave_sum(rs);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                if (j < Tk) P[i * ps + j] = sv[u] * (dsd[u] - rs) * kTtQkScale;
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < Tq * kTtHd; e += 256) { // dQ[i][d] = sum_j dZ[i][j] K[j][d]
        const int i = e >> 5, d = e & 31;
        float a = 0.f;
        for (int j = 0; j < Tk; ++j) a = fmaf(P[i * ps + j], K[j * kTtQs + d], a);
        outq[(int64_t)i * kTtD + d] = a;
    }
    for (int e = threadIdx.x; e < Tk * kTtHd; e += 256) { // dK[j][d] = sum_i dZ[i][j] Q[i][d]
        const int j = e >> 5, d = e & 31;
        float a = 0.f;
        for (int i = 0; i < Tq; ++i) a = fmaf(P[i * ps + j], Q[i * kTtQs + d], a);
        outkv[(int64_t)j * (2 * kTtD) + d] = a;
    }
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
