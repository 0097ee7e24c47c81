// Whole-matrix attention for training, up to 128 x 128 per (sequence, head): every attention of TransformerEnc and of
// TextPoseTransformer's encoder, and the decoder's self- and cross-attention up to 128 frames.  Same style as
// kernel_tenc_train.h: exact fp32 on the vector ALU, keep-masks (uint8, 1 = keep) as inputs, `scale` = 1 / (1 - p),
// a NULL mask means p = 0, fmaf over d ascending and 1 / sqrt(32) applied after the dot product.
//
//   b2h_tt_sdpa      O = drop(softmax(Q K^T / sqrt(32))) V between the Tq query rows and the Tk key rows of one
//                    (sequence, head), the whole (Tq, Tk) matrix in LDS
//   b2h_tt_sdpa_bwd  recomputes the probabilities from Q, K; dQ for the query rows, dK and dV for the key rows
//
// The operands are described by AttnSrc (b2h_common.h) and the gradients' destinations by LtGradDst, so the one pair serves
// self-attention ([Q | K | V] rows at ld 384, Tq = Tk) and cross-attention (QC at ld 128 against the memory's [K | V]
// rows at ld 256), as the blocked kernels beyond 128 rows do (kernel_train_attn_long.h, kernel_train_attn_mfma.h).
// In self-attention q and kv are one buffer, and so are dq and dkv: nothing reached through the two structs is
// __restrict__.
#pragma once
#include "kernel_tenc_train.h"

namespace b2h {

// Where the gradients of one attention go (AttnSrc's counterpart, b2h_common.h): dQ rows (B*Tq, lddq) from column coldq + 32 h; dK and dV rows
// (B*Tk, lddkv) from coldk + 32 h and coldv + 32 h.
struct LtGradDst {
    float* dq;
    int lddq, coldq;
    float* dkv;
    int lddkv, coldk, coldv;
};

// Key-padding mask as a key length: sequence b attends to its key rows 0 .. kl - 1 only, with
// kl = klen[b] clamped to [1, Tk], or Tk without klen.  Tk stays the stride of the rows and of the keep-masks.
__device__ inline int tt_key_len(const int64_t* __restrict__ klen, int64_t b, int Tk) {
    if (!klen) return Tk;
    const int64_t n = klen[b];
    return n < 1 ? 1 : n > Tk ? Tk : (int)n;
}

__host__ __device__ inline int tt_ps(int Tk) { return Tk | 1; } // LDS row stride of the (Tq, Tk) probabilities

// Dynamic LDS of the pair: Q (and dO) at stride 33 over Tq rows, K and V at stride 33 over Tk rows, the (Tq, Tk)
// probabilities at stride Tk | 1, and (backward) the mask bytes.  Tq = Tk = 128: 116 736 B forward, 150 016 B backward.
__host__ __device__ inline size_t tt_sdpa_lds_bytes(int Tq, int Tk, bool bwd) {
    return (size_t)4 * (((bwd ? 2 : 1) * Tq + 2 * Tk) * kTtQs + Tq * tt_ps(Tk)) + (bwd ? (size_t)(Tq * Tk + 3) / 4 * 4 : 0);
}

// n rows of 32 floats from src (leading dimension ld) into LDS at stride 33; every caller runs 256 threads
__device__ inline void tt_load_head(const float* __restrict__ src, int ld, float* dst, int n) {
    for (int e = threadIdx.x; e < n * kTtHd; e += 256) {
        const int i = e >> 5, d = e & 31;
        dst[i * kTtQs + d] = src[(int64_t)i * ld + d];
    }
}

// P[i][j] = softmax_j(Q_i . K_j / sqrt(32)), i < Tq, j < Tk <= 128, one wave per row (a lane: keys lane and
// lane + 64), PRE-dropout.  The softmax runs over the keys j < kl <= Tk; P[i][j] is written as +0 for kl <= j < Tk, so
// that every sum over the Tk keys downstream adds true zeros for them.
__device__ inline void tt_softmax_rows(const float* Q, const float* K, float* P, int Tq, int Tk, int kl) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6, ps = tt_ps(Tk);
    for (int i = w; i < Tq; i += nw) {
        float s[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = lane + 64 * u;
            float a = 0.f;
            if (j < kl)
#pragma unroll
                for (int d = 0; d < kTtHd; ++d) a = fmaf(Q[i * kTtQs + d], K[j * kTtQs + d], a);
            s[u] = j < kl ? a * kTtQkScale : -INFINITY;
        }
        const float mx = tt_wave_max(fmaxf(s[0], s[1]));
        const float e0 = expf(s[0] - mx), e1 = lane + 64 < kl ? expf(s[1] - mx) : 0.f; // lane 0 < kl always; e0 = 0 past kl
        const float sum = tt_wave_sum((lane < kl ? e0 : 0.f) + e1);
        if (lane < Tk) P[i * ps + lane] = e0 / sum;
        if (lane + 64 < Tk) P[i * ps + lane + 64] = e1 / sum; // 0 / sum = +0 from kl on
    }
}

// O[i][32 h + d] = sum_j drop(P)[i][j] V[j][d], O (B*Tq, 128); mask (B, 4, Tq, Tk).
// grid B * 4, 256 threads, tt_sdpa_lds_bytes(Tq, Tk, false) of dynamic LDS.  1 <= Tq, Tk <= 128.  klen: (B) key lengths
// or NULL (tt_key_len).
__global__ __launch_bounds__(256) void b2h_tt_sdpa(AttnSrc src, const uint8_t* __restrict__ mask, float scale,
                                                   float* __restrict__ O, int Tq, int Tk,
                                                   const int64_t* __restrict__ klen) {
    extern __shared__ __attribute__((aligned(16))) float smem_tt[];
    float* Q = smem_tt;
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
    tt_softmax_rows(Q, K, P, Tq, Tk, tt_key_len(klen, b, Tk));
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

// Backward of b2h_tt_sdpa for one (sequence, head), i < Tq, j < Tk.  S = softmax (recomputed), Pd = drop(S):
//   dV[j] = sum_i Pd[i][j] dO[i];  dP = dO V^T;  dSd = keep ? dP * scale : 0;  dZ = S o (dSd - rowsum(dSd o S));
//   dQ[i] = sum_j dZ[i][j] K[j] / sqrt(32);  dK[j] = sum_i dZ[i][j] Q[i] / sqrt(32).
// dO (B*Tq, 128) is the gradient of the concatenated heads.  tt_sdpa_lds_bytes(Tq, Tk, true) of dynamic LDS: Q, dO,
// K, V, the (Tq, Tk) matrix and the mask bytes.  With klen the rows kl .. Tk - 1 of dK and dV are written as +0: their
// columns of S and of dZ are +-0, and a sum that starts at +0 and adds +-0 stays +0.
__global__ __launch_bounds__(256) void b2h_tt_sdpa_bwd(AttnSrc src, const float* __restrict__ dO,
                                                       const uint8_t* __restrict__ mask, float scale, LtGradDst dst,
                                                       int Tq, int Tk, const int64_t* __restrict__ klen) {
    extern __shared__ __attribute__((aligned(16))) float smem_tt[];
    float* Q = smem_tt;
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
    tt_softmax_rows(Q, K, P, Tq, Tk, tt_key_len(klen, b, Tk));
    __syncthreads();
    float* outq = dst.dq + b * Tq * dst.lddq + dst.coldq + h * kTtHd;
    float* outkv = dst.dkv + b * Tk * dst.lddkv + h * kTtHd;
    for (int e = threadIdx.x; e < Tk * kTtHd; e += 256) { // dV[j][d] = sum_i Pd[i][j] dO[i][d]
        const int j = e >> 5, d = e & 31;
        float a = 0.f;
        for (int i = 0; i < Tq; ++i) {
            float pd = P[i * ps + j];
            if (mask) pd = Mk[i * Tk + j] ? pd * scale : 0.f;
            a = fmaf(pd, G[i * kTtQs + d], a);
        }
        outkv[(int64_t)j * dst.lddkv + dst.coldv + d] = a;
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
        outq[(int64_t)i * dst.lddq + d] = a;
    }
    for (int e = threadIdx.x; e < Tk * kTtHd; e += 256) { // dK[j][d] = sum_i dZ[i][j] Q[i][d]
        const int j = e >> 5, d = e & 31;
        float a = 0.f;
        for (int i = 0; i < Tq; ++i) a = fmaf(P[i * ps + j], Q[i * kTtQs + d], a);
        outkv[(int64_t)j * dst.lddkv + dst.coldk + d] = a;
    }
}

} // namespace b2h
