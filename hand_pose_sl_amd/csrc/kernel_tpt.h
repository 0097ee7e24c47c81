// TextPoseTransformer (body2hand/src/models/HandPoseModels.py:181-230) on gfx950: the three kernels the
// text-conditioned model needs beyond TransformerEnc's (kernel_tenc.h).  Inference, exact fp32.
//
//   b2h_tpt_embed        token_embedding(input_tokens) (:206): row n of the (B*S, 128) encoder input is
//                        table[tokens[n]], not scaled.
//   b2h_attn_cross_f32   the decoder's multihead_attn: queries are the Tq target frames of a sequence, keys and
//                        values the Tk rows of the encoder memory of the same sequence.  The reference passes no
//                        mask (:211), so every memory row is attended, padded token ids included.
//   b2h_tpt_layernorm    encoder.norm / decoder.norm, the LayerNorm that ends each stack of torch.nn.Transformer.
//
// Everything else of the model is per-frame and runs as descriptors of b2h_tenc_chain<false>; the decoder's
// self-attention is b2h_attn_mfma_f32 (b2h_api.hip: b2h_tpt_forward has the launch list).
#pragma once
#include "kernel_tenc.h"

namespace b2h {

// out[n] = table[tokens[n]], one float4 per thread (32 threads per row).  An id outside [0, n_tokens) never
// reads the table: its row becomes 128 NaNs, which every later layer carries to that sequence's output (and
// to no other: attention never crosses sequences), so the error is visible without a host synchronisation
// (nn.Embedding raises IndexError on the host there).
__global__ __launch_bounds__(256) void b2h_tpt_embed(const int64_t* __restrict__ tokens, const float* __restrict__ table,
                                                     float* __restrict__ out, int64_t n, int n_tokens) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = i >> 5;
    const int c = (int)(i & 31);
    if (row >= n) return;
    const int64_t id = tokens[row];
    float4 v = make_float4(NAN, NAN, NAN, NAN);
    if (id >= 0 && id < n_tokens) v = reinterpret_cast<const float4*>(table + id * kTencD)[c];
    reinterpret_cast<float4*>(out + row * kTencD)[c] = v;
}

// y = (x - mean) / sqrt(var + 1e-5) * gamma + beta over 128 features, var biased (torch.nn.LayerNorm).
// Half a wave per row, one float4 per lane; b2h_tt_layernorm (kernel_tenc_train.h) without the saved
// statistics.  Y may be X: a lane writes only the four features it has read.
__global__ __launch_bounds__(256) void b2h_tpt_layernorm(const float* X, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* Y, int64_t n) {
    const int64_t row = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int c = threadIdx.x & 31;
    if (row >= n) return; // whole half-waves leave: the shuffles below stay inside one 32-lane half
    const float4 v = reinterpret_cast<const float4*>(X + row * kTencD)[c];
    float s = (v.x + v.y) + (v.z + v.w);
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    const float mean = s * (1.0f / kTencD);
    const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
    float var = (dx * dx + dy * dy) + (dz * dz + dw * dw);
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) var += __shfl_xor(var, m, 64);
    const float rstd = 1.0f / sqrtf(var * (1.0f / kTencD) + 1e-5f);
    const float4 g = reinterpret_cast<const float4*>(gamma)[c], b = reinterpret_cast<const float4*>(beta)[c];
    reinterpret_cast<float4*>(Y + row * kTencD)[c] =
        make_float4(dx * rstd * g.x + b.x, dy * rstd * g.y + b.y, dz * rstd * g.z + b.z, dw * rstd * g.w + b.w);
}

// Cross-attention on the matrix cores, exact fp32 (v_mfma_f32_16x16x4_f32).  Everything after the operands are
// staged is attn_core_f32 (kernel_tenc.h), which b2h_attn_mfma_f32 runs too: q pre-scaled by 32^-0.5, K and V rows
// in LDS at the 36-float pitch.  What differs is where the operands come from:
//   q   : (B*Tq, ldq)  rows, the head's 32 columns start at colq + 32 h
//   kv  : (B*Tk, ldkv) rows of ANOTHER row set, K at colk + 32 h and V at colv + 32 h
//   out : (B*Tq, 128), head h -> columns 32 h ..
// Workgroup = (sequence, head); wave w owns query tile w, so the block size is 64 * ceil(Tq / 16) (<= 512) and
// only the key-tile count NK = ceil(Tk / 16) is a template parameter: 8 instantiations, not 8 x 8.  All global
// accesses are buffer instructions over the sequence's rows: key rows >= Tk read 0 and are masked to -inf,
// query rows >= Tq read 0 (a uniform softmax over the valid keys, finite) and their stores are dropped by the
// range check; nothing is predicated.
template <int NK>
__global__ __launch_bounds__(64 * kAttnMaxTiles) void b2h_attn_cross_f32(const float* __restrict__ qm, int ldq, int colq,
                                                                         const float* __restrict__ kv, int ldkv, int colk,
                                                                         int colv, float* __restrict__ out, int Tq, int Tk) {
    extern __shared__ __attribute__((aligned(16))) char smem_attnx[];
    float* Ks = reinterpret_cast<float*>(smem_attnx);
    float* Vs = reinterpret_cast<float*>(smem_attnx + attn_f32_lds_bytes(NK) / 2);
    const int b = blockIdx.x / kTencHeads, h = blockIdx.x % kTencHeads;
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(kv + (int64_t)b * Tk * ldkv, Tk * ldkv * 4);
    const __amdgpu_buffer_rsrc_t qrs = make_rsrc(qm + (int64_t)b * Tq * ldq, Tq * ldq * 4);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nthreads = __builtin_amdgcn_readfirstlane(blockDim.x);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const int tq = wave * 16 + col;
    f32x4 qb[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) // B operand of S^T: d = 16g + 4q + j
        qb[g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
            qrs, (tq * ldq + colq + h * kTencHd + 16 * g + 4 * q) * 4, 0, 0));
    // K, V rows of the head: NK*16 rows x 8 float4 each, two per thread and round (one round when Tq and Tk
    // have the same tile count); every LDS row below 16 NK is written, rows >= Tk with the zeros of the range check
    constexpr int kChunks = NK * 16 * 8;
#pragma unroll 1
    for (int i0 = threadIdx.x; i0 < kChunks; i0 += 2 * nthreads) {
        f32x4 k4[2], v4[2];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int i = i0 + it * nthreads, t = i >> 3, c = i & 7;
            const int off = i < kChunks ? (t * ldkv + h * kTencHd + 4 * c) * 4 : (int)kOob;
            k4[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, off, colk * 4, 0));
            v4[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, off, colv * 4, 0));
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int i = i0 + it * nthreads, t = i >> 3, c = i & 7;
            if (i < kChunks) {
                *reinterpret_cast<f32x4*>(Ks + t * kAttnRow + 4 * c) = k4[it];
                *reinterpret_cast<f32x4*>(Vs + t * kAttnRow + 4 * c) = v4[it];
            }
        }
    }
    qb[0] *= 0.17677669529663687f; // pre-scaled query (torch scales q, not the scores)
    qb[1] *= 0.17677669529663687f;
    __syncthreads();
    attn_core_f32<NK>(Ks, Vs, qb, Tk, out, Tq, b, h, tq, col, q);
}

} // namespace b2h
