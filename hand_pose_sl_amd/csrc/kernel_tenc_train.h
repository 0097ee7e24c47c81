// Training kernels of TransformerEnc (HandPoseModels.py:154-178 under autograd; torch's post-norm
// nn.TransformerEncoderLayer with ReLU), exact fp32 on the vector ALU, one kernel per operation, no fusion.
//
// Every kernel reads the parameters straight from the caller's fp32 tensors in state_dict layout, passed per
// launch.  Dropout keep-masks (one uint8 per element, 1 = keep) are INPUTS, drawn by the caller; `scale` is
// 1 / (1 - p) (0 at p = 1, where torch multiplies by zero); a NULL mask means p = 0: nothing is scaled.
// Rows are frames, n = b * T + t, N = B * T of them; activations are row-major (N, width).
//
//   b2h_tt_posenc        X0 = drop((x + pe[t]))                                              (:101-103)
//   b2h_tt_linear        Y = X W^T + b  [ReLU] [keep-mask] [+ residual]
//   b2h_tt_linear_dx     dX = dY W  [gate: (g > 0) * scale] [keep-mask] [+ add]
//   b2h_tt_linear_dw     slab partials of dW = dY^T X and db = sum dY
//   b2h_tt_layernorm     y = (x - mean) rstd gamma + beta, saves mean / rstd (eps 1e-5, biased variance)
//   b2h_tt_layernorm_bwd dx [and dx through a keep-mask], slab partials of dgamma / dbeta
//   b2h_tt_reduce        sums the slabs in ascending order into the gradient tensors
//
// The attention pair b2h_tt_sdpa / b2h_tt_sdpa_bwd is in kernel_train_attn.h, which builds on this header's
// constants and wave reductions.
//
// Parameter gradients are bitwise deterministic: workgroup s of a *_dw / *_bwd launch owns the row tiles
// s, s + S, s + 2S, ... (S = tt_nslabs(N), a function of (B, T) only), sums them in that order in
// registers and writes slab s; b2h_tt_reduce adds the S slabs in ascending order.  No float atomics, no
// last-arriver handoff.  Everything that produces dx is row-wise or per sequence, so a sequence's dx
// depends on that sequence alone.
#pragma once
#include "b2h_common.h"

namespace b2h {

constexpr int kTtD = 128, kTtHeads = 4, kTtHd = 32; // nhid, nhead, head width
constexpr int kTtRows = 16;                         // rows per workgroup of b2h_tt_linear / _dx
constexpr int kTtDwRows = 64, kTtDwM = 32;          // row tile and output-row tile of b2h_tt_linear_dw
constexpr int kTtMaxSlabs = 64;
constexpr int kTtQs = kTtHd + 1;                    // LDS row stride of Q, K, V, dO (odd: conflict-free columns)
constexpr float kTtLnEps = 1e-5f;
constexpr float kTtQkScale = kAttnQkScale;          // 1 / sqrt(32)

__host__ __device__ inline int tt_nslabs(int64_t N) {
    const int64_t t = (N + 2 * kTtDwRows - 1) / (2 * kTtDwRows);
    return (int)(t < 1 ? 1 : (t > kTtMaxSlabs ? kTtMaxSlabs : t));
}

__device__ inline float tt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline float tt_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// A store in an unrolled, branchy epilogue, followed by two wait states.  Not a hardware requirement: the hazard of
// DESIGN.md section 4 concerns stores of more than 64 bits of data, and the compiler pads those itself; a dword
// store whose data register is reused for the next row is safe.  tools/store_war_audit.py does not tell the two
// apart and the project keeps its count at zero over the whole listing, so the reuse is moved out of its window
// (as kernel_tenc.h does in its output head).  Cost: 16 idle cycles per thread and output column.
__device__ inline void tt_store(float* p, float v) {
    *p = v;
    asm volatile("s_nop 1" ::: "memory");
}

// X0[n][c] = (x[n][c] + pe[t][c]) * keep * scale, c < 24
__global__ __launch_bounds__(256) void b2h_tt_posenc(const float* __restrict__ x, const float* __restrict__ pe,
                                                     const uint8_t* __restrict__ mask, float scale,
                                                     float* __restrict__ out, int64_t N, int T) {
    const int64_t total = N * kInCh;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = e / kInCh;
        const int c = (int)(e % kInCh), t = (int)(n % T);
        float v = x[e] + pe[t * kInCh + c];
        if (mask) v = mask[e] ? v * scale : 0.f;
        out[e] = v;
    }
}

// Y[n][m] = b[m] + sum_k X[n][k] W[m][k], any K <= 128, any M; then, in torch's order:
// ReLU, keep-mask (mask (N, M)), + res (N, M).  One workgroup (128 threads) per 16 rows, a thread per column.
// The rows lie in LDS at the pitch Kp = K rounded up to 4 with zeros behind column K, and the weights past a row's end
// enter as zeros, so the float4 steps stay aligned and add exact zeros; per output the sum runs over k ascending.
__global__ __launch_bounds__(128) void b2h_tt_linear(const float* __restrict__ X, const float* __restrict__ W,
                                                     const float* __restrict__ bias, float* __restrict__ Y,
                                                     int64_t N, int K, int M, int relu,
                                                     const uint8_t* __restrict__ mask, float scale,
                                                     const float* __restrict__ res) {
    __shared__ __attribute__((aligned(16))) float Xs[kTtRows * kTtD];
    const int64_t n0 = (int64_t)blockIdx.x * kTtRows;
    const int nrows = (int)(N - n0 < kTtRows ? N - n0 : kTtRows); // a 32-bit scalar bound for the store loops
    const int Kp = (K + 3) & ~3;
    for (int i = threadIdx.x; i < kTtRows * Kp; i += 128) {
        const int64_t n = n0 + i / Kp;
        const int k = i % Kp;
        Xs[i] = (n < N && k < K) ? X[n * K + k] : 0.f;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < M; m += 128) {
        float acc[kTtRows];
        const float b = bias[m];
#pragma unroll
        for (int r = 0; r < kTtRows; ++r) acc[r] = b;
        const float* w = W + (size_t)m * K;
        for (int k = 0; k < K; k += 4) {
            const float w0 = w[k], w1 = k + 1 < K ? w[k + 1] : 0.f, w2 = k + 2 < K ? w[k + 2] : 0.f, w3 = k + 3 < K ? w[k + 3] : 0.f;
#pragma unroll
            for (int r = 0; r < kTtRows; ++r) {
                const float4 xv = *reinterpret_cast<const float4*>(Xs + r * Kp + k);
                acc[r] = fmaf(xv.w, w3, fmaf(xv.z, w2, fmaf(xv.y, w1, fmaf(xv.x, w0, acc[r]))));
            }
        }
#pragma unroll
        for (int r = 0; r < kTtRows; ++r) {
            if (r >= nrows) break;
            const int64_t n = n0 + r;
            float v = acc[r];
            if (relu) v = fmaxf(v, 0.f);
            if (mask) v = mask[n * M + m] ? v * scale : 0.f;
            if (res) v += res[n * M + m];
            tt_store(Y + n * M + m, v);
        }
    }
}

// dX[n][k] = sum_m dY[n][m] W[m][k], K <= 128, M <= 384; then
//   gate (N, K): dX = gate > 0 ? dX * scale : 0   (ReLU and its dropout: gate is the post-dropout activation)
//   mask (N, K): dX = keep ? dX * scale : 0
//   add  (N, K): dX += add                        (the residual branch)
__global__ __launch_bounds__(128) void b2h_tt_linear_dx(const float* __restrict__ dY, const float* __restrict__ W,
                                                        float* __restrict__ dX, int64_t N, int K, int M,
                                                        const float* __restrict__ gate,
                                                        const uint8_t* __restrict__ mask, float scale,
                                                        const float* __restrict__ add) {
    __shared__ float Ys[kTtRows * 3 * kTtD];
    const int64_t n0 = (int64_t)blockIdx.x * kTtRows;
    const int nrows = (int)(N - n0 < kTtRows ? N - n0 : kTtRows); // a 32-bit scalar bound for the store loops
    for (int i = threadIdx.x; i < kTtRows * M; i += 128) {
        const int64_t n = n0 + i / M;
        Ys[i] = n < N ? dY[n * M + i % M] : 0.f;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= K) return;
    float acc[kTtRows];
#pragma unroll
    for (int r = 0; r < kTtRows; ++r) acc[r] = 0.f;
    for (int m = 0; m < M; ++m) {
        const float w = W[(size_t)m * K + k];
#pragma unroll
        for (int r = 0; r < kTtRows; ++r) acc[r] = fmaf(Ys[r * M + m], w, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kTtRows; ++r) {
        if (r >= nrows) break;
        const int64_t n = n0 + r;
        float v = acc[r];
        if (gate) v = gate[n * K + k] > 0.f ? v * scale : 0.f;
        if (mask) v = mask[n * K + k] ? v * scale : 0.f;
        if (add) v += add[n * K + k];
        tt_store(dX + n * K + k, v);
    }
}

// Slab partials of dW[m][k] = sum_n dY[n][m] X[n][k] and db[m] = sum_n dY[n][m], any K <= 128 (X in LDS at the pitch
// Kp = K rounded up to 4, zeros behind column K; a thread stores only its columns < K).
// grid (S, ceil(M / 32)): workgroup (s, j) owns output rows 32 j .. and the row tiles s, s + S, ... of 64 rows,
// summed in ascending row order in registers (a thread: 4 output rows x 4 columns), and writes them into
// slab s = [dW (M, K) | db (M)].
__global__ __launch_bounds__(256) void b2h_tt_linear_dw(const float* __restrict__ dY, const float* __restrict__ X,
                                                        float* __restrict__ slabs, int64_t slab, int64_t N, int K,
                                                        int M) {
    __shared__ __attribute__((aligned(16))) float Ys[kTtDwRows * kTtDwM];
    __shared__ __attribute__((aligned(16))) float Xs[kTtDwRows * kTtD];
    const int m0 = blockIdx.y * kTtDwM;
    const int tm = threadIdx.x >> 5, tk = threadIdx.x & 31; // output rows m0 + 4 tm .., columns 4 tk ..
    const bool live = 4 * tk < K;
    const int Kp = (K + 3) & ~3;
    float acc[4][4], accb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        accb[u] = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
    }
    const int64_t ntiles = (N + kTtDwRows - 1) / kTtDwRows;
    for (int64_t q = blockIdx.x; q < ntiles; q += gridDim.x) {
        const int64_t n0 = q * kTtDwRows;
        __syncthreads(); // the previous tile is done with LDS
        for (int i = threadIdx.x; i < kTtDwRows * kTtDwM; i += 256) {
            const int64_t n = n0 + i / kTtDwM;
            const int m = m0 + i % kTtDwM;
            Ys[i] = (n < N && m < M) ? dY[n * M + m] : 0.f;
        }
        for (int i = threadIdx.x; i < kTtDwRows * Kp; i += 256) {
            const int64_t n = n0 + i / Kp;
            const int k = i % Kp;
            Xs[i] = (n < N && k < K) ? X[n * K + k] : 0.f;
        }
        __syncthreads();
        if (live)
            for (int r = 0; r < kTtDwRows; ++r) { // rows past N hold zeros
                const float4 y = *reinterpret_cast<const float4*>(Ys + r * kTtDwM + 4 * tm);
                const float4 x = *reinterpret_cast<const float4*>(Xs + r * Kp + 4 * tk);
                const float yy[4] = {y.x, y.y, y.z, y.w}, xx[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    accb[u] += yy[u];
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(yy[u], xx[v], acc[u][v]);
                }
            }
    }
    if (!live) return;
    float* out = slabs + (int64_t)blockIdx.x * slab;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int m = m0 + 4 * tm + u;
        if (m >= M) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (4 * tk + v < K) out[(size_t)m * K + 4 * tk + v] = acc[u][v];
        if (tk == 0) out[(size_t)M * K + m] = accb[u];
    }
}

// g0[e] = sum_s slabs[s][e] (e < n0), g1[e - n0] = sum_s slabs[s][e] (n0 <= e < n0 + n1), s ascending.
__global__ __launch_bounds__(256) void b2h_tt_reduce(const float* __restrict__ slabs, int64_t slab, int nslabs,
                                                     float* __restrict__ g0, int n0, float* __restrict__ g1, int n1) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n0 + n1) return;
    float s = 0.f;
    for (int k = 0; k < nslabs; ++k) s += slabs[(int64_t)k * slab + e];
    if (e < n0) g0[e] = s;
    else g1[e - n0] = s;
}

// LayerNorm over 128 features, one wave per row (a lane: features lane and lane + 64):
//   y = (x - mean) * rstd * gamma + beta,  rstd = 1 / sqrt(var + 1e-5), var biased; stats[n] = {mean, rstd}.
__global__ __launch_bounds__(256) void b2h_tt_layernorm(const float* __restrict__ X, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ Y,
                                                        float* __restrict__ stats, int stats_ld, int64_t N) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float a = X[n * kTtD + lane], b = X[n * kTtD + lane + 64];
    const float mean = tt_wave_sum(a + b) * (1.f / kTtD);
    const float da = a - mean, db = b - mean;
    const float var = tt_wave_sum(fmaf(da, da, db * db)) * (1.f / kTtD);
    const float rstd = 1.f / sqrtf(var + kTtLnEps);
    Y[n * kTtD + lane] = fmaf(da * rstd, gamma[lane], beta[lane]);
    Y[n * kTtD + lane + 64] = fmaf(db * rstd, gamma[lane + 64], beta[lane + 64]);
    if (lane == 0) {
        stats[n * stats_ld] = mean;
        stats[n * stats_ld + 1] = rstd;
    }
}

// LayerNorm backward.  xhat = (x - mean) rstd, g = dy gamma:
//   dx = rstd * (g - mean(g) - xhat * mean(g xhat));  dxm = keep ? dx * scale : 0 (when mask != NULL)
//   dgamma = sum_n dy xhat,  dbeta = sum_n dy  -> slab s = [dgamma (128) | dbeta (128)].
// grid S: wave w of workgroup s owns the rows 4 q + w of the row groups q = s, s + S, ..., in ascending
// order; the four waves' sums are added in wave order.
__global__ __launch_bounds__(256) void b2h_tt_layernorm_bwd(const float* __restrict__ dY, const float* __restrict__ X,
                                                            const float* __restrict__ stats, int stats_ld,
                                                            const float* __restrict__ gamma, float* __restrict__ dX,
                                                            float* __restrict__ dXm, const uint8_t* __restrict__ mask,
                                                            float scale, float* __restrict__ slabs, int64_t slab,
                                                            int64_t N) {
    __shared__ float part[4][2 * kTtD];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float g0 = gamma[lane], g1 = gamma[lane + 64];
    float dg0 = 0.f, dg1 = 0.f, db0 = 0.f, db1 = 0.f;
    const int64_t ngroups = (N + 3) / 4;
    for (int64_t q = blockIdx.x; q < ngroups; q += gridDim.x) {
        const int64_t n = q * 4 + w;
        if (n >= N) break;
        const float mean = stats[n * stats_ld], rstd = stats[n * stats_ld + 1];
        const float y0 = dY[n * kTtD + lane], y1 = dY[n * kTtD + lane + 64];
        const float h0 = (X[n * kTtD + lane] - mean) * rstd, h1 = (X[n * kTtD + lane + 64] - mean) * rstd;
        const float a0 = y0 * g0, a1 = y1 * g1;
        const float c1 = tt_wave_sum(a0 + a1) * (1.f / kTtD);
        const float c2 = tt_wave_sum(fmaf(a0, h0, a1 * h1)) * (1.f / kTtD);
        const float d0 = rstd * (a0 - c1 - h0 * c2), d1 = rstd * (a1 - c1 - h1 * c2);
        dX[n * kTtD + lane] = d0;
        dX[n * kTtD + lane + 64] = d1;
        if (mask) {
            dXm[n * kTtD + lane] = mask[n * kTtD + lane] ? d0 * scale : 0.f;
            dXm[n * kTtD + lane + 64] = mask[n * kTtD + lane + 64] ? d1 * scale : 0.f;
        }
        dg0 = fmaf(y0, h0, dg0);
        dg1 = fmaf(y1, h1, dg1);
        db0 += y0;
        db1 += y1;
    }
    part[w][lane] = dg0;
    part[w][lane + 64] = dg1;
    part[w][kTtD + lane] = db0;
    part[w][kTtD + lane + 64] = db1;
    __syncthreads();
    const int e = threadIdx.x; // 256 threads, 256 slab elements
    slabs[(int64_t)blockIdx.x * slab + e] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
}

} // namespace b2h
