// Training kernels of ConvModel (HandPoseModels.py:40-64 under autograd), exact fp32 on the vector ALU.
//
// Every kernel reads the weights straight from the eight fp32 tensors in state_dict layout
// (w1 (C, 24|25, 5), b1 (C), ..., w4 (42, C, 5), b4 (42)), passed per launch: a training step needs
// neither the model's packed buffers nor a host synchronisation.
//
// b2h_train_conv<MODE> -- one workgroup (256 threads) per frame tile of one sequence:
//   MODE 0 (forward): tiles of kTrainFwdTile frames, +-8 frame halo; layers 1-3 into LDS, layer 4 to y.
//   MODE 1 / 2 (backward, 2 = also dx): tiles of kTrainBwdTile frames, +-12 frame halo.  Layers 1-3 are
//     recomputed in LDS, then dL/dy (staged with +-8 frames) is back-propagated layer by layer: dz_l
//     overwrites a_l in place (the ReLU mask is a_l > 0, which is also 0 outside [0, T), so the
//     reference's per-layer zero padding needs no extra test), the weight gradients of the tile's own
//     frames are accumulated right after each dz_l.  Nothing is saved between forward and backward.
//   Workgroup s of a backward launch owns tiles s, s + S, s + 2S, ... (S = slab count, a function of
//   (B, T) and the width only) and sums their parameter gradients, in tile order, into slab s of the
//   workspace: the first tile writes the slab, the next ones add to it, each element always by the
//   same thread.
// b2h_train_reduce -- sums the S slabs element by element in a fixed order (launch-boundary reduce: no
//   float atomics, no last-arriver handoff) and scatters the sums into the eight gradient tensors.
//
// Thread mapping of the convolutions: lane = frame row, wave = a group of kTrainGroup output channels, so every
// weight address is wave-uniform (scalar loads) and the activations come from LDS rows of odd stride
// (conflict-free).  The tiles are sized so that every layer's rows fit one 64-lane chunk.
#pragma once
#include "b2h_common.h"

namespace b2h {

constexpr int kTrainFwdTile = 52, kTrainFwdHalo = 8;  // 68 LDS rows; layer rows 64, 60, 56, 52
constexpr int kTrainBwdTile = 40, kTrainBwdHalo = 12; // 64 LDS rows; layer rows 60, 56, 52; dz 52, 48, 44
constexpr int kTrainMaxSlabs = 2048;
constexpr int kTrainGroup = 4; // output channels per wave and pass of a convolution (8 exceeds the SGPR budget)

struct TrainParams {
    const float* w[4];
    const float* b[4];
    int C, cin0, pos_emb;
    int xs, as, gs;   // LDS row strides (odd) of the input, hidden and dL/dy buffers
    int off[8];       // offset of each parameter's gradient inside a slab (floats, state_dict order)
    int slab;         // floats per slab (multiple of 4)
};

struct TrainGrads {
    float* g[8];
    int64_t off[9];   // off[8] = total floats
};

__host__ __device__ constexpr int train_tile(int mode) { return mode == 0 ? kTrainFwdTile : kTrainBwdTile; }
__host__ __device__ constexpr int train_halo(int mode) { return mode == 0 ? kTrainFwdHalo : kTrainBwdHalo; }
__host__ __device__ constexpr int train_rows(int mode) { return train_tile(mode) + 2 * train_halo(mode); }

__device__ inline int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// out[r][o] = b[o] + sum_{i,k} in[r+k-2][i] * w[o][i][k] for LDS rows r in [r0, r1) (r1 - r0 <= 64).
// HEAD = false: ReLU, 0 outside [0, T), into LDS.  HEAD = true: layer 4 into y rows of frames < T.
template <bool HEAD>
__device__ inline void train_conv(const float* in, int is, int cin, float* out, int os, int cout,
                                  const float* __restrict__ w, const float* __restrict__ bias, int r0, int r1,
                                  int tbase, int T, float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int ng = (cout + kTrainGroup - 1) / kTrainGroup;
    const int r = r0 + lane;
    const bool live = r < r1;
    const int rr = live ? r : r0;
    for (int g = wave_id(); g < ng; g += 4) {
        const int last = cout - 1 - g * kTrainGroup; // channels past cout read the last one (in bounds), dropped below
        const float* wg = w + (size_t)g * kTrainGroup * cin * kTaps;
        float acc[kTrainGroup];
#pragma unroll
        for (int j = 0; j < kTrainGroup; ++j) acc[j] = bias[g * kTrainGroup + min(j, last)];
        const float* arow = in + (rr - kPad) * is;
        for (int i = 0; i < cin; ++i) {
#pragma unroll 1 // kTrainGroup weights in flight, not 5x (SGPR budget)
            for (int k = 0; k < kTaps; ++k) {
                const float a = arow[k * is + i];
#pragma unroll
                for (int j = 0; j < kTrainGroup; ++j) acc[j] = fmaf(a, wg[(min(j, last) * cin + i) * kTaps + k], acc[j]);
            }
        }
        if (!live) continue;
        const int t = tbase + r;
        const bool inside = t >= 0 && t < T;
        if constexpr (HEAD) {
            if (inside)
#pragma unroll
                for (int j = 0; j < kTrainGroup; ++j)
                    if (g * kTrainGroup + j < cout) y[(int64_t)t * kOutCh + g * kTrainGroup + j] = acc[j];
        } else {
#pragma unroll
            for (int j = 0; j < kTrainGroup; ++j)
                if (g * kTrainGroup + j < cout) out[r * os + g * kTrainGroup + j] = inside ? fmaxf(acc[j], 0.f) : 0.f;
        }
    }
}

// Transposed convolution: d[r][i] = sum_{o,k} dz[r-k+2][o] * w[o][i][k], rows r in [r0, r1).
// dx == nullptr: dz_prev in place, a[r][i] = a[r][i] > 0 ? d : 0 (a holds the activation).
// else        : dL/dx rows of frames in [0, T) into dx (B-row base), channel i - c0 (the pos_emb
//             channel 0 gets no gradient).
__device__ inline void train_convT(const float* dz, int zs, int cout, float* a, int as, int cin,
                                   const float* __restrict__ w, int r0, int r1, int tbase, int T, int c0,
                                   float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int ng = (cin + kTrainGroup - 1) / kTrainGroup;
    const int r = r0 + lane;
    const bool live = r < r1;
    const int rr = live ? r : r0;
    for (int g = wave_id(); g < ng; g += 4) {
        const int last = cin - 1 - g * kTrainGroup; // channels past cin read the last one (in bounds), dropped below
        float acc[kTrainGroup];
#pragma unroll
        for (int j = 0; j < kTrainGroup; ++j) acc[j] = 0.f;
        const float* zrow = dz + (rr + kPad) * zs; // tap k reads row r - k + 2
        const float* wg = w + (size_t)g * kTrainGroup * kTaps;
        for (int o = 0; o < cout; ++o) {
            const float* wo = wg + (size_t)o * cin * kTaps;
#pragma unroll 1 // kTrainGroup weights in flight, not 5x (SGPR budget)
            for (int k = 0; k < kTaps; ++k) {
                const float z = zrow[-k * zs + o];
#pragma unroll
                for (int j = 0; j < kTrainGroup; ++j) acc[j] = fmaf(z, wo[min(j, last) * kTaps + k], acc[j]);
            }
        }
        if (!live) continue;
        const int t = tbase + r;
        if (dx) {
            if (t >= 0 && t < T)
#pragma unroll
                for (int j = 0; j < kTrainGroup; ++j) {
                    const int i = g * kTrainGroup + j;
                    if (i >= c0 && i < cin) dx[(int64_t)t * kInCh + i - c0] = acc[j];
                }
        } else {
#pragma unroll
            for (int j = 0; j < kTrainGroup; ++j) {
                const int i = g * kTrainGroup + j;
                if (i < cin) a[r * as + i] = a[r * as + i] > 0.f ? acc[j] : 0.f;
            }
        }
    }
}

// Parameter gradients of one layer over the tile's own frames, LDS rows [rlo, rlo + n):
//   gw[o][i][k] (+)= sum_r dz[r][o] * a[r+k-2][i],   gb[o] (+)= sum_r dz[r][o]
// in ascending row order.  Blocks of 2 out x 2 in channels x 5 taps per thread, a 5-row window of `a`
// slides in registers.  `first`: the slab's first tile writes instead of adding.
__device__ inline void train_wgrad(const float* dz, int zs, int cout, const float* a, int as, int cin, int rlo,
                                   int n, float* __restrict__ gw, float* __restrict__ gb, bool first) {
    const int no = (cout + 1) / 2, ni = (cin + 1) / 2;
    for (int blk = threadIdx.x; blk < no * ni; blk += 256) {
        const int o0 = 2 * (blk / ni), i0 = 2 * (blk % ni);
        const int o1 = min(o0 + 1, cout - 1), i1 = min(i0 + 1, cin - 1);
        float acc[2][2][kTaps];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int k = 0; k < kTaps; ++k) acc[u][v][k] = 0.f;
        float w0[kTaps], w1[kTaps];
#pragma unroll
        for (int k = 0; k < kTaps - 1; ++k) {
            w0[k] = a[(rlo - kPad + k) * as + i0];
            w1[k] = a[(rlo - kPad + k) * as + i1];
        }
        for (int r = rlo; r < rlo + n; ++r) {
            w0[kTaps - 1] = a[(r + kPad) * as + i0];
            w1[kTaps - 1] = a[(r + kPad) * as + i1];
            const float z0 = dz[r * zs + o0], z1 = dz[r * zs + o1];
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                acc[0][0][k] = fmaf(z0, w0[k], acc[0][0][k]);
                acc[0][1][k] = fmaf(z0, w1[k], acc[0][1][k]);
                acc[1][0][k] = fmaf(z1, w0[k], acc[1][0][k]);
                acc[1][1][k] = fmaf(z1, w1[k], acc[1][1][k]);
            }
#pragma unroll
            for (int k = 0; k < kTaps - 1; ++k) {
                w0[k] = w0[k + 1];
                w1[k] = w1[k + 1];
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const int o = o0 + u, i = i0 + v;
                if (o >= cout || i >= cin) continue;
                float* dst = gw + ((size_t)o * cin + i) * kTaps;
#pragma unroll
                for (int k = 0; k < kTaps; ++k) dst[k] = first ? acc[u][v][k] : dst[k] + acc[u][v][k];
            }
    }
    for (int o = threadIdx.x; o < cout; o += 256) {
        float s = 0.f;
        for (int r = rlo; r < rlo + n; ++r) s += dz[r * zs + o];
        gb[o] = first ? s : gb[o] + s;
    }
}

// MODE 0: y = ConvModel(x); grid = B * tiles, one tile per workgroup.
// MODE 1 / 2: parameter gradients into `slabs` (and dx for MODE 2); grid = nslabs, workgroup s owns
// tiles s, s + nslabs, ...  `out` = y (MODE 0) or dx (MODE 2).
template <int MODE>
__global__ __launch_bounds__(256) void b2h_train_conv(const float* __restrict__ x, const float* __restrict__ dy,
                                                      float* __restrict__ out, float* __restrict__ slabs,
                                                      TrainParams p, int T, int tiles_per_seq, int64_t ntiles,
                                                      int nslabs) {
    constexpr int F = train_tile(MODE), H = train_halo(MODE), R = train_rows(MODE);
    extern __shared__ __attribute__((aligned(16))) float smem_train[];
    const int C = p.C, cin0 = p.cin0, c0 = p.pos_emb ? 1 : 0;
    const int xs = p.xs, as = p.as, gs = p.gs;
    float* X = smem_train;
    float* A1 = X + R * xs;
    float* A2 = A1 + R * as;
    float* A3 = A2 + R * as;
    float* G = A3 + R * as;
    const int tid = threadIdx.x;
    const int64_t stride = MODE == 0 ? (int64_t)gridDim.x : (int64_t)nslabs;
    float* slab = MODE == 0 ? nullptr : slabs + (int64_t)blockIdx.x * p.slab;
    bool first = true;

    for (int64_t q = blockIdx.x; q < ntiles; q += stride) {
        const int64_t b = q / tiles_per_seq;
        const int t0 = (int)(q % tiles_per_seq) * F;
        const int tbase = t0 - H;
        const int n = min(F, T - t0); // frames of the tile inside the sequence (>= 1)
        const float* xb = x + b * (int64_t)T * kInCh;

        __syncthreads(); // the previous tile is done with LDS
        for (int i = tid; i < R * (kInCh / 4); i += 256) {
            const int r = i / (kInCh / 4), c4 = i % (kInCh / 4);
            const int t = tbase + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t >= 0 && t < T) v = *reinterpret_cast<const float4*>(xb + (int64_t)t * kInCh + c4 * 4);
            float* dst = X + r * xs + c0 + c4 * 4;
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
        if (p.pos_emb) // channel 0 = t/100 (HandPoseModels.py:71-75), zero outside the sequence
            for (int r = tid; r < R; r += 256) {
                const int t = tbase + r;
                X[r * xs] = (t >= 0 && t < T) ? (float)t / 100.0f : 0.f;
            }
        __syncthreads();
#pragma unroll 1 // layers 1-3, one copy of the loop body (SGPR budget)
        for (int l = 0; l < 3; ++l) {
            const float* in = l == 0 ? X : (l == 1 ? A1 : A2);
            float* o = l == 0 ? A1 : (l == 1 ? A2 : A3);
            train_conv<false>(in, l == 0 ? xs : as, l == 0 ? cin0 : C, o, as, C, p.w[l], p.b[l], 2 * l + 2,
                                         R - 2 * l - 2, tbase, T, nullptr);
            __syncthreads();
        }
        if constexpr (MODE == 0) {
            train_conv<true>(A3, as, C, nullptr, 0, kOutCh, p.w[3], p.b[3], H, H + n, tbase, T,
                             out + b * (int64_t)T * kOutCh);
        } else {
            // dL/dy rows [H - 8, H + F + 8), zero outside [0, T)
            const float* dyb = dy + b * (int64_t)T * kOutCh;
            for (int i = tid; i < (F + 16) * (kOutCh / 2); i += 256) {
                const int r = H - 8 + i / (kOutCh / 2), c2 = i % (kOutCh / 2);
                const int t = tbase + r;
                float2 v = make_float2(0.f, 0.f);
                if (t >= 0 && t < T) v = *reinterpret_cast<const float2*>(dyb + (int64_t)t * kOutCh + c2 * 2);
                G[r * gs + 2 * c2] = v.x;
                G[r * gs + 2 * c2 + 1] = v.y;
            }
            __syncthreads();
            // layer l: its weight gradients from dz_l and a_{l-1}, then dz_{l-1} in place of a_{l-1}.  One loop,
            // not four inlined copies: keeps the kernel within its SGPR budget.
#pragma unroll 1
            for (int l = 3; l >= 0; --l) {
                const float* dz = l == 3 ? G : (l == 2 ? A3 : (l == 1 ? A2 : A1));
                float* a = l == 3 ? A3 : (l == 2 ? A2 : (l == 1 ? A1 : X));
                const int zs = l == 3 ? gs : as, co = l == 3 ? kOutCh : C;
                const int ss = l == 0 ? xs : as, ci = l == 0 ? cin0 : C;
                train_wgrad(dz, zs, co, a, ss, ci, H, n, slab + p.off[2 * l], slab + p.off[2 * l + 1], first);
                if (l == 0 && MODE == 1) break;
                __syncthreads();
                // l > 0: dz_{l-1} over the rows layer l-1's gradients need; l == 0: dL/dx of the tile's own frames
                train_convT(dz, zs, co, a, ss, ci, p.w[l], H - 2 * l, H + F + 2 * l, tbase, T, c0,
                            l == 0 ? out + b * (int64_t)T * kInCh : nullptr);
                __syncthreads();
            }
        }
        first = false;
    }
}

// grads[e] = sum_{s < nslabs} slabs[s][e].  A workgroup covers 64 consecutive elements; wave w sums the
// w-th quarter of the slabs in ascending order, the four partial sums are added in wave order.
__global__ __launch_bounds__(256) void b2h_train_reduce(const float* __restrict__ slabs, int64_t slab, int nslabs,
                                                        TrainGrads g) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 64 + lane;
    const int per = (nslabs + 3) / 4;
    const int s0 = min(w * per, nslabs), s1 = min(s0 + per, nslabs);
    float s = 0.f;
    if (e < g.off[8])
        for (int k = s0; k < s1; ++k) s += slabs[(int64_t)k * slab + e];
    part[w][lane] = s;
    __syncthreads();
    if (w != 0 || e >= g.off[8]) return;
    const float v = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    int j = 7;
    while (e < g.off[j]) --j;
    g.g[j][e - g.off[j]] = v;
}

// dL/dpred of maskedPoseL1 (steps/utils.py:413-428; WEIGHTED = poderatedPoseL1, :431-452), with
// g = dL/dloss read from device memory:
//   plain   : dpred[i, t < n_i] = (g / B) * sign(p - t) / (n_i * 42)
//   weighted: dpred[i, t < n_i] = g * sign(p*s - t*s) / (n_i * 42) * s   (no /B: the class sums)
// frames t >= n_i (n_i clamped to [0, T] as slicing does) get 0.  sign(0) = 0 as in torch.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void b2h_l1_backward_kernel(const float* __restrict__ pred,
                                                              const float* __restrict__ target,
                                                              const float* __restrict__ scores,
                                                              const int64_t* __restrict__ n_frames,
                                                              const float* __restrict__ dloss,
                                                              float* __restrict__ dpred, int64_t B, int T,
                                                              int nch) { // nch = 2 x joints per frame
    const float g = WEIGHTED ? dloss[0] : dloss[0] / (float)B;
    const int64_t total = B * (int64_t)T * (nch / 2); // one (frame, joint) per step
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bt = e / (nch / 2);
        const int64_t b = bt / T;
        const int t = (int)(bt % T);
        int64_t nf = n_frames ? n_frames[b] : T;
        nf = nf < 0 ? 0 : (nf > T ? T : nf);
        float2 d = make_float2(0.f, 0.f);
        if (t < nf) {
            const float2 p = reinterpret_cast<const float2*>(pred)[e];
            const float2 q = reinterpret_cast<const float2*>(target)[e];
            const float cnt = (float)(nf * nch);
            auto sgn = [](float v) { return (float)((v > 0.f) - (v < 0.f)); };
            if constexpr (WEIGHTED) {
                const float s = scores[e];
                d.x = sgn(__fmul_rn(p.x, s) - __fmul_rn(q.x, s)) * g / cnt * s;
                d.y = sgn(__fmul_rn(p.y, s) - __fmul_rn(q.y, s)) * g / cnt * s;
            } else {
                d.x = sgn(p.x - q.x) * g / cnt;
                d.y = sgn(p.y - q.y) * g / cnt;
            }
        }
        reinterpret_cast<float2*>(dpred)[e] = d;
    }
}

} // namespace b2h
