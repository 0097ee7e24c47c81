// The Linear trio of kernel_tenc_train.h on the matrix cores: b2h_ml_linear, b2h_ml_linear_dx and b2h_ml_linear_dw are
// drop-in counterparts of b2h_tt_linear, b2h_tt_linear_dx and b2h_tt_linear_dw -- the same arguments, the same order
// of the epilogue operations, the same shape ranges (any K <= 128; any M for the forward and dw, M <= 384 for dx), the
// same slab contract for dw (S = tt_nslabs(N) workgroup columns, slab s owns the 64-row tiles s, s + S, ... in
// ascending order and writes [dW (M, K) | db (M)]), so b2h_tt_reduce, the slab scratch and b2h_tpt_train_bytes do not
// know which trio ran.  b2h_tpt_set_train_linear selects them.
//
// All products run on v_mfma_f32_16x16x4_f32 in exact fp32.  A k-step adds its four products in ascending k (the
// lane groups q = lane / 16 = 0 .. 3), so with lane group q holding index 4 s + q in k-step s an output element is
// the VALU kernels' chain: the forward starts at bias[m] and adds k ascending, dx starts at 0 and adds m ascending,
// dw starts at 0 and adds the rows of the slab's tiles ascending, db is the same walk against a fragment of ones.
//
//   b2h_ml_linear      Y^T tile = W X^T.  A wave owns 16 rows as the COLUMNS of its products: their X values are B
//                      fragments in registers for the whole kernel (32 VGPRs at K = 128), the weights are staged once
//                      per workgroup and column block of <= 128 output features in LDS (pitch 132: the 16 rows x 4
//                      k of an A fragment fall into 64 different banks).  A lane ends with 4 consecutive output
//                      features of one row: the epilogue is a 4-byte mask load and a 16-byte residual load, both
//                      requested before the tile's MFMAs, and a 16-byte store (dword accesses when M is no multiple
//                      of 4: nout = 42).
//   b2h_ml_linear_dx   dX^T tile = W^T dY^T, the same ownership.  W is walked in row blocks of <= 128 (pitch 144,
//                      since here the k index walks LDS rows); the dY values are the B fragments, requested 16 summed
//                      indices ahead; the eight accumulators of the 128 input features live across the blocks.
//   b2h_ml_linear_dw   grid (S, ceil(M / 32)) as b2h_tt_linear_dw.  Per 64-row tile the dY columns of the workgroup
//                      and the X rows are staged in LDS (the next tile is requested into registers before this tile's
//                      MFMAs); the rows are the k index.  Wave w owns the column tiles w and w + 4 of K for both 16-row
//                      output tiles; wave 0 also adds db.
//
// Padded rows.  Tiles run over whole 16s and the k-steps in groups of four (16 indices), and
// 0 x stale NaN is NaN, so everything summed over is a true zero past its range: X columns >= K are explicit zeros in
// the fragments and in LDS, W columns >= K and rows >= M are written as zeros into LDS (every word that can be read is
// written for every block), dY columns >= M are explicit zeros, rows >= N read 0 through a buffer descriptor over the
// workgroup's own rows.  Rows and columns past the end in the OUTPUT position are computed and dropped: rows by the
// store's descriptor, features by an explicit test (a feature past M would land in the next row).
//
// Determinism as in kernel_tenc_train.h: one owner lane per output element, no atomics, no handoff, and a row of y or
// dx is computed from that row alone.
#pragma once
#include "kernel_tenc_train.h"
#include "kernel_train_attn_mfma.h"

namespace b2h {

constexpr int kMlRows = 64;                  // rows per workgroup of b2h_ml_linear / _dx: 16 per wave
constexpr int kMlBlock = 128;                // weight rows staged at a time
constexpr int kMlWf = kTtD + 4;              // LDS pitch of W in the forward: A[i][k] = Ws[i][4 s + q]
constexpr int kMlWd = kTtD + 16;             // LDS pitch where the k index walks rows: dx's W, dw's X
constexpr int kMlYd = kTtDwM + 16;           // LDS pitch of dw's dY columns
constexpr size_t kMlFwdLds = (size_t)kMlBlock * kMlWf * 4;                  // 67 584 B
constexpr size_t kMlDxLds = (size_t)kMlBlock * kMlWd * 4;                   // 73 728 B
constexpr size_t kMlDwLds = (size_t)kTtDwRows * (kMlWd + kMlYd) * 4;        // 49 152 B

__device__ __forceinline__ float ml_load1(__amdgpu_buffer_rsrc_t rs, int float_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, float_off * 4, 0, 0));
}
__device__ __forceinline__ void ml_store1(__amdgpu_buffer_rsrc_t rs, int float_off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), rs, float_off * 4, 0, 0);
    asm volatile("s_nop 1" ::: "memory"); // as tt_store: keeps tools/store_war_audit.py at zero, no hardware need
}

// Four keep-mask bytes as one word.  The training calls state no alignment for their masks (bytes), so the word load
// is taken only where the address allows it (uniform: `p` is the mask's base plus a multiple of 4).
__device__ __forceinline__ uint32_t ml_mask4(const uint8_t* p) {
    if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// W rows r0 .. r0 + 127 -> LDS at `pitch` (a multiple of 4), all 128 columns: zeros for rows >= M and columns >= K.
// With K a multiple of 4 and W 16-byte aligned a thread moves 16 float4, all requested before the first is written:
// one memory latency per block; otherwise dwords, eight in flight.
__device__ __forceinline__ void ml_stage_w(float* Ws, int pitch, const float* __restrict__ W, int r0, int K, int M) {
    if (((K & 3) | (int)(reinterpret_cast<uintptr_t>(W) & 15)) == 0) { // (uniform)
        const int k = 4 * (threadIdx.x & 31);
#pragma unroll
        for (int i = 0; i < kMlBlock / 8; ++i) {
            const int r = (threadIdx.x >> 5) + 8 * i, m = r0 + r;
            *reinterpret_cast<f32x4*>(Ws + r * pitch + k) =
                (m < M && k < K) ? *reinterpret_cast<const f32x4*>(W + (size_t)m * K + k) : mt_zero4();
        }
        return;
    }
    const int k = threadIdx.x & (kTtD - 1);
#pragma unroll 8
    for (int r = threadIdx.x >> 7; r < kMlBlock; r += 2) {
        const int m = r0 + r;
        Ws[r * pitch + k] = (m < M && k < K) ? W[(size_t)m * K + k] : 0.f;
    }
}

// acc[u] += W rows (a0 + 16 u rows)[4 s + q] . xb[s] over the k-steps of K: two independent chains.  FULL: K = 128, no
// test between the groups, so the compiler may move the epilogue's loads over the whole chain.
template <bool FULL>
__device__ __forceinline__ void ml_fwd_pair(const float* a0, const float (&xb)[kTtD / 4], int K, f32x4 (&acc)[2]) {
#pragma unroll
    for (int g = 0; g < kTtD / 16; ++g)
        if (FULL || 16 * g < K) { // (uniform)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int s = 4 * g + j;
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[4 * s], xb[s], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[16 * kMlWf + 4 * s], xb[s], acc[1], 0, 0, 0);
            }
        }
}

// Y[n][m] = b[m] + sum_k X[n][k] W[m][k], then ReLU, keep-mask, + res: b2h_tt_linear.  grid ceil(N / 64), 256 threads,
// kMlFwdLds.
__global__ __launch_bounds__(256) void b2h_ml_linear(const float* __restrict__ X, const float* __restrict__ W,
                                                     const float* __restrict__ bias, float* __restrict__ Y,
                                                     int64_t N, int K, int M, int relu,
                                                     const uint8_t* __restrict__ mask, float scale,
                                                     const float* __restrict__ res) {
    extern __shared__ __attribute__((aligned(16))) float smem_ml[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * kMlRows;
    const int rows = (int)(N - n0 < kMlRows ? N - n0 : kMlRows);
    const int row = wave * 16 + col;
    const bool live = wave * 16 < rows; // wave-uniform: a wave past the end only stages
    const __amdgpu_buffer_rsrc_t xrs = make_rsrc(X + n0 * K, rows * K * 4);
    const __amdgpu_buffer_rsrc_t yrs = make_rsrc(Y + n0 * M, rows * M * 4);
    float xb[kTtD / 4]; // B[k = 4 s + q][col] of k-step s; rows past the end lie outside xrs and read 0
#pragma unroll
    for (int s = 0; s < kTtD / 4; ++s) xb[s] = 4 * s + q < K ? ml_load1(xrs, row * K + 4 * s + q) : 0.f;
    const int64_t e0 = (n0 + row) * M; // the row's first element of mask / res
    const bool vec = (M & 3) == 0;
    for (int mb = 0; mb < M; mb += kMlBlock) {
        if (mb) __syncthreads(); // the previous block is done with LDS
        ml_stage_w(smem_ml, kMlWf, W, mb, K, M);
        __syncthreads();
        if (!live) continue;
        const int left = min(kMlBlock, M - mb);
#pragma unroll 1
        for (int mt = 0; mt * 16 < left; mt += 2) { // two independent chains
            // the bias, and on the 16-byte path the mask and the residual, are requested before the MFMAs
            f32x4 acc[2], rs[2];
            uint32_t k4[2];
            bool put[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int m = mb + 16 * (mt + u) + 4 * q; // the lane's features m .. m + 3 of row `row`
                put[u] = row < rows && m < M;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[u][r] = m + r < M ? bias[m + r] : 0.f;
                k4[u] = vec && mask && put[u] ? ml_mask4(mask + e0 + m) : 0u;
                rs[u] = vec && res && put[u] ? *reinterpret_cast<const f32x4*>(res + e0 + m) : mt_zero4();
            }
            const float* a0 = smem_ml + (16 * mt + col) * kMlWf + q;
            if (K == kTtD)
                ml_fwd_pair<true>(a0, xb, K, acc);
            else
                ml_fwd_pair<false>(a0, xb, K, acc);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int m = mb + 16 * (mt + u) + 4 * q;
                if (!put[u]) continue;
                f32x4 v = acc[u];
                if (relu)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                if (vec) {
                    if (mask)
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = (k4[u] >> (8 * r)) & 0xff ? v[r] * scale : 0.f;
                    if (res) v += rs[u];
                    buf_store4(yrs, row * M + m, v);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (m + r >= M) break;
                        float o = v[r];
                        if (mask) o = mask[e0 + m + r] ? o * scale : 0.f;
                        if (res) o += res[e0 + m + r];
                        ml_store1(yrs, row * M + m + r, o);
                    }
                }
            }
        }
    }
}

// dX[n][k] = sum_m dY[n][m] W[m][k], then gate, keep-mask, + add: b2h_tt_linear_dx.  grid ceil(N / 64), 256 threads,
// kMlDxLds.  All eight column tiles are computed whatever K is (W's columns >= K are zeros; the store drops them).
__global__ __launch_bounds__(256) void b2h_ml_linear_dx(const float* __restrict__ dY, const float* __restrict__ W,
                                                        float* __restrict__ dX, int64_t N, int K, int M,
                                                        const float* __restrict__ gate,
                                                        const uint8_t* __restrict__ mask, float scale,
                                                        const float* __restrict__ add) {
    extern __shared__ __attribute__((aligned(16))) float smem_ml[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * kMlRows;
    const int rows = (int)(N - n0 < kMlRows ? N - n0 : kMlRows);
    const int row = wave * 16 + col;
    const bool live = wave * 16 < rows;
    const __amdgpu_buffer_rsrc_t grs = make_rsrc(dY + n0 * M, rows * M * 4);
    const __amdgpu_buffer_rsrc_t ors = make_rsrc(dX + n0 * K, rows * K * 4);
    f32x4 acc[kTtD / 16]; // D rows 16 kt + 4 q + r = input features of row `row`
#pragma unroll
    for (int kt = 0; kt < kTtD / 16; ++kt) acc[kt] = mt_zero4();
    for (int mb = 0; mb < M; mb += kMlBlock) {
        if (mb) __syncthreads();
        ml_stage_w(smem_ml, kMlWd, W, mb, K, M);
        __syncthreads();
        if (!live) continue;
        const int left = min(kMlBlock, M - mb);
        // B[m = mb + 4 s + q][col] of k-step s: zeros behind column M, and past the last row (outside grs); the next
        // 16 indices are requested before this group's MFMAs
        const auto fetch = [&](int g, float (&y)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int m = mb + 16 * g + 4 * j + q;
                y[j] = m < M ? ml_load1(grs, row * M + m) : 0.f;
            }
        };
        float yn[4];
        fetch(0, yn);
#pragma unroll 1
        for (int g = 0; 16 * g < left; ++g) {
            const float y[4] = {yn[0], yn[1], yn[2], yn[3]};
            if (16 * (g + 1) < left) fetch(g + 1, yn);
            const float* a = smem_ml + (16 * g + q) * kMlWd + col;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int kt = 0; kt < kTtD / 16; ++kt)
                    acc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * j * kMlWd + 16 * kt], y[j], acc[kt], 0, 0, 0);
        }
    }
    if (!live || row >= rows) return;
    const int64_t e0 = (n0 + row) * K;
    const bool vec = (K & 3) == 0;
#pragma unroll
    for (int kt = 0; kt < kTtD / 16; ++kt) {
        const int k = 16 * kt + 4 * q;
        if (k >= K) continue;
        f32x4 v = acc[kt];
        if (vec) {
            if (gate) {
                const f32x4 g4 = *reinterpret_cast<const f32x4*>(gate + e0 + k);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = g4[r] > 0.f ? v[r] * scale : 0.f;
            }
            if (mask) {
                const uint32_t k4 = ml_mask4(mask + e0 + k);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (k4 >> (8 * r)) & 0xff ? v[r] * scale : 0.f;
            }
            if (add) v += *reinterpret_cast<const f32x4*>(add + e0 + k);
            buf_store4(ors, row * K + k, v);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (k + r >= K) break;
                float o = v[r];
                if (gate) o = gate[e0 + k + r] > 0.f ? o * scale : 0.f;
                if (mask) o = mask[e0 + k + r] ? o * scale : 0.f;
                if (add) o += add[e0 + k + r];
                ml_store1(ors, row * K + k + r, o);
            }
        }
    }
}

// Slab partials of dW[m][k] = sum_n dY[n][m] X[n][k] and db[m] = sum_n dY[n][m]: b2h_tt_linear_dw.
// grid (S, ceil(M / 32)), 256 threads, kMlDwLds.
__global__ __launch_bounds__(256) void b2h_ml_linear_dw(const float* __restrict__ dY, const float* __restrict__ X,
                                                        float* __restrict__ slabs, int64_t slab, int64_t N, int K,
                                                        int M) {
    extern __shared__ __attribute__((aligned(16))) float smem_ml[];
    float* Xs = smem_ml;
    float* Ys = smem_ml + kTtDwRows * kMlWd;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const int m0 = blockIdx.y * kTtDwM;
    const int xk = threadIdx.x & (kTtD - 1), xr = threadIdx.x >> 7; // X: column xk of the rows xr + 2 i
    const int ym = m0 + (threadIdx.x & (kTtDwM - 1)), yr = threadIdx.x >> 5; // dY: column ym of the rows yr + 8 i
    float nx[kTtDwRows / 2], ny[kTtDwRows / 8];
    // rows n0 .. n0 + 63 -> registers: zeros behind column K / M, and past row N (outside the descriptors)
    auto fetch = [&](int64_t n0) {
        const int rows = (int)(N - n0 < kTtDwRows ? N - n0 : kTtDwRows);
        const __amdgpu_buffer_rsrc_t xrs = make_rsrc(X + n0 * K, rows * K * 4);
        const __amdgpu_buffer_rsrc_t grs = make_rsrc(dY + n0 * M, rows * M * 4);
#pragma unroll
        for (int i = 0; i < kTtDwRows / 2; ++i) nx[i] = xk < K ? ml_load1(xrs, (xr + 2 * i) * K + xk) : 0.f;
#pragma unroll
        for (int i = 0; i < kTtDwRows / 8; ++i) ny[i] = ym < M ? ml_load1(grs, (yr + 8 * i) * M + ym) : 0.f;
    };
    f32x4 acc[2][2], accb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        accb[u] = mt_zero4();
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = mt_zero4();
    }
    const bool two = m0 + 16 < M; // (uniform) the second 16-row output tile has a valid row
    const int64_t ntiles = (N + kTtDwRows - 1) / kTtDwRows;
    if ((int64_t)blockIdx.x < ntiles) fetch((int64_t)blockIdx.x * kTtDwRows);
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        __syncthreads(); // the previous tile is done with LDS
#pragma unroll
        for (int i = 0; i < kTtDwRows / 2; ++i) Xs[(xr + 2 * i) * kMlWd + xk] = nx[i];
#pragma unroll
        for (int i = 0; i < kTtDwRows / 8; ++i) Ys[(yr + 8 * i) * kMlYd + (threadIdx.x & (kTtDwM - 1))] = ny[i];
        __syncthreads();
        if (t + gridDim.x < ntiles) fetch((t + gridDim.x) * kTtDwRows);
        if (16 * wave >= K) continue; // (uniform) no column tile of this wave has a valid column
        const bool kt1 = 16 * (wave + 4) < K;
#pragma unroll 4
        for (int s = 0; s < kTtDwRows / 4; ++s) { // the rows 4 s + q are the k index: ascending
            const float* xs = Xs + (4 * s + q) * kMlWd + 16 * wave + col;
            const float* ys = Ys + (4 * s + q) * kMlYd + col;
            const float b0 = xs[0], b1 = xs[64], a0 = ys[0], a1 = ys[16];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            if (two) acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            if (kt1) {
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
                if (two) acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
            }
            if (wave == 0) { // db: fmaf(y, 1, acc) is acc + y
                accb[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, 1.f, accb[0], 0, 0, 0);
                if (two) accb[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, 1.f, accb[1], 0, 0, 0);
            }
        }
    }
    // D rows 4 q + r = output rows m0 + 16 u + 4 q + r, column col of the column tile
    const __amdgpu_buffer_rsrc_t ors = make_rsrc(slabs + (int64_t)blockIdx.x * slab, (M * K + M) * 4);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * u + 4 * q + r;
            if (m >= M) continue;
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const int k = 16 * (wave + 4 * v) + col;
                if (k < K) ml_store1(ors, m * K + k, acc[u][v][r]);
            }
            if (wave == 0 && col == 0) ml_store1(ors, M * K + m, accb[u][r]);
        }
}

} // namespace b2h
