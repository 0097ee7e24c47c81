// The whole-matrix training attention of kernel_train_attn.h on the matrix cores: b2h_mw_sdpa and b2h_mw_sdpa_bwd are
// drop-in counterparts of b2h_tt_sdpa and b2h_tt_sdpa_bwd -- the same arguments (AttnSrc operands, a uint8 keep-mask
// (B, 4, Tq, Tk) or NULL, `scale` = 1 / (1 - p), O or dO (B*Tq, 128), LtGradDst), the same range 1 <= Tq, Tk <= 128,
// the same grid of one workgroup of 256 threads per (sequence, head), no LSE and no buffer besides the operands: the
// backward recomputes the softmax from Q and K.  b2h_tenc_set_train_kernel selects them.
//
// All six products run on v_mfma_f32_16x16x4_f32, whose result is a k-ordered fmaf chain in exact fp32.  Lane group
// q = lane / 16 holds the summed index 4 s + q in k-step s, so every output element is accumulated from 0 over its
// summed index ascending, one accumulator per element: the chains of b2h_tt_sdpa.  The row softmax (the wave
// reductions of tt_softmax_rows: a lane holds the keys lane and lane + 64), the mask, scale and
// dZ = S o (dSd - rowsum(dSd o S)) stay on the vector ALU.  The forward is bit-equal to b2h_tt_sdpa, and so are dV
// and dP; the backward's rowsum is formed from the accumulators (a lane adds its 32 keys in ascending order, then the
// row's four lanes are added), not by tt_wave_sum over keys lane and lane + 64, because LDS has no room for dP beside
// S: dQ and dK are exact fp32 in another order, not bit-equal.
//
// A wave owns 16-row tiles as the COLUMNS of its products, the tiles w and w + 4 together so that an A operand read
// from LDS feeds two chains:
//
//   query owner   columns = 16 queries.  S^T = K Q^T and dP^T = V dO^T (A = the key rows from LDS, B = the queries' Q
//                 or dO values, eight registers per tile, read through a descriptor); the S tile row goes to LDS, its
//                 16 rows are normalised by the same wave, and O^T = V^T Pd^T, dQ^T = K^T dZ^T follow with
//                 B = P[query][4 s + q] from LDS.  Nothing of this needs a barrier: the rows of P are the wave's own.
//   key owner     columns = 16 keys.  dV^T = dO^T Pd and dK^T = Q^T dZ: A = a column of the dO / Q rows,
//                 B = P[4 s + q][key], both from LDS.  Pd is formed from S and the mask bytes on the way.
//
// LDS: K, V (and Q, dO in the backward) rows at pitch kMwRow = 34, the (Tq, Tk) matrix at pitch mw_ps(Tk) = 18 mod 32,
// the backward's mask bytes; everything over the sizes rounded up to 16.  128 x 128: 109 568 B forward, 160 768 B
// backward; 100 x 100: 81 536 B (two workgroups per CU) and 122 000 B.  With 32 banks per half wave an operand read
// of the form [16 rows][k = q] is conflict-free at a pitch of 2 mod 32 and at 18 mod 32, one of the form
// [k = q][16 columns] at 18 mod 32; at 2 mod 32 the latter is two-way.
//
// Padded rows (DESIGN.md sections 17 and 19).  Tiles run over whole 16s and k-steps of 4 and 0 x stale NaN is NaN, so
// what is summed over is a true zero past Tq and Tk: rows are staged through a descriptor over the sequence's own
// rows, all rows up to the next multiple of 16; every tile of P with a valid row and a valid column is written whole;
// scores of keys >= Tk are -inf before the maximum; P and dZ are written as 0 for keys in [Tk, 16 ceil(Tk / 16)) and
// for queries in [Tq, 16 ceil(Tq / 16)); the mask is read inside [0, Tq) x [0, Tk) only; stores go through descriptors
// over the sequence's rows, which drop rows past the end.
//
// Determinism: a function of (Tq, Tk) and the sequence's key length alone.  No atomics, nothing read from another sequence.
#pragma once
#include "kernel_train_attn.h"
#include "kernel_train_linear_mfma.h" // ml_load1, mt_zero4

namespace b2h {

constexpr int kMwRow = kTtHd + 2; // LDS pitch of the Q, dO, K, V rows

__host__ __device__ inline int mw_pad(int T) { return (T + 15) & ~15; }
__host__ __device__ inline int mw_ps(int Tk) { return mw_pad(Tk) + ((mw_pad(Tk) & 16) ? 2 : 18); } // pitch of P: 18 mod 32
__host__ __device__ inline size_t mw_sdpa_lds_bytes(int Tq, int Tk, bool bwd) {
    return (size_t)4 * (((bwd ? 2 : 0) * mw_pad(Tq) + 2 * mw_pad(Tk)) * kMwRow + mw_pad(Tq) * mw_ps(Tk)) +
           (bwd ? (size_t)(Tq * Tk + 3) / 4 * 4 : 0);
}

// The rows 0 .. mw_pad(n) - 1 of one head (32 floats from float offset `off` of rows of ld floats) -> LDS at kMwRow.
// rs ends behind row n - 1, so the rows from n on are written as zeros.
__device__ __forceinline__ void mw_stage(__amdgpu_buffer_rsrc_t rs, int ld, int off, float* dst, int n) {
    const int c = 4 * (threadIdx.x & 7);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int i = (threadIdx.x >> 3) + 32 * it;
        if (i < mw_pad(n)) { // (uniform per wave: 8 rows of a wave lie in one 16-row tile)
            const f32x4 v = buf_load4(rs, i * ld + off + c);
            f32x2* p = reinterpret_cast<f32x2*>(dst + i * kMwRow + c);
            p[0] = f32x2{v[0], v[1]};
            p[1] = f32x2{v[2], v[3]};
        }
    }
}

// The B operand of a wave's column tile for a product summed over d: f[s] = element d = 4 s + q of the lane's row,
// `off` = the float offset of the row's element q; a row past the descriptor's end reads 0.
__device__ __forceinline__ void mw_frag(__amdgpu_buffer_rsrc_t rs, int off, float (&f)[kTtHd / 4]) {
#pragma unroll
    for (int s = 0; s < kTtHd / 4; ++s) f[s] = ml_load1(rs, off + 4 * s);
}

// For the row tiles kt < nkt of X (LDS, pitch kMwRow): sink(kt, c0, c1) with c_u[r] = X[16 kt + 4 q + r] . (the row
// behind f_u), summed over d ascending.  `two`: (uniform) the wave has a second column tile.
template <typename Sink>
__device__ __forceinline__ void mw_rows_dot(const float* X, int nkt, const float (&f0)[kTtHd / 4],
                                            const float (&f1)[kTtHd / 4], bool two, Sink&& sink) {
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
#pragma unroll
    for (int kt = 0; kt < kAttnMaxTiles; ++kt) {
        if (kt < nkt) { // (uniform)
            const float* a = X + (16 * kt + col) * kMwRow + q;
            f32x4 c0 = mt_zero4(), c1 = mt_zero4();
#pragma unroll
            for (int s = 0; s < kTtHd / 4; ++s) {
                const float av = a[4 * s];
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, f0[s], c0, 0, 0, 0);
                if (two) c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, f1[s], c1, 0, 0, 0);
            }
            sink(kt, c0, c1);
        }
    }
}

// The rows i0 .. i0 + 15 of P hold Q_i . K_j for j < mw_pad(Tk): replaced by drop(softmax_j(. / sqrt(32))), with the
// reductions of tt_softmax_rows (one wave per row, a lane holds the keys lane and lane + 64).  mk: the keep-mask
// (Tq, Tk) of this (sequence, head) or NULL.  Keys in [kl, mw_pad(Tk)) and rows >= Tq are written as 0: kl <= Tk is the
// sequence's key length (tt_key_len), the softmax runs over the keys below it.
__device__ __forceinline__ void mw_softmax_tile(float* P, int ps, int i0, int Tq, int Tk, int kl, const uint8_t* mk,
                                                float scale) {
    const int lane = threadIdx.x & 63, tkp = mw_pad(Tk);
    const bool in0 = lane < kl, in1 = lane + 64 < kl;
    for (int i = i0; i < i0 + 16; ++i) {
        float* row = P + i * ps;
        float p0 = 0.f, p1 = 0.f;
        if (i < Tq) { // (uniform)
            const float s0 = in0 ? row[lane] * kTtQkScale : -INFINITY, s1 = in1 ? row[lane + 64] * kTtQkScale : -INFINITY;
            const float mx = tt_wave_max(fmaxf(s0, s1));
            const float e0 = expf(s0 - mx), e1 = in1 ? expf(s1 - mx) : 0.f; // e0 = 0 past kl
            const float sum = tt_wave_sum((in0 ? e0 : 0.f) + e1);
            p0 = e0 / sum;
            p1 = e1 / sum;
            if (mk) {
                p0 = in0 && mk[i * Tk + lane] ? p0 * scale : 0.f;
                p1 = in1 && mk[i * Tk + lane + 64] ? p1 * scale : 0.f;
            }
        }
        if (lane < tkp) row[lane] = in0 ? p0 : 0.f;
        if (lane + 64 < tkp) row[lane + 64] = in1 ? p1 : 0.f;
    }
}

// out[u][mt][r] = sum_j X[j][16 mt + 4 q + r] P[i0_u + col][j], j ascending over 4 * nsteps columns of P: O^T from V
// and drop(P), dQ^T from K and dZ.
__device__ __forceinline__ void mw_acc_over_cols(const float* X, const float* P, int ps, const int (&i0)[2], bool two,
                                                 int nsteps, f32x4 (&out)[2][2]) {
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const float* x = X + q * kMwRow + col;
    const float* p0 = P + (i0[0] + col) * ps + q;
    const float* p1 = P + (i0[two ? 1 : 0] + col) * ps + q;
    float na0 = x[0], na1 = x[16], nb0 = p0[0], nb1 = p1[0];
    for (int s = 0; s < nsteps; ++s) {
        const float a0 = na0, a1 = na1, b0 = nb0, b1 = nb1;
        const int n = 4 * min(s + 1, nsteps - 1); // the next step's operands are read before this step's MFMAs
        na0 = x[n * kMwRow], na1 = x[n * kMwRow + 16], nb0 = p0[n], nb1 = p1[n];
        out[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, out[0][0], 0, 0, 0);
        out[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, out[0][1], 0, 0, 0);
        if (two) {
            out[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, out[1][0], 0, 0, 0);
            out[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, out[1][1], 0, 0, 0);
        }
    }
}

// out[u][mt][r] = sum_i X[i][16 mt + 4 q + r] W[i][j0_u + col], i ascending over 4 * nsteps rows of P: dK^T from Q and
// W = dZ (Mk NULL), dV^T from dO and W = drop(S), formed from S and the mask bytes Mk (Tq, Tk) in LDS.
__device__ __forceinline__ void mw_acc_over_rows(const float* X, const float* P, int ps, const int (&j0)[2], bool two,
                                                 int nsteps, const uint8_t* Mk, float scale, int Tq, int Tk,
                                                 f32x4 (&out)[2][2]) {
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const float* x = X + q * kMwRow + col;
    const int ja = j0[0] + col, jb = j0[two ? 1 : 0] + col;
    // operand (W[i][ja], W[i][jb]) of the k-step whose lane group q holds row i = 4 s + q
    const auto fetch = [&](int s, float& a0, float& a1, float& b0, float& b1) {
        const int i = 4 * s + q;
        a0 = x[4 * s * kMwRow], a1 = x[4 * s * kMwRow + 16];
        b0 = P[i * ps + ja], b1 = P[i * ps + jb];
        if (Mk) {
            b0 = i < Tq && ja < Tk && Mk[i * Tk + ja] ? b0 * scale : 0.f;
            b1 = i < Tq && jb < Tk && Mk[i * Tk + jb] ? b1 * scale : 0.f;
        }
    };
    float na0, na1, nb0, nb1;
    fetch(0, na0, na1, nb0, nb1);
    for (int s = 0; s < nsteps; ++s) {
        const float a0 = na0, a1 = na1, b0 = nb0, b1 = nb1;
        fetch(min(s + 1, nsteps - 1), na0, na1, nb0, nb1); // the next step's operands, before this step's MFMAs
        out[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, out[0][0], 0, 0, 0);
        out[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, out[0][1], 0, 0, 0);
        if (two) {
            out[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, out[1][0], 0, 0, 0);
            out[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, out[1][1], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ void mw_zero(f32x4 (&out)[2][2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) out[u][0] = out[u][1] = mt_zero4();
}

// out[u][mt] = the elements 16 mt + 4 q .. + 3 from float column c0 of the rows t0_u + col behind rs (ld floats per
// row); rows past the descriptor's end are dropped.
__device__ __forceinline__ void mw_store(__amdgpu_buffer_rsrc_t rs, int ld, int c0, const int (&t0)[2], bool two,
                                         const f32x4 (&out)[2][2]) {
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
#pragma unroll
    for (int u = 0; u < 2; ++u)
        if (u == 0 || two) {
            const int off = (t0[u] + col) * ld + c0 + 4 * q;
            buf_store4(rs, off, out[u][0]);
            buf_store4(rs, off + 16, out[u][1]);
        }
}

// S^T tiles of the wave's query tiles -> P, then their rows' softmax (and dropout, under mk)
__device__ __forceinline__ void mw_probs(const float* K, float* P, int ps, const int (&i0)[2], bool two,
                                         const float (&qf)[2][kTtHd / 4], int Tq, int Tk, int kl, const uint8_t* mk,
                                         float scale) {
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    mw_rows_dot(K, mw_pad(Tk) >> 4, qf[0], qf[1], two, [&](int kt, f32x4 c0, f32x4 c1) {
        // c_u[r] = S[i0_u + col][16 kt + 4 q + r]
        f32x2* d0 = reinterpret_cast<f32x2*>(P + (i0[0] + col) * ps + 16 * kt + 4 * q);
        d0[0] = f32x2{c0[0], c0[1]};
        d0[1] = f32x2{c0[2], c0[3]};
        if (two) {
            f32x2* d1 = reinterpret_cast<f32x2*>(P + (i0[1] + col) * ps + 16 * kt + 4 * q);
            d1[0] = f32x2{c1[0], c1[1]};
            d1[1] = f32x2{c1[2], c1[3]};
        }
    });
    __builtin_amdgcn_wave_barrier(); // the rows are read back across the wave's lanes (LDS serves a wave in order)
    mw_softmax_tile(P, ps, i0[0], Tq, Tk, kl, mk, scale);
    if (two) mw_softmax_tile(P, ps, i0[1], Tq, Tk, kl, mk, scale);
    __builtin_amdgcn_wave_barrier();
}

// O[i][32 h + d] = sum_j drop(P)[i][j] V[j][d]: b2h_tt_sdpa.  grid B * 4, 256 threads,
// mw_sdpa_lds_bytes(Tq, Tk, false) of dynamic LDS.  1 <= Tq, Tk <= 128.  klen: (B) key lengths or NULL (tt_key_len).
__global__ __launch_bounds__(256) void b2h_mw_sdpa(AttnSrc src, const uint8_t* __restrict__ mask, float scale,
                                                   float* __restrict__ O, int Tq, int Tk,
                                                   const int64_t* __restrict__ klen) {
    extern __shared__ __attribute__((aligned(16))) float smem_mw[];
    float* K = smem_mw;
    float* V = K + mw_pad(Tk) * kMwRow;
    float* P = V + mw_pad(Tk) * kMwRow;
    const int64_t b = blockIdx.x / kTtHeads;
    const int h = blockIdx.x % kTtHeads, ps = mw_ps(Tk);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(src.kv + b * Tk * src.ldkv, Tk * src.ldkv * 4);
    const __amdgpu_buffer_rsrc_t qrs = make_rsrc(src.q + b * Tq * src.ldq, Tq * src.ldq * 4);
    mw_stage(krs, src.ldkv, src.colk + h * kTtHd, K, Tk);
    mw_stage(krs, src.ldkv, src.colv + h * kTtHd, V, Tk);
    const int i0[2] = {16 * wave, 16 * (wave + 4)};
    const bool two = i0[1] < Tq;
    float qf[2][kTtHd / 4];
#pragma unroll
    for (int u = 0; u < 2; ++u) mw_frag(qrs, (i0[u] + col) * src.ldq + src.colq + h * kTtHd + q, qf[u]);
    __syncthreads();
    if (i0[0] >= Tq) return; // (uniform) no query tile for this wave; no barrier follows
    mw_probs(K, P, ps, i0, two, qf, Tq, Tk, tt_key_len(klen, b, Tk), mask ? mask + (int64_t)blockIdx.x * Tq * Tk : nullptr,
             scale);
    f32x4 o[2][2];
    mw_zero(o);
    mw_acc_over_cols(V, P, ps, i0, two, (Tk + 3) >> 2, o);
    mw_store(make_rsrc(O + b * Tq * kTtD, Tq * kTtD * 4), kTtD, h * kTtHd, i0, two, o);
}

// Backward of b2h_mw_sdpa for one (sequence, head): b2h_tt_sdpa_bwd.  grid B * 4, 256 threads,
// mw_sdpa_lds_bytes(Tq, Tk, true) of dynamic LDS: Q, dO, K, V, the (Tq, Tk) matrix (S, then dZ / sqrt(32)) and the
// mask bytes.  With klen the columns kl .. Tk - 1 of S and of dZ are +-0, so the rows kl .. Tk - 1 of dK and dV, sums
// from +0, are written as +0.
__global__ __launch_bounds__(256) void b2h_mw_sdpa_bwd(AttnSrc src, const float* __restrict__ dO,
                                                       const uint8_t* __restrict__ mask, float scale, LtGradDst dst,
                                                       int Tq, int Tk, const int64_t* __restrict__ klen) {
    extern __shared__ __attribute__((aligned(16))) float smem_mw[];
    float* Q = smem_mw;
    float* G = Q + mw_pad(Tq) * kMwRow;
    float* K = G + mw_pad(Tq) * kMwRow;
    float* V = K + mw_pad(Tk) * kMwRow;
    float* P = V + mw_pad(Tk) * kMwRow;
    const int64_t b = blockIdx.x / kTtHeads;
    const int h = blockIdx.x % kTtHeads, ps = mw_ps(Tk);
    uint8_t* Mk = mask ? reinterpret_cast<uint8_t*>(P + mw_pad(Tq) * ps) : nullptr;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(src.kv + b * Tk * src.ldkv, Tk * src.ldkv * 4);
    const __amdgpu_buffer_rsrc_t qrs = make_rsrc(src.q + b * Tq * src.ldq, Tq * src.ldq * 4);
    const __amdgpu_buffer_rsrc_t grs = make_rsrc(dO + b * Tq * kTtD, Tq * kTtD * 4);
    mw_stage(qrs, src.ldq, src.colq + h * kTtHd, Q, Tq);
    mw_stage(grs, kTtD, h * kTtHd, G, Tq);
    mw_stage(krs, src.ldkv, src.colk + h * kTtHd, K, Tk);
    mw_stage(krs, src.ldkv, src.colv + h * kTtHd, V, Tk);
    if (mask) {
        const uint8_t* mk = mask + (int64_t)blockIdx.x * Tq * Tk;
        for (int e = threadIdx.x; e < Tq * Tk; e += 256) Mk[e] = mk[e];
    }
    const int t0[2] = {16 * wave, 16 * (wave + 4)}; // the wave's query tiles, and its key tiles
    const bool qone = t0[0] < Tq, qtwo = t0[1] < Tq, kone = t0[0] < Tk, ktwo = t0[1] < Tk; // (uniform)
    float qf[2][kTtHd / 4], gf[2][kTtHd / 4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        mw_frag(qrs, (t0[u] + col) * src.ldq + src.colq + h * kTtHd + q, qf[u]);
        mw_frag(grs, (t0[u] + col) * kTtD + h * kTtHd + q, gf[u]);
    }
    __syncthreads();
    if (qone) mw_probs(K, P, ps, t0, qtwo, qf, Tq, Tk, tt_key_len(klen, b, Tk), nullptr, 1.f); // P = S
    __syncthreads();
    const __amdgpu_buffer_rsrc_t okv = make_rsrc(dst.dkv + b * Tk * dst.lddkv, Tk * dst.lddkv * 4);
    f32x4 o[2][2];
    if (kone) { // dV[j][d] = sum_i drop(S)[i][j] dO[i][d]
        mw_zero(o);
        mw_acc_over_rows(G, P, ps, t0, ktwo, (Tq + 3) >> 2, Mk, scale, Tq, Tk, o);
        mw_store(okv, dst.lddkv, dst.coldv + h * kTtHd, t0, ktwo, o);
    }
    __syncthreads(); // every wave is done with S
    if (qone) {
        // dP^T = V dO^T for the wave's queries: dp[u][kt][r] = dP[t0_u + col][16 kt + 4 q + r]
        const int nkt = mw_pad(Tk) >> 4;
        f32x4 dp[2][kAttnMaxTiles];
        mw_rows_dot(V, nkt, gf[0], gf[1], qtwo, [&](int kt, f32x4 c0, f32x4 c1) {
            dp[0][kt] = c0;
            dp[1][kt] = c1;
        });
        // P <- dZ / sqrt(32) = S o (dSd - rowsum(dSd o S)) / sqrt(32); a row's sum: the lane's keys ascending, then
        // the row's four lanes
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u == 0 || qtwo) {
                const int i = t0[u] + col;
                float* row = P + i * ps + 4 * q;
                float rs = 0.f;
#pragma unroll
                for (int kt = 0; kt < kAttnMaxTiles; ++kt) {
                    if (kt < nkt) {
                        const f32x2 sa = *reinterpret_cast<const f32x2*>(row + 16 * kt);
                        const f32x2 sb = *reinterpret_cast<const f32x2*>(row + 16 * kt + 2);
                        const float sv[4] = {sa[0], sa[1], sb[0], sb[1]};
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int j = 16 * kt + 4 * q + r;
                            float dsd = dp[u][kt][r];
                            if (Mk) dsd = i < Tq && j < Tk && Mk[i * Tk + j] ? dsd * scale : 0.f;
                            dp[u][kt][r] = dsd;
                            rs = fmaf(dsd, sv[r], rs);
                        }
                    }
                }
                rs = quad_sum(rs);
#pragma unroll
                for (int kt = 0; kt < kAttnMaxTiles; ++kt) {
                    if (kt < nkt) {
                        const f32x2 sa = *reinterpret_cast<const f32x2*>(row + 16 * kt);
                        const f32x2 sb = *reinterpret_cast<const f32x2*>(row + 16 * kt + 2);
                        const float sv[4] = {sa[0], sa[1], sb[0], sb[1]};
                        float dz[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int j = 16 * kt + 4 * q + r;
                            dz[r] = i < Tq && j < Tk ? sv[r] * (dp[u][kt][r] - rs) * kTtQkScale : 0.f;
                        }
                        *reinterpret_cast<f32x2*>(row + 16 * kt) = f32x2{dz[0], dz[1]};
                        *reinterpret_cast<f32x2*>(row + 16 * kt + 2) = f32x2{dz[2], dz[3]};
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        mw_zero(o); // dQ[i][d] = sum_j dZ[i][j] K[j][d]
        mw_acc_over_cols(K, P, ps, t0, qtwo, (Tk + 3) >> 2, o);
        mw_store(make_rsrc(dst.dq + b * Tq * dst.lddq, Tq * dst.lddq * 4), dst.lddq, dst.coldq + h * kTtHd, t0, qtwo, o);
    }
    __syncthreads();
    if (kone) { // dK[j][d] = sum_i dZ[i][j] Q[i][d]
        mw_zero(o);
        mw_acc_over_rows(Q, P, ps, t0, ktwo, (Tq + 3) >> 2, nullptr, 1.f, Tq, Tk, o);
        mw_store(okv, dst.lddkv, dst.coldk + h * kTtHd, t0, ktwo, o);
    }
}

} // namespace b2h
