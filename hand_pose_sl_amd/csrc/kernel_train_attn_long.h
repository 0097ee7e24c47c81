// Blocked attention for training at more than 128 frames: the two attentions of TextPoseTransformer's decoder,
// self (Tq = Tk = T) and cross (Tq = T, Tk = S <= 128), forward and backward, where one (sequence, head) no longer
// fits LDS (kernel_train_attn.h's b2h_tt_sdpa keeps the whole (Tq, Tk) matrix there and stops at 128 x 128).  Same style
// as kernel_tenc_train.h / kernel_train_attn.h: exact fp32 on the vector ALU, one kernel per operation, keep-masks
// (uint8, 1 = keep) as inputs -- read from global memory here, Tq x Tk bytes do not fit LDS either --, `scale` =
// 1 / (1 - p), a NULL mask means p = 0, fmaf over d and 1 / sqrt(32) applied after the dot product.
//
//   b2h_lt_sdpa        O = drop(softmax(Q K^T / sqrt(32))) V by query blocks of 64 rows, the keys walked in blocks of
//                      128 with an online softmax; saves LSE_i = m_i + log l_i per (sequence, head, row)
//   b2h_lt_sdpa_bwd_q  the query owner: one workgroup per query block walks the key blocks, first for the row terms
//                      sigma_i = rowsum(P) and D_i = rowsum(dSd o P) / sigma_i, then for dQ, which it writes once
//   b2h_lt_sdpa_bwd_kv the key owner: one workgroup per key block walks the query blocks and writes dK, dV once
//
// The operands are described by AttnSrc and the gradients' destinations by LtGradDst (kernel_train_attn.h), so the
// same three kernels serve [Q | K | V] rows at ld 384 and QC at ld 128 against the memory's [K | V] rows at ld 256.
// The backward recomputes P_ij = exp(s_ij - LSE_i) / sigma_i block by block.  With dSd = keep ? dP * scale : 0 and
// dZ = P o (dSd - D):  dV_j = sum_i Pd_ij dO_i,  dK_j = sum_i dZ_ij Q_i / sqrt(32),  dQ_i = sum_j dZ_ij K_j / sqrt(32).
//
// Determinism: a workgroup belongs to one (sequence, head); every output element has one owner thread, which adds
// its terms in registers in ascending block and row order, an order fixed by (Tq, Tk) and the sequence's key length
// alone.  No atomics, no handoff between workgroups, nothing read from another sequence.
//
// Key lengths (klen, tt_key_len): the forward and the query owner end their key walk at
// kl <= Tk, so every walked block still holds a valid key 0 and the keys from kl on are never read; the key owner
// treats its block's keys from kl on as it treats keys past Tk, stores +0 for them, and a block wholly beyond kl
// stores its zeros without walking the queries.
#pragma once
#include "kernel_train_attn.h"

namespace b2h {

constexpr int kLtQb = 64, kLtKb = 128; // query rows and key rows per block
constexpr int kLtPs = kLtKb | 1;       // LDS row stride of a (64, 128) block of the score matrix

// Dynamic LDS (floats at stride 33 for the 32-wide rows):
//   forward   Q 64, K 128, V 128 rows, P 64 x 129, {m, l, alpha} x 64       =  76 032 B
//   key owner Q 64, dO 64, K 128, V 128 rows, Pd and dZ 64 x 129 each       = 116 736 B
//   query own Q 64, dO 64, K 128, V 128 rows, dZ 64 x 129, {D, sigma} x 64  =  84 224 B
constexpr size_t kLtFwdLds = (size_t)4 * ((kLtQb + 2 * kLtKb) * kTtQs + kLtQb * kLtPs + 3 * kLtQb);
constexpr size_t kLtBwdKvLds = (size_t)4 * ((2 * kLtQb + 2 * kLtKb) * kTtQs + 2 * kLtQb * kLtPs);
constexpr size_t kLtBwdQLds = (size_t)4 * ((2 * kLtQb + 2 * kLtKb) * kTtQs + kLtQb * kLtPs + 2 * kLtQb);

__host__ __device__ inline int lt_blocks(int n, int per) { return (n + per - 1) / per; }

__device__ inline float lt_dot(const float* a, const float* b) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < kTtHd; ++d) s = fmaf(a[d], b[d], s);
    return s;
}

// O[i][32 h + d] = sum_j keep_ij scale e_ij V[j][d] / l_i with e_ij = exp(s_ij - m_i), l_i = sum_j e_ij (unmasked);
// O (B*Tq, 128), mask (B, 4, Tq, Tk), lse (B, 4, Tq).  grid (B * 4, ceil(Tq / 64)), 256 threads, kLtFwdLds.
// A wave owns the rows w, w + 4, .. of the query block for the scores; a thread owns column d = tid % 32 of the
// rows tid / 32 + 8 r for the output.  The row state lives in LDS: running maximum, running sum and the factor
// alpha = exp(m_old - m_new) of the current key block (0 on the first block, where m_old is not formed).
__global__ __launch_bounds__(256) void b2h_lt_sdpa(AttnSrc src, const uint8_t* __restrict__ mask, float scale,
                                                   float* __restrict__ O, float* __restrict__ lse, int Tq, int Tk,
                                                   const int64_t* __restrict__ klen) {
    extern __shared__ __attribute__((aligned(16))) float smem_lt[];
    float* Q = smem_lt;
    float* K = Q + kLtQb * kTtQs;
    float* V = K + kLtKb * kTtQs;
    float* P = V + kLtKb * kTtQs;
    float* Mx = P + kLtQb * kLtPs;
    float* Ls = Mx + kLtQb;
    float* Al = Ls + kLtQb;
    const int64_t b = blockIdx.x / kTtHeads;
    const int h = blockIdx.x % kTtHeads;
    const int i0 = blockIdx.y * kLtQb, nq = min(kLtQb, Tq - i0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int d = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const float* kv = src.kv + b * Tk * src.ldkv + h * kTtHd;
    const uint8_t* mk = mask ? mask + ((int64_t)blockIdx.x * Tq + i0) * Tk : nullptr;
    tt_load_head(src.q + (b * Tq + i0) * src.ldq + src.colq + h * kTtHd, src.ldq, Q, nq);
    float acc[kLtQb / 8];
#pragma unroll
    for (int r = 0; r < kLtQb / 8; ++r) acc[r] = 0.f;
    const int kl = tt_key_len(klen, b, Tk);
    for (int j0 = 0; j0 < kl; j0 += kLtKb) {
        const int nk = min(kLtKb, kl - j0); // < 128 only in the last block
        __syncthreads();                    // the previous block is done with K, V, P
        tt_load_head(kv + (int64_t)j0 * src.ldkv + src.colk, src.ldkv, K, nk);
        tt_load_head(kv + (int64_t)j0 * src.ldkv + src.colv, src.ldkv, V, nk);
        __syncthreads();
        for (int i = w; i < nq; i += 4) {
            float s[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                s[u] = j < nk ? lt_dot(Q + i * kTtQs, K + j * kTtQs) * kTtQkScale : -INFINITY;
            }
            const float bm = tt_wave_max(fmaxf(s[0], s[1])); // finite: nk >= 1 (a NaN row stays NaN throughout)
            const float mo = j0 ? Mx[i] : bm, mn = fmaxf(mo, bm);
            const float al = j0 ? expf(mo - mn) : 0.f;
            float e[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) e[u] = lane + 64 * u < nk ? expf(s[u] - mn) : 0.f;
            const float sum = tt_wave_sum(e[0] + e[1]);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                float pd = e[u];
                if (mk && j < nk) pd = mk[(int64_t)i * Tk + j0 + j] ? pd * scale : 0.f;
                P[i * kLtPs + j] = pd;
            }
            if (lane == 0) {
                Mx[i] = mn;
                Ls[i] = j0 ? fmaf(Ls[i], al, sum) : sum; // no state is read on the first block
                Al[i] = al;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kLtQb / 8; ++r) {
            const int i = r0 + 8 * r;
            if (i < nq) {
                float a = acc[r] * Al[i];
                for (int j = 0; j < nk; ++j) a = fmaf(P[i * kLtPs + j], V[j * kTtQs + d], a);
                acc[r] = a;
            }
        }
    }
    float* out = O + (b * Tq + i0) * kTtD + h * kTtHd + d;
#pragma unroll
    for (int r = 0; r < kLtQb / 8; ++r) {
        const int i = r0 + 8 * r;
        if (i < nq) tt_store(out + (int64_t)i * kTtD, acc[r] / Ls[i]);
    }
    if (threadIdx.x < nq) lse[(int64_t)blockIdx.x * Tq + i0 + threadIdx.x] = Mx[threadIdx.x] + logf(Ls[threadIdx.x]);
}

// One row of a backward block, by the wave that owns it: for the keys j = lane + 64 u of the block
//   p = exp(s_ij - LSE_i) / sigma,  pd = keep ? p scale : 0,  dsd = keep ? (dO_i . V_j) scale : 0
// and zeros for the keys past nk.  mrow: the row's mask bytes from the block's first key, or nullptr.
__device__ inline void lt_bwd_terms(const float* q, const float* g, const float* K, const float* V, float lse, float sigma,
                                    const uint8_t* __restrict__ mrow, float scale, int nk, float (&p)[2], float (&pd)[2],
                                    float (&dsd)[2]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int j = lane + 64 * u;
        p[u] = pd[u] = dsd[u] = 0.f;
        if (j < nk) {
            p[u] = pd[u] = expf(lt_dot(q, K + j * kTtQs) * kTtQkScale - lse) / sigma;
            dsd[u] = lt_dot(g, V + j * kTtQs);
            if (mrow) {
                const bool keep = mrow[j] != 0;
                dsd[u] = keep ? dsd[u] * scale : 0.f;
                pd[u] = keep ? pd[u] * scale : 0.f;
            }
        }
    }
}

// The key owner: dK[j] and dV[j] of the key rows j0 .. j0 + 127 of one (sequence, head), summed over the query blocks
// in ascending order, rows ascending inside a block.  grid (B * 4, ceil(Tk / 128)), 256 threads, kLtBwdKvLds.
// A thread owns column d = tid % 32 of the key rows tid / 32 + 8 r, r < 16: 32 sums in registers, stored once.
__global__ __launch_bounds__(256) void b2h_lt_sdpa_bwd_kv(AttnSrc src, const float* __restrict__ dO,
                                                          const float* __restrict__ lse, const float* __restrict__ D,
                                                          const uint8_t* __restrict__ mask, float scale, LtGradDst dst,
                                                          int Tq, int Tk, const int64_t* __restrict__ klen) {
    extern __shared__ __attribute__((aligned(16))) float smem_lt[];
    float* Q = smem_lt;
    float* G = Q + kLtQb * kTtQs;
    float* K = G + kLtQb * kTtQs;
    float* V = K + kLtKb * kTtQs;
    float* Pd = V + kLtKb * kTtQs;
    float* dZ = Pd + kLtQb * kLtPs;
    const int64_t b = blockIdx.x / kTtHeads;
    const int h = blockIdx.x % kTtHeads;
    // nst rows are stored; the first nk of them are attended keys, the others get the +0 their sums start from
    const int j0 = blockIdx.y * kLtKb, nst = min(kLtKb, Tk - j0), nk = min(nst, tt_key_len(klen, b, Tk) - j0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, d = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const float* kv = src.kv + (b * Tk + j0) * src.ldkv + h * kTtHd;
    tt_load_head(kv + src.colk, src.ldkv, K, nk);
    tt_load_head(kv + src.colv, src.ldkv, V, nk);
    float av[kLtKb / 8], ak[kLtKb / 8];
#pragma unroll
    for (int r = 0; r < kLtKb / 8; ++r) av[r] = ak[r] = 0.f;
    const int tqw = nk > 0 ? Tq : 0; // (workgroup-uniform) a block with no attended key walks no query: it stores its +0
    for (int i0 = 0; i0 < tqw; i0 += kLtQb) {
        const int nq = min(kLtQb, Tq - i0);
        __syncthreads(); // the previous block is done with Q, G, Pd, dZ
        tt_load_head(src.q + (b * Tq + i0) * src.ldq + src.colq + h * kTtHd, src.ldq, Q, nq);
        tt_load_head(dO + (b * Tq + i0) * kTtD + h * kTtHd, kTtD, G, nq);
        __syncthreads();
        const int64_t row0 = (int64_t)blockIdx.x * Tq + i0;
        for (int i = w; i < nq; i += 4) {
            float p[2], pd[2], dsd[2];
            const float Di = D[2 * (row0 + i)], sigma = D[2 * (row0 + i) + 1];
            lt_bwd_terms(Q + i * kTtQs, G + i * kTtQs, K, V, lse[row0 + i], sigma,
                         mask ? mask + (row0 + i) * Tk + j0 : nullptr, scale, nk, p, pd, dsd);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                Pd[i * kLtPs + lane + 64 * u] = pd[u];
                dZ[i * kLtPs + lane + 64 * u] = p[u] * (dsd[u] - Di) * kTtQkScale;
            }
        }
        __syncthreads();
        for (int i = 0; i < nq; ++i) {
            const float g = G[i * kTtQs + d], q = Q[i * kTtQs + d];
#pragma unroll
            for (int r = 0; r < kLtKb / 8; ++r) {
                av[r] = fmaf(Pd[i * kLtPs + r0 + 8 * r], g, av[r]);
                ak[r] = fmaf(dZ[i * kLtPs + r0 + 8 * r], q, ak[r]);
            }
        }
    }
    float* out = dst.dkv + (b * Tk + j0) * dst.lddkv + h * kTtHd + d;
#pragma unroll
    for (int r = 0; r < kLtKb / 8; ++r) {
        const int j = r0 + 8 * r;
        if (j < nst) {
            tt_store(out + (int64_t)j * dst.lddkv + dst.coldk, ak[r]);
            tt_store(out + (int64_t)j * dst.lddkv + dst.coldv, av[r]);
        }
    }
}

// The query owner: dQ[i] of the query rows i0 .. i0 + 63 of one (sequence, head), summed over the key blocks in
// ascending order, keys ascending inside a block.  grid (B * 4, ceil(Tq / 64)), 256 threads, kLtBwdQLds.
// It walks the key blocks twice.  The first walk forms, from the very products the second walk and the key owner use,
//   sigma_i = sum_j exp(s_ij - LSE_i)   and   D_i = sum_j dSd_ij exp(s_ij - LSE_i) / sigma_i
// -- a lane adds its two keys of a block, the wave adds its lanes, the blocks are added in ascending order -- and
// writes {D_i, sigma_i} to D (B, 4, Tq, 2) for the key owner, which therefore runs after this kernel.  Both walks and
// the key owner then use P_ij = exp(s_ij - LSE_i) / sigma_i.  In mathematics sigma_i = 1 and D_i = dO_i . O_i; in fp32
// LSE_i is rounded to 2^-22 at its usual size of 4 .. 8, which scales a whole row of P by up to 1 +- 2.4e-7, and
// sum_j dZ_ij = D_i (1 - sum_j P_ij) is then a coherent residue instead of torch's few random ulps.  The gradients
// that are zero in mathematics (the key third of every in_proj_bias) consist of that residue alone, and Adam steps
// along it: without sigma the five-step trajectory at (4, 40, 200) ended 2.8e-5 from float64 in such a tensor, the
// fp32 reference 1.5e-6.  Dividing by sigma_i makes the row sum 1 to the rounding of its own
// terms, as in b2h_tt_sdpa_bwd.
// A thread owns column d = tid % 32 of the rows tid / 32 + 8 r, r < 8.
__global__ __launch_bounds__(256) void b2h_lt_sdpa_bwd_q(AttnSrc src, const float* __restrict__ dO,
                                                         const float* __restrict__ lse, float* __restrict__ D,
                                                         const uint8_t* __restrict__ mask, float scale, LtGradDst dst,
                                                         int Tq, int Tk, const int64_t* __restrict__ klen) {
    extern __shared__ __attribute__((aligned(16))) float smem_lt[];
    float* Q = smem_lt;
    float* G = Q + kLtQb * kTtQs;
    float* K = G + kLtQb * kTtQs;
    float* V = K + kLtKb * kTtQs;
    float* dZ = V + kLtKb * kTtQs;
    float* Ds = dZ + kLtQb * kLtPs;
    float* Sg = Ds + kLtQb;
    const int64_t b = blockIdx.x / kTtHeads;
    const int h = blockIdx.x % kTtHeads;
    const int i0 = blockIdx.y * kLtQb, nq = min(kLtQb, Tq - i0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, d = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const float* kv = src.kv + b * Tk * src.ldkv + h * kTtHd;
    const int64_t row0 = (int64_t)blockIdx.x * Tq + i0;
    tt_load_head(src.q + (b * Tq + i0) * src.ldq + src.colq + h * kTtHd, src.ldq, Q, nq);
    tt_load_head(dO + (b * Tq + i0) * kTtD + h * kTtHd, kTtD, G, nq);
    float aq[kLtQb / 8];
#pragma unroll
    for (int r = 0; r < kLtQb / 8; ++r) aq[r] = 0.f;
    const int kl = tt_key_len(klen, b, Tk);
    for (int walk = 0; walk < 2; ++walk)
        for (int j0 = 0; j0 < kl; j0 += kLtKb) {
            const int nk = min(kLtKb, kl - j0);
            __syncthreads(); // the previous block is done with K, V, dZ; the first walk's Ds is complete
            if (walk == 0 || kl > kLtKb) { // a single key block is still there
                tt_load_head(kv + (int64_t)j0 * src.ldkv + src.colk, src.ldkv, K, nk);
                tt_load_head(kv + (int64_t)j0 * src.ldkv + src.colv, src.ldkv, V, nk);
                __syncthreads();
            }
            for (int i = w; i < nq; i += 4) {
                float p[2], pd[2], dsd[2];
                const float sigma = walk ? Sg[i] : 1.f; // x / 1 is x
                lt_bwd_terms(Q + i * kTtQs, G + i * kTtQs, K, V, lse[row0 + i], sigma,
                             mask ? mask + (row0 + i) * Tk + j0 : nullptr, scale, nk, p, pd, dsd);
                if (walk == 0) {
                    // dsd carries the mask and the scale; p is the undropped probability
                    const float rs = tt_wave_sum(fmaf(dsd[1], p[1], dsd[0] * p[0])), sg = tt_wave_sum(p[0] + p[1]);
                    if (lane == 0) {
                        Ds[i] = j0 ? Ds[i] + rs : rs;
                        Sg[i] = j0 ? Sg[i] + sg : sg;
                    }
                } else {
                    const float Di = Ds[i] / sigma;
#pragma unroll
                    for (int u = 0; u < 2; ++u) dZ[i * kLtPs + lane + 64 * u] = p[u] * (dsd[u] - Di) * kTtQkScale;
                }
            }
            if (walk == 0) continue;
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kLtQb / 8; ++r) {
                const int i = r0 + 8 * r;
                if (i < nq) {
                    float a = aq[r];
                    for (int j = 0; j < nk; ++j) a = fmaf(dZ[i * kLtPs + j], K[j * kTtQs + d], a);
                    aq[r] = a;
                }
            }
        }
    if (threadIdx.x < nq) {
        D[2 * (row0 + threadIdx.x)] = Ds[threadIdx.x] / Sg[threadIdx.x];
        D[2 * (row0 + threadIdx.x) + 1] = Sg[threadIdx.x];
    }
    float* out = dst.dq + (b * Tq + i0) * dst.lddq + dst.coldq + h * kTtHd + d;
#pragma unroll
    for (int r = 0; r < kLtQb / 8; ++r) {
        const int i = r0 + 8 * r;
        if (i < nq) tt_store(out + (int64_t)i * dst.lddq, aq[r]);
    }
}

} // namespace b2h
