// The blocked training attention of kernel_train_attn_long.h on the matrix cores: b2h_mt_sdpa, b2h_mt_sdpa_bwd_q and
// b2h_mt_sdpa_bwd_kv are drop-in counterparts of b2h_lt_sdpa, b2h_lt_sdpa_bwd_q and b2h_lt_sdpa_bwd_kv -- the same
// arguments (AttnSrc operands, a uint8 keep-mask (B, 4, Tq, Tk) in global memory or NULL, `scale` = 1 / (1 - p)), the
// same O (B*Tq, 128), LSE (B, 4, Tq) and {D, sigma} (B, 4, Tq, 2) layouts, the same grids (64 query rows or 128 key
// rows per workgroup of 256 threads) and the same mathematics (DESIGN.md sections 16 and 17): an online softmax whose
// first block sets alpha = 0 and reads no state, mask and scale on the numerator only, a backward that recomputes
// P = exp(s - LSE) / sigma with sigma and D summed from the walk's own products.  b2h_tpt_set_train_kernel selects them.
//
// All six products run on v_mfma_f32_16x16x4_f32, whose result is a k-ordered fmaf chain in exact fp32; exp, the
// running maximum / sum / alpha, the mask, scale, sigma and D stay on the vector ALU.  A wave owns a 16-wide tile of
// the workgroup's rows as the COLUMNS of every product it forms, so a row of that tile never meets another row's
// numbers, and the first product's accumulator is the B operand of the second without leaving its registers
// (lane = (col, q): the 16 x 16 result holds row 4 q + r of column col in register r, and B[k = q][col] of the k-step
// r of the next product is that very register -- tile_rows_dot and tile_cols_acc of kernel_tenc.h, which the inference
// kernels b2h_attn_f32 and b2h_attn_long_f32 run too):
//
//   forward, query owner   columns = the wave's 16 queries.  S^T = K Q^T and dP^T = V dO^T (A = the key block's rows
//                          from LDS, B = Q / dO fragments in registers), then O^T += V^T Pd^T, dQ^T += K^T dZ^T
//                          (A = a column of the key block's V / K rows from LDS, B = the lane's own Pd / dZ).
//   key owner              columns = 16 keys; wave w owns the key tiles w and w + 4 of the block.  S = Q K^T and
//                          dP = dO V^T (A = the query block's rows from LDS, B = K / V fragments in registers), then
//                          dV^T += dO^T Pd and dK^T += Q^T dZ (A = a column of the query block's dO / Q rows).
//
// LDS holds two buffers of the walked block at the kAttnRow pitch -- K and V rows of 128 keys for the forward and the
// query owner, Q and dO rows of 64 queries with their LSE and {D, sigma} for the key owner.  Block n + 1 is requested
// into registers before block n's MFMAs and written to the other buffer after them: one barrier per block.
//
// Padded rows.  MFMA tiles run over whole multiples of 16 rows and 4 k-steps, so whatever is summed over must be
// zero, not stale, past the valid range: every staged row comes from a buffer load over the sequence's own rows, which
// returns 0 past its end, and all rows of a buffer are written for every block; scores of keys >= Tk are -inf before
// the maximum (forward) and their P is 0 (query owner); Pd and dZ of queries >= Tq are 0 (key owner); key tiles and
// query tiles with no valid row are skipped, wave-uniformly.  Rows past the end in the COLUMN position (queries of the
// forward and the query owner, keys of the key owner) only produce columns that the stores' range check drops.  The
// mask is read inside [0, Tq) x [0, Tk) only; stores are buffer stores over the sequence's rows.
//
// Key lengths (klen, tt_key_len), as in kernel_train_attn_long.h: the forward and the query owner
// put the end of their key descriptor and of their walk at kl <= Tk, so the keys from kl on are what the keys past Tk
// were, zeros that are never attended; the key owner forces Pd and dZ of its keys in [kl, Tk) to 0, as it does for the
// queries >= Tq, and stores the +0 its sums start from for every key tile below Tk that it did not walk.
//
// Determinism as in kernel_train_attn_long.h: one (sequence, head) per workgroup, one owner lane per output element,
// blocks and tiles added in ascending order, inside a tile the k-steps r = 0 .. 3 over the rows 4 q + r, q ascending.
// No atomics, no handoff between workgroups, nothing read from another sequence.
#pragma once
#include "kernel_tenc.h"
#include "kernel_train_attn_long.h"

namespace b2h {

constexpr int kMtQb = kLtQb, kMtKb = kLtKb;                 // the grids of the b2h_lt_* kernels
constexpr int kMtKvBuf = 2 * kMtKb * kAttnRow * 4;          // K, then V rows of one key block: 36 864 B
constexpr int kMtQgRows = 2 * kMtQb * kAttnRow;             // Q, then dO rows of one query block (floats)
constexpr int kMtQgBuf = (kMtQgRows + 3 * kMtQb) * 4;       // + LSE x 64, {D, sigma} x 64:     19 200 B
constexpr size_t kMtFwdLds = 2 * kMtKvBuf, kMtBwdQLds = 2 * kMtKvBuf, kMtBwdKvLds = 2 * kMtQgBuf;

struct MtRows {
    f32x4 a[4], b[4];
};

__device__ __forceinline__ f32x4 mt_zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// K and V rows j0 .. j0 + 127 of head h -> registers; rows >= Tk lie outside krs and read 0
__device__ __forceinline__ void mt_fetch_kv(__amdgpu_buffer_rsrc_t krs, const AttnSrc& src, int h, int j0, MtRows& x) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = threadIdx.x + 256 * r, off = (j0 + (i >> 3)) * src.ldkv + h * kTtHd + 4 * (i & 7);
        x.a[r] = buf_load4(krs, off + src.colk);
        x.b[r] = buf_load4(krs, off + src.colv);
    }
}
__device__ __forceinline__ void mt_put_kv(char* buf, const MtRows& x) {
    float* Ks = reinterpret_cast<float*>(buf);
    float* Vs = Ks + kMtKb * kAttnRow;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = threadIdx.x + 256 * r, o = (i >> 3) * kAttnRow + 4 * (i & 7);
        *reinterpret_cast<f32x4*>(Ks + o) = x.a[r];
        *reinterpret_cast<f32x4*>(Vs + o) = x.b[r];
    }
}

// O[i][32 h + d] = sum_j keep_ij scale e_ij V[j][d] / l_i with e_ij = exp(s_ij - m_i), l_i = sum_j e_ij (unmasked);
// lse_i = m_i + log l_i.  grid (B * 4, ceil(Tq / 64)), 256 threads, kMtFwdLds.  Wave w owns the queries i0 + 16 w ..;
// the row state (m, l) lives in the registers of the four lanes of a column.
__global__ __launch_bounds__(256) void b2h_mt_sdpa(AttnSrc src, const uint8_t* __restrict__ mask, float scale,
                                                   float* __restrict__ O, float* __restrict__ lse, int Tq, int Tk,
                                                   const int64_t* __restrict__ klen) {
    extern __shared__ __attribute__((aligned(16))) char smem_mt[];
    const int64_t b = blockIdx.x / kTtHeads;
    const int h = blockIdx.x % kTtHeads;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const int t0 = blockIdx.y * kMtQb + wave * 16, tq = t0 + col;
    const bool live = t0 < Tq; // wave-uniform: a wave past the end only stages
    const int kl = tt_key_len(klen, b, Tk); // the keys walked; Tk stays the stride of the rows and of the mask
    const int nkb = lt_blocks(kl, kMtKb);
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(src.kv + b * Tk * src.ldkv, kl * src.ldkv * 4);
    const __amdgpu_buffer_rsrc_t qrs = make_rsrc(src.q + b * Tq * src.ldq, Tq * src.ldq * 4);
    const uint8_t* mrow = mask && tq < Tq ? mask + ((int64_t)blockIdx.x * Tq + tq) * Tk : nullptr;
    MtRows nx;
    mt_fetch_kv(krs, src, h, 0, nx);
    f32x4 qb[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) qb[g] = buf_load4(qrs, tq * src.ldq + src.colq + h * kTtHd + 16 * g + 4 * q);
    mt_put_kv(smem_mt, nx);
    __syncthreads();
    float m = -INFINITY, l = 0.f;
    f32x4 o[2] = {mt_zero4(), mt_zero4()};
#pragma unroll 1
    for (int jb = 0; jb < nkb; ++jb) {
        const bool more = jb + 1 < nkb;
        if (more) mt_fetch_kv(krs, src, h, (jb + 1) * kMtKb, nx);
        const float* Ks = reinterpret_cast<const float*>(smem_mt + (jb & 1) * kMtKvBuf);
        const float* Vs = Ks + kMtKb * kAttnRow;
        const int left = min(kMtKb, kl - jb * kMtKb); // valid keys of this block (>= 1)
        if (live) {
            f32x4 sc[kMtKb / 16];
            float bm = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < kMtKb / 16; ++kt) {
                if (kt * 16 < left) {
                    sc[kt] = tile_rows_dot(Ks, kt, qb, mt_zero4());
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        sc[kt][r] = kt * 16 + 4 * q + r < left ? sc[kt][r] * kTtQkScale : -INFINITY;
                        bm = fmaxf(bm, sc[kt][r]);
                    }
                }
            }
            bm = quad_max(bm); // finite: the block's key 0 is valid (a NaN row stays NaN throughout)
            const float mn = fmaxf(m, bm);
            const float alpha = jb ? expf(m - mn) : 0.f; // the first block has nothing to rescale and reads no state
            m = mn;
            float ls = 0.f;
#pragma unroll
            for (int kt = 0; kt < kMtKb / 16; ++kt) {
                if (kt * 16 < left) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = kt * 16 + 4 * q + r;
                        float e = expf(sc[kt][r] - mn); // keys >= kl: exp(-inf) = 0
                        ls += e;
                        if (mask) e = mrow && j < left && mrow[jb * kMtKb + j] ? e * scale : 0.f;
                        sc[kt][r] = e;
                    }
                }
            }
            ls = quad_sum(ls);
            l = jb ? fmaf(l, alpha, ls) : ls;
            o[0] *= alpha;
            o[1] *= alpha;
#pragma unroll
            for (int kt = 0; kt < kMtKb / 16; ++kt)
                if (kt * 16 < left) tile_cols_acc(Vs, kt, sc[kt], o);
        }
        if (more) { // (workgroup-uniform)
            mt_put_kv(smem_mt + ((jb + 1) & 1) * kMtKvBuf, nx);
            __syncthreads();
        }
    }
    if (!live) return;
    // D rows 16 mt + 4 q + r = d of query tq; queries >= Tq fall outside the descriptor
    const __amdgpu_buffer_rsrc_t ors = make_rsrc(O + b * Tq * kTtD, Tq * kTtD * 4);
    buf_store4(ors, tq * kTtD + h * kTtHd + 4 * q, o[0] / l);
    buf_store4(ors, tq * kTtD + h * kTtHd + 16 + 4 * q, o[1] / l);
    if (q == 0 && tq < Tq) lse[(int64_t)blockIdx.x * Tq + tq] = m + logf(l);
}

// The query owner: dQ[i] of the query rows i0 .. i0 + 63 of one (sequence, head) and their row terms {D_i, sigma_i} for
// the key owner, which runs after this kernel.  grid (B * 4, ceil(Tq / 64)), 256 threads, kMtBwdQLds.  The key blocks
// are walked twice, as in b2h_lt_sdpa_bwd_q: first for sigma_i = sum_j exp(s_ij - LSE_i) and
// D_i = sum_j dSd_ij exp(s_ij - LSE_i) / sigma_i -- a lane adds its keys of a block, the column's four lanes are added,
// the blocks are added in ascending order --, then for dZ = P o (dSd - D) / sqrt(32) and dQ^T += K^T dZ^T.  A single key
// block (cross-attention) is staged once.
__global__ __launch_bounds__(256) void b2h_mt_sdpa_bwd_q(AttnSrc src, const float* __restrict__ dO,
                                                         const float* __restrict__ lse, float* __restrict__ D,
                                                         const uint8_t* __restrict__ mask, float scale, LtGradDst dst,
                                                         int Tq, int Tk, const int64_t* __restrict__ klen) {
    extern __shared__ __attribute__((aligned(16))) char smem_mt[];
    const int64_t b = blockIdx.x / kTtHeads;
    const int h = blockIdx.x % kTtHeads;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const int t0 = blockIdx.y * kMtQb + wave * 16, tq = t0 + col;
    const bool live = t0 < Tq;
    const int kl = tt_key_len(klen, b, Tk);
    const int nkb = lt_blocks(kl, kMtKb);
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(src.kv + b * Tk * src.ldkv, kl * src.ldkv * 4);
    const __amdgpu_buffer_rsrc_t qrs = make_rsrc(src.q + b * Tq * src.ldq, Tq * src.ldq * 4);
    const __amdgpu_buffer_rsrc_t grs = make_rsrc(dO + b * Tq * kTtD, Tq * kTtD * 4);
    const int64_t row = (int64_t)blockIdx.x * Tq + tq;
    const uint8_t* mrow = mask && tq < Tq ? mask + row * Tk : nullptr;
    MtRows nx;
    mt_fetch_kv(krs, src, h, 0, nx);
    f32x4 qb[2], gb[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        qb[g] = buf_load4(qrs, tq * src.ldq + src.colq + h * kTtHd + 16 * g + 4 * q);
        gb[g] = buf_load4(grs, tq * kTtD + h * kTtHd + 16 * g + 4 * q);
    }
    const float lse_i = tq < Tq ? lse[row] : 0.f;
    mt_put_kv(smem_mt, nx);
    __syncthreads();
    float Ds = 0.f, Sg = 0.f, sigma = 1.f, Di = 0.f; // x / 1 is x: the first walk's P is exp(s - LSE)
    f32x4 aq[2] = {mt_zero4(), mt_zero4()};
#pragma unroll 1
    for (int t = 0; t < 2 * nkb; ++t) {
        const bool walk = t >= nkb, more = nkb > 1 && t + 1 < 2 * nkb;
        const int jb = walk ? t - nkb : t;
        if (more) mt_fetch_kv(krs, src, h, (jb + 1 == nkb ? 0 : jb + 1) * kMtKb, nx);
        const float* Ks = reinterpret_cast<const float*>(smem_mt + (nkb > 1 ? t & 1 : 0) * kMtKvBuf);
        const float* Vs = Ks + kMtKb * kAttnRow;
        const int left = min(kMtKb, kl - jb * kMtKb);
        if (live) {
            if (t == nkb) { // the first walk's sums are complete
                sigma = Sg;
                Di = Ds / Sg;
            }
            float rs = 0.f, sg = 0.f;
#pragma unroll
            for (int kt = 0; kt < kMtKb / 16; ++kt) {
                if (kt * 16 < left) {
                    const f32x4 s = tile_rows_dot(Ks, kt, qb, mt_zero4()), dp = tile_rows_dot(Vs, kt, gb, mt_zero4());
                    f32x4 dz;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = kt * 16 + 4 * q + r;
                        // keys >= kl: P = 0; their V rows are 0, so is dP
                        const float p = j < left ? expf(s[r] * kTtQkScale - lse_i) / sigma : 0.f;
                        float dsd = dp[r];
                        if (mask) dsd = mrow && j < left && mrow[jb * kMtKb + j] ? dsd * scale : 0.f;
                        rs = fmaf(dsd, p, rs);
                        sg += p;
                        dz[r] = p * (dsd - Di) * kTtQkScale;
                    }
                    if (walk) tile_cols_acc(Ks, kt, dz, aq);
                }
            }
            if (!walk) {
                rs = quad_sum(rs);
                sg = quad_sum(sg);
                Ds = jb ? Ds + rs : rs;
                Sg = jb ? Sg + sg : sg;
            }
        }
        if (more) {
            mt_put_kv(smem_mt + ((t + 1) & 1) * kMtKvBuf, nx);
            __syncthreads();
        }
    }
    if (!live) return;
    if (q == 0 && tq < Tq) {
        D[2 * row] = Ds / Sg;
        D[2 * row + 1] = Sg;
    }
    const __amdgpu_buffer_rsrc_t ors = make_rsrc(dst.dq + b * Tq * dst.lddq, Tq * dst.lddq * 4);
    buf_store4(ors, tq * dst.lddq + dst.coldq + h * kTtHd + 4 * q, aq[0]);
    buf_store4(ors, tq * dst.lddq + dst.coldq + h * kTtHd + 16 + 4 * q, aq[1]);
}

// The key owner: dK[j] and dV[j] of the key rows j0 .. j0 + 127 of one (sequence, head), summed over the query blocks
// in ascending order.  grid (B * 4, ceil(Tk / 128)), 256 threads, kMtBwdKvLds.  Wave w owns the key tiles w and w + 4
// of the block (so that a short block, cross-attention's S keys, spreads over the waves); its K and V rows are B
// fragments in registers for the whole kernel.  Per query tile P and dP come out with the queries 4 q + r in the
// lane's four registers; Pd and dZ of queries >= Tq are forced to 0, since the queries are what dV and dK sum over.
__global__ __launch_bounds__(256) void b2h_mt_sdpa_bwd_kv(AttnSrc src, const float* __restrict__ dO,
                                                          const float* __restrict__ lse, const float* __restrict__ D,
                                                          const uint8_t* __restrict__ mask, float scale, LtGradDst dst,
                                                          int Tq, int Tk, const int64_t* __restrict__ klen) {
    extern __shared__ __attribute__((aligned(16))) char smem_mt[];
    const int64_t b = blockIdx.x / kTtHeads;
    const int h = blockIdx.x % kTtHeads;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const int kl = tt_key_len(klen, b, Tk);
    // the block's key tiles below `left` are walked, those below `nst` are stored (+0 where not walked)
    const int j0 = blockIdx.y * kMtKb, nst = min(kMtKb, Tk - j0), left = min(kMtKb, kl - j0);
    // a block wholly beyond kl (left <= 0) walks no query block: it only stores its zeros, and meets no barrier
    const int nqb = left > 0 ? lt_blocks(Tq, kMtQb) : 0;
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(src.kv + b * Tk * src.ldkv, Tk * src.ldkv * 4);
    const __amdgpu_buffer_rsrc_t qrs = make_rsrc(src.q + b * Tq * src.ldq, Tq * src.ldq * 4);
    const __amdgpu_buffer_rsrc_t grs = make_rsrc(dO + b * Tq * kTtD, Tq * kTtD * 4);
    const int64_t row0 = (int64_t)blockIdx.x * Tq;
    // query rows i0 .. i0 + 63 -> registers: Q and dO rows (>= Tq read 0), and for the first 64 threads a row's
    // LSE, D and sigma (0, 0, 1 past the end: finite, and forced out of the sums below)
    f32x4 nq4[2], ng4[2];
    float nl, nd, ns;
    auto fetch = [&](int i0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = threadIdx.x + 256 * r, t = i0 + (i >> 3), c = 4 * (i & 7);
            nq4[r] = buf_load4(qrs, t * src.ldq + src.colq + h * kTtHd + c);
            ng4[r] = buf_load4(grs, t * kTtD + h * kTtHd + c);
        }
        const int t = i0 + (int)threadIdx.x;
        const bool have = threadIdx.x < kMtQb && t < Tq;
        nl = have ? lse[row0 + t] : 0.f;
        nd = have ? D[2 * (row0 + t)] : 0.f;
        ns = have ? D[2 * (row0 + t) + 1] : 1.f;
    };
    auto put = [&](char* buf) {
        float* Qs = reinterpret_cast<float*>(buf);
        float* Gs = Qs + kMtQb * kAttnRow;
        float* St = Qs + kMtQgRows;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = threadIdx.x + 256 * r, o = (i >> 3) * kAttnRow + 4 * (i & 7);
            *reinterpret_cast<f32x4*>(Qs + o) = nq4[r];
            *reinterpret_cast<f32x4*>(Gs + o) = ng4[r];
        }
        if (threadIdx.x < kMtQb) {
            St[threadIdx.x] = nl;
            St[kMtQb + threadIdx.x] = nd;
            St[2 * kMtQb + threadIdx.x] = ns;
        }
    };
    fetch(0);
    f32x4 kb[2][2], vb[2][2], ak[2][2], av[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int off = (j0 + (wave + 4 * u) * 16 + col) * src.ldkv + h * kTtHd + 16 * g + 4 * q; // keys >= Tk read 0
            kb[u][g] = buf_load4(krs, off + src.colk);
            vb[u][g] = buf_load4(krs, off + src.colv);
            ak[u][g] = av[u][g] = mt_zero4();
        }
    put(smem_mt);
    __syncthreads();
#pragma unroll 1
    for (int ib = 0; ib < nqb; ++ib) {
        const bool more = ib + 1 < nqb;
        if (more) fetch((ib + 1) * kMtQb);
        const float* Qs = reinterpret_cast<const float*>(smem_mt + (ib & 1) * kMtQgBuf);
        const float* Gs = Qs + kMtQb * kAttnRow;
        const float* St = Qs + kMtQgRows;
        const int i0 = ib * kMtQb, nq = min(kMtQb, Tq - i0);
        if (wave * 16 < left) { // (wave-uniform) the wave has a key tile with a valid key
#pragma unroll 1
            for (int qt = 0; qt * 16 < nq; ++qt) {
                const f32x4 ls4 = *reinterpret_cast<const f32x4*>(St + qt * 16 + 4 * q);
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(St + kMtQb + qt * 16 + 4 * q);
                const f32x4 s4 = *reinterpret_cast<const f32x4*>(St + 2 * kMtQb + qt * 16 + 4 * q);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int kt = wave + 4 * u, j = j0 + kt * 16 + col;
                    if (kt * 16 < left) {
                        const f32x4 s = tile_rows_dot(Qs, qt, kb[u], mt_zero4()), dp = tile_rows_dot(Gs, qt, vb[u], mt_zero4());
                        f32x4 pd, dz;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int i = qt * 16 + 4 * q + r;
                            const float p = expf(s[r] * kTtQkScale - ls4[r]) / s4[r];
                            float w = p, dsd = dp[r];
                            if (mask) {
                                const bool keep = i < nq && j < kl && mask[(row0 + i0 + i) * Tk + j] != 0;
                                w = keep ? p * scale : 0.f;
                                dsd = keep ? dsd * scale : 0.f;
                            }
                            pd[r] = i < nq && j < kl ? w : 0.f; // a key in [kl, Tk) is stored, so it must sum zeros
                            dz[r] = i < nq && j < kl ? p * (dsd - d4[r]) * kTtQkScale : 0.f;
                        }
                        tile_cols_acc(Gs, qt, pd, av[u]);
                        tile_cols_acc(Qs, qt, dz, ak[u]);
                    }
                }
            }
        }
        if (more) {
            put(smem_mt + ((ib + 1) & 1) * kMtQgBuf);
            __syncthreads();
        }
    }
    // D rows 16 mt + 4 q + r = d of key j; keys >= Tk fall outside the descriptor
    const __amdgpu_buffer_rsrc_t ors = make_rsrc(dst.dkv + b * Tk * dst.lddkv, Tk * dst.lddkv * 4);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int kt = wave + 4 * u, off = (j0 + kt * 16 + col) * dst.lddkv + h * kTtHd + 4 * q;
        if (kt * 16 < nst) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                buf_store4(ors, off + dst.coldk + 16 * mt, ak[u][mt]);
                buf_store4(ors, off + dst.coldv + 16 * mt, av[u][mt]);
            }
        }
    }
}

} // namespace b2h
