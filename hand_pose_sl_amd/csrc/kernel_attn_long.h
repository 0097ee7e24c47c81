// Attention over more than 128 query rows (TextPoseTransformer's decoder at T > 128, b2h_tpt_forward_fused): the
// keys no longer fit one workgroup's LDS and a query's scores no longer fit its registers, so the keys are walked
// in blocks with an online softmax.  Two kernels, one per arithmetic, on described operands (AttnSrc, b2h_common.h)
// like b2h_attn_f32 (kernel_tenc.h), so that each serves both uses:
//   out : (B*Tq, 128), head h -> columns 32 h ..
//   self-attention : q = kv = the chain's Q | K | V rows (ld 384, columns 0 / 128 / 256), Tk = Tq = T
//   cross-attention: q = the chain's QC rows (ld 128), kv = the memory's K | V rows (ld 256), Tk = S <= 128: one block
//
//   b2h_attn_long_f32<NK>  exact fp32 (v_mfma_f32_16x16x4_f32): K, V rows in LDS at the kAttnRow pitch, the score
//                          tile is the B operand of P.V: the tile products of b2h_attn_f32 (kernel_tenc.h).
//   b2h_attn_long_h3<NK>   B2H_TENC_F16X3: reads the same fp32 rows and splits them into f16 hi + lo as it stages
//                          them -- K rows at the kKRow pitch in the chain's k-slot order, V^T in vt_slot order --
//                          then split8 of the probabilities and three v_mfma_f32_16x16x32_f16 per product, as in
//                          attn_core_h3 (kernel_tpt.h).  The projections stay in the chain.
//
// Launch : grid (B * 4, query blocks), block = 64 * (query tiles per block): the host cuts the ceil(Tq / 16) query
//          tiles into ceil(tiles / 8) blocks of equal tile count, which is >= kLongMinWaves whenever Tq > 128 (9
//          tiles -> 2 x 5).  Wave w owns the 16 queries q0 + 16 w .. of its block.  NK = key tiles per key block,
//          cut the same way (13 tiles -> 2 blocks of NK = 7); the kernel walks ceil(Tk / (16 NK)) blocks, so the last
//          one always holds a valid key.
// Per key block: scores of the block's 16 NK keys, keys >= Tk masked to -inf (last block only), the block's maximum;
//          m' = max(m, block max); accumulators and sum are rescaled by exp(m - m') -- forced to 0 for the first
//          block, where m = -inf -- then p = exp(s - m'), l += sum p, O^T += V^T . P^T.  One division at the end.
// LDS    : two buffers of one key block's K and V.  Block j + 1 is requested into registers before block j's MFMAs
//          and written to the other buffer after them; one barrier per block (a buffer is rewritten one block after
//          the barrier every wave passed behind its reads of it).
// Global accesses are buffer instructions over the sequence's rows: rows past the end read 0, stores past the end
// are dropped, nothing is predicated per lane.  No atomics: a sequence's output depends on its own rows only and on
// nothing that varies between runs, streams or batch positions.
#pragma once
#include "kernel_tpt.h"

namespace b2h {

constexpr int kLongMinWaves = 5; // waves per workgroup the staging rounds below are sized for
constexpr int attn_long_f32_lds_bytes(int nk) { return 2 * attn_f32_lds_bytes(nk); }
constexpr int attn_long_h3_lds_bytes(int nk) { return 2 * attn_kv_bytes(nk); }

// attn_long_f32_body is the kernel; kl is the number of key rows attended, as in attn_f32_body (kernel_tenc.h): Tk in
// b2h_attn_long_f32, the sequence's key length in b2h_attn_long_klen_f32, where the key descriptor and the walk end at
// row kl, so a key block wholly beyond it is never staged.
template <int NK>
__device__ __forceinline__ void attn_long_f32_body(AttnSrc src, float* __restrict__ out, int Tq, int Tk, int kl) {
    extern __shared__ __attribute__((aligned(16))) char smem_al[];
    constexpr int kBuf = attn_f32_lds_bytes(NK);      // K, then V of one key block
    constexpr int kChunks = NK * 16 * 8;              // float4 of a block's K (and of its V)
    constexpr int R = (kChunks + 64 * kLongMinWaves - 1) / (64 * kLongMinWaves); // staging rounds: <= 4
    const int b = blockIdx.x / kTencHeads, h = blockIdx.x % kTencHeads;
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(src.kv + (int64_t)b * Tk * src.ldkv, kl * src.ldkv * 4);
    const __amdgpu_buffer_rsrc_t qrs = make_rsrc(src.q + (int64_t)b * Tq * src.ldq, Tq * src.ldq * 4);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nthreads = __builtin_amdgcn_readfirstlane(blockDim.x);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const int tq = (int)blockIdx.y * (nthreads >> 2) + wave * 16 + col; // 16 queries per wave
    const int nkb = (kl + 16 * NK - 1) / (16 * NK);
    // key block jb -> registers: rows >= kl (and chunks past the block) read 0
    auto fetch = [&](int jb, f32x4 (&k4)[R], f32x4 (&v4)[R]) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = threadIdx.x + r * nthreads, t = jb * 16 * NK + (i >> 3), c = i & 7;
            const int off = i < kChunks ? (t * src.ldkv + h * kTencHd + 4 * c) * 4 : (int)kOob;
            k4[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, off, src.colk * 4, 0));
            v4[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, off, src.colv * 4, 0));
        }
    };
    auto put = [&](int buf, const f32x4 (&k4)[R], const f32x4 (&v4)[R]) {
        float* Ks = reinterpret_cast<float*>(smem_al + buf * kBuf);
        float* Vs = reinterpret_cast<float*>(smem_al + buf * kBuf + kBuf / 2);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = threadIdx.x + r * nthreads, t = i >> 3, c = i & 7;
            if (i < kChunks) {
                *reinterpret_cast<f32x4*>(Ks + t * kAttnRow + 4 * c) = k4[r];
                *reinterpret_cast<f32x4*>(Vs + t * kAttnRow + 4 * c) = v4[r];
            }
        }
    };
    f32x4 kr[R], vr[R], qb[2];
    fetch(0, kr, vr);
#pragma unroll
    for (int g = 0; g < 2; ++g) // B operand of S^T: d = 16g + 4q + j
        qb[g] = buf_load4(qrs, tq * src.ldq + src.colq + h * kTencHd + 16 * g + 4 * q);
    put(0, kr, vr);
    qb[0] *= kAttnQkScale; // pre-scaled query (torch scales q, not the scores)
    qb[1] *= kAttnQkScale;
    __syncthreads();
    float m = -INFINITY, l = 0.f;
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 1
    for (int jb = 0; jb < nkb; ++jb) {
        const bool more = jb + 1 < nkb;
        fetch(jb + 1, kr, vr); // past the last block every row is >= kl: zeros, no memory traffic
        const float* Ks = reinterpret_cast<const float*>(smem_al + (jb & 1) * kBuf);
        const float* Vs = reinterpret_cast<const float*>(smem_al + (jb & 1) * kBuf + kBuf / 2);
        const int left = more ? 16 * NK : kl - jb * 16 * NK; // valid keys of this block (>= 1)
        f32x4 sc[NK];
        float bm = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NK; ++kt) {
            sc[kt] = tile_rows_dot(Ks, kt, qb, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int r = 0; r < 4; ++r) { // D row 4q + r = key index within the tile
                if (kt * 16 + 4 * q + r >= left) sc[kt][r] = -INFINITY;
                bm = fmaxf(bm, sc[kt][r]);
            }
        }
        bm = quad_max(bm); // finite: the block's key 0 is valid
        const float mn = fmaxf(m, bm);
        const float alpha = jb == 0 ? 0.f : expf(m - mn); // the first block has nothing to rescale (m = -inf)
        m = mn;
        float ls = 0.f;
#pragma unroll
        for (int kt = 0; kt < NK; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[kt][r] = expf(sc[kt][r] - mn); // masked keys: exp(-inf) = 0
                ls += sc[kt][r];
            }
        l = l * alpha + quad_sum(ls);
        o[0] *= alpha;
        o[1] *= alpha;
#pragma unroll
        for (int kt = 0; kt < NK; ++kt) tile_cols_acc(Vs, kt, sc[kt], o);
        if (more) { // (workgroup-uniform)
            put((jb + 1) & 1, kr, vr);
            __syncthreads();
        }
    }
    attn_store_out(out, b, Tq, tq, h, o, l);
}

template <int NK>
__global__ __launch_bounds__(64 * kAttnMaxTiles) void b2h_attn_long_f32(AttnSrc src, float* __restrict__ out, int Tq,
                                                                        int Tk) {
    attn_long_f32_body<NK>(src, out, Tq, Tk, Tk);
}

// b2h_attn_long_f32 with a key-padding mask: klen (B) int64 as in b2h_attn_klen_f32
template <int NK>
__global__ __launch_bounds__(64 * kAttnMaxTiles) void b2h_attn_long_klen_f32(AttnSrc src, float* __restrict__ out, int Tq,
                                                                           int Tk, const int64_t* __restrict__ klen) {
    attn_long_f32_body<NK>(src, out, Tq, Tk, attn_key_len(klen, blockIdx.x / kTencHeads, Tk));
}

template <int NK>
__global__ __launch_bounds__(64 * kAttnMaxTiles) void b2h_attn_long_h3(AttnSrc src, float* __restrict__ out, int Tq,
                                                                       int Tk) {
    extern __shared__ __attribute__((aligned(16))) char smem_alh[];
    constexpr int KS = (NK + 1) / 2;                  // k-steps of 32 keys
    constexpr int kKBytes = attn_k_bytes(NK), kKV = attn_kv_bytes(NK);
    constexpr int kItems = NK * 16 * 4;               // (key, lane quarter): 8 of the key's 32 K dims and 8 of its V dims
    constexpr int R = (kItems + 64 * kLongMinWaves - 1) / (64 * kLongMinWaves); // staging rounds: <= 2
    const int b = blockIdx.x / kTencHeads, h = blockIdx.x % kTencHeads;
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(src.kv + (int64_t)b * Tk * src.ldkv, Tk * src.ldkv * 4);
    const __amdgpu_buffer_rsrc_t qrs = make_rsrc(src.q + (int64_t)b * Tq * src.ldq, Tq * src.ldq * 4);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nthreads = __builtin_amdgcn_readfirstlane(blockDim.x);
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const int tq = (int)blockIdx.y * (nthreads >> 2) + wave * 16 + col;
    const int nkb = (Tk + 16 * NK - 1) / (16 * NK);
    // item (key t, quarter qq) holds k-slots (qq, j) = dims 16 (j >> 2) + 4 qq + (j & 3): two float4 of K, two of V
    auto fetch = [&](int jb, f32x4 (&k4)[R][2], f32x4 (&v4)[R][2]) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = threadIdx.x + r * nthreads, t = jb * 16 * NK + (i >> 2), qq = i & 3;
            const int off = i < kItems ? (t * src.ldkv + h * kTencHd + 4 * qq) * 4 : (int)kOob;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                k4[r][u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, off, (src.colk + 16 * u) * 4, 0));
                v4[r][u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, off, (src.colv + 16 * u) * 4, 0));
            }
        }
    };
    auto put = [&](int buf, const f32x4 (&k4)[R][2], const f32x4 (&v4)[R][2]) {
        _Float16* Kh = reinterpret_cast<_Float16*>(smem_alh + buf * kKV);
        _Float16* Kl = Kh + NK * 16 * kKRow;
        _Float16* Vh = Kl + NK * 16 * kKRow;
        _Float16* Vl = Vh + kTencHd * kAttnVtRow;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = threadIdx.x + r * nthreads, t = i >> 2, qq = i & 3;
            float vk[8], vv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                vk[j] = k4[r][j >> 2][j & 3];
                vv[j] = v4[r][j >> 2][j & 3];
            }
            f16x8 kh, kl, vh, vl;
            split8(vk, kh, kl);
            split8(vv, vh, vl);
            if (i < kItems) {
                *reinterpret_cast<f16x8*>(Kh + t * kKRow + 8 * qq) = kh;
                *reinterpret_cast<f16x8*>(Kl + t * kKRow + 8 * qq) = kl;
                const int vslot = vt_slot(t >> 4, t & 15);
#pragma unroll
                for (int j = 0; j < 8; ++j) { // V[key t][dim] -> V^T[dim][slot of the key]
                    const int d = 16 * (j >> 2) + 4 * qq + (j & 3);
                    Vh[d * kAttnVtRow + vslot] = vh[j];
                    Vl[d * kAttnVtRow + vslot] = vl[j];
                }
            }
        }
    };
    f32x4 kr[R][2], vr[R][2];
    fetch(0, kr, vr);
    f16x8 qh, ql;
    {
        f32x4 q4[2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
            q4[u] = buf_load4(qrs, tq * src.ldq + src.colq + h * kTencHd + 16 * u + 4 * q);
        float vq[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vq[j] = q4[j >> 2][j & 3] * kAttnQkScale; // torch scales q, not the scores
        split8(vq, qh, ql);
    }
    if (KS * 32 > NK * 16) { // odd NK: the last k-step's upper 16 key slots of V^T have no writer (both buffers)
        for (int i = threadIdx.x; i < 2 * kTencHd * 16; i += nthreads) {
            const int bufi = i / (kTencHd * 16), r = i % (kTencHd * 16);
            const int d = r >> 4, p = (KS - 1) * 32 + 8 * ((r >> 2) & 3) + 4 + (r & 3); // = vt_slot(NK, r & 15)
            _Float16* Vh = reinterpret_cast<_Float16*>(smem_alh + bufi * kKV + 2 * kKBytes);
            Vh[d * kAttnVtRow + p] = (_Float16)0.f;
            (Vh + kTencHd * kAttnVtRow)[d * kAttnVtRow + p] = (_Float16)0.f;
        }
    }
    put(0, kr, vr);
    __syncthreads();
    float m = -INFINITY, l = 0.f;
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 1
    for (int jb = 0; jb < nkb; ++jb) {
        const bool more = jb + 1 < nkb;
        fetch(jb + 1, kr, vr); // past the last block every row is >= Tk: zeros, no memory traffic
        const _Float16* Kh = reinterpret_cast<const _Float16*>(smem_alh + (jb & 1) * kKV);
        const _Float16* Kl = Kh + NK * 16 * kKRow;
        const _Float16* Vh = Kl + NK * 16 * kKRow;
        const _Float16* Vl = Vh + kTencHd * kAttnVtRow;
        const int left = more ? 16 * NK : Tk - jb * 16 * NK; // valid keys of this block (>= 1)
        f32x4 sc[2 * KS];
        float bm = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NK; ++kt) {
            const f16x8 ah = *reinterpret_cast<const f16x8*>(Kh + (kt * 16 + col) * kKRow + 8 * q);
            const f16x8 al = *reinterpret_cast<const f16x8*>(Kl + (kt * 16 + col) * kKRow + 8 * q);
            f32x4 s4 = f32x4{0.f, 0.f, 0.f, 0.f};
            s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, qh, s4, 0, 0, 0);
            s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, ql, s4, 0, 0, 0);
            s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, qh, s4, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) { // D row 4q + r = key index within the tile
                if (kt * 16 + 4 * q + r >= left) s4[r] = -INFINITY;
                bm = fmaxf(bm, s4[r]);
            }
            sc[kt] = s4;
        }
        if (2 * KS > NK) sc[2 * KS - 1] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        bm = quad_max(bm); // finite: the block's key 0 is valid
        const float mn = fmaxf(m, bm);
        const float alpha = jb == 0 ? 0.f : __expf(m - mn); // the first block has nothing to rescale (m = -inf)
        m = mn;
        float ls = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2 * KS; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[kt][r] = __expf(sc[kt][r] - mn); // v_exp_f32 (1 ulp); masked keys: exp(-inf) = 0
                ls += sc[kt][r];
            }
        l = l * alpha + quad_sum(ls);
        o[0] *= alpha;
        o[1] *= alpha;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            f16x8 ph, pl;
            float pv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) pv[j] = sc[2 * s + (j >> 2)][j & 3];
            split8(pv, ph, pl);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) { // A: V^T row d = 16mt + col, key slots 32s + 8q .. +7
                const f16x8 vh = *reinterpret_cast<const f16x8*>(Vh + (16 * mt + col) * kAttnVtRow + 32 * s + 8 * q);
                const f16x8 vl = *reinterpret_cast<const f16x8*>(Vl + (16 * mt + col) * kAttnVtRow + 32 * s + 8 * q);
                o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, o[mt], 0, 0, 0);
                o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, o[mt], 0, 0, 0);
                o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o[mt], 0, 0, 0);
            }
        }
        if (more) { // (workgroup-uniform)
            put((jb + 1) & 1, kr, vr);
            __syncthreads();
        }
    }
    attn_store_out(out, b, Tq, tq, h, o, l);
}

} // namespace b2h
