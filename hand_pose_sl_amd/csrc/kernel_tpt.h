// TextPoseTransformer (body2hand/src/models/HandPoseModels.py:181-230) on gfx950: the kernels the
// text-conditioned model needs beyond TransformerEnc's (kernel_tenc.h).  Inference, exact fp32 or f16x3.
//
//   b2h_tpt_embed        token_embedding(input_tokens) (:206): row n of the (B*S, 128) encoder input is
//                        table[tokens[n]], not scaled.
//   b2h_attn_cross_h3    the decoder's multihead_attn for B2H_TENC_F16X3, with its Q, K and V projections inside:
//                        queries are the T target frames of a sequence (their norm1 rows), keys and values the S rows
//                        of the encoder memory of the same sequence, so neither Q nor the memory's K | V cross HBM.
//                        The reference passes no mask (:211): every memory row is attended, padded token ids included.
//                        (In exact fp32 that attention is b2h_attn_f32, kernel_tenc.h, on the QC and memory K | V rows.)
//   b2h_tpt_layernorm    encoder.norm / decoder.norm, the LayerNorm that ends each stack of torch.nn.Transformer.
//   b2h_item_pad_rows     42- and 58-float pose rows -> zero-padded 64-float rows for the chain's front.
//   b2h_item_build_kernel  the composite input rows of `--predict right_index` / `right_3fingers`.
//
// Everything else of the model is per-frame and runs as descriptors of b2h_tenc_chain<H3>; the self-attention of
// both stacks is b2h_attn_f32 or b2h_attn_qkv_h3 (b2h_api.hip: tpt_launch has the launch lists).  Targets of
// more than 128 frames (b2h_tpt_forward_fused) run the decoder's two attentions on kernel_attn_long.h instead.
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

// Pose rows of 42 or 58 floats (the composite inputs of `--predict right_index` / `right_3fingers`) end inside a
// lane's float4 of the chain kernel's row load, and their 168- / 232-byte pitch is no multiple of 16.  The chain
// therefore reads them from a copy at a pitch of kTptPadLd floats whose surplus columns are zeros: out[n][c] =
// c < ninp ? x[n][c] : 0.  One thread per output float; 256 B per frame in front of ~1 Mflop per frame.
constexpr int kTptPadLd = 64;
__global__ __launch_bounds__(256) void b2h_item_pad_rows(const float* __restrict__ x, float* __restrict__ out, int64_t n,
                                                        int ninp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = i / kTptPadLd;
    const int c = (int)(i % kTptPadLd);
    if (row >= n) return;
    out[i] = c < ninp ? x[row * ninp + c] : 0.f;
}

// The model input of `--predict right_index` (predict = 1) and `right_3fingers` (predict = 2) from raw body (N, 12, 2)
// and right-hand (N, 21, 2) keypoints, in run.py:85-104's order: WristDifference on the hand with the RAW body wrist
// (joint 4), ChestDifference on the body (joint 1) [flags & kPreChest], / factor on both [flags & kPreNorm], then
//   predict 1 (BuildIndexItem,   29 joints): body 0..11, hand 0..4, hand 9..20
//   predict 2 (Build3fingerItem, 21 joints): hand 13..20, hand 0, body 0..11        (steps/utils.py:194-259)
// One thread per (frame, output joint): a subtraction and a true division, each correctly rounded.
__global__ __launch_bounds__(256) void b2h_item_build_kernel(const float* __restrict__ body,
                                                                 const float* __restrict__ hand, float* __restrict__ item,
                                                                 int64_t frames, int predict, int flags, float factor) {
    const int nj = predict == 1 ? 29 : 21;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= frames * nj) return;
    const int64_t f = i / nj;
    const int j = (int)(i % nj);
    int src; // < 12: body joint src; otherwise hand joint src - 12
    if (predict == 1) src = j < 12 ? j : (j < 17 ? j : j + 4);           // hand 0..4 -> 12..16, hand 9..20 -> 21..32
    else src = j < 8 ? 12 + 13 + j : (j == 8 ? 12 : j - 9);
    const bool is_body = src < 12;
    const float2* b2 = reinterpret_cast<const float2*>(body + f * kInCh);
    float2 v = is_body ? b2[src] : reinterpret_cast<const float2*>(hand + f * kOutCh)[src - 12];
    if (flags & kPreChest) {
        const float2 w = b2[is_body ? 1 : 4];
        v.x -= w.x; v.y -= w.y;
    }
    if (flags & kPreNorm) { v.x = v.x / factor; v.y = v.y / factor; }
    *reinterpret_cast<float2*>(item + i * 2) = v;
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

// ---- Q, K, V projection + cross-attention in one kernel (B2H_TENC_F16X3) ------------------------------------------
// The two-row-set sibling of b2h_attn_qkv_h3 (kernel_tenc.h; its comment has the fragment layouts, all reused here):
// queries come from the T frame rows `x` (the decoder's norm1 output), keys and values from the S rows `mem` of the
// encoder memory of the same sequence, both projected here from multihead_attn.in_proj on three
// v_mfma_f32_16x16x32_f16 per product, so that Q and the memory's K | V never cross HBM.
//   Launch : persistent and bound to a head like the sibling (blockIdx = 8 (4 slot + head) + xcd, b += 8 nslots);
//            block = 64 ceil(T / 16) threads, wave w owns query tile w; only NK = ceil(S / 16) is a template
//            parameter (8 instantiations, as b2h_attn_f32).
//   Weights: the head's blob is the one b2h_attn_qkv_h3 takes -- [hi: mt(6)][g(4)][lane] f16x8, [lo] the same, 384
//            fp32 with the 96 biases first; M-tiles 0-1 = Q_h, 2-3 = K_h, 4-5 = V_h -- copied to LDS once per
//            workgroup.  The two projections address their M-tiles inside it with chain_gemm_h3_at: Q at (hi, lo),
//            K | V at (hi + 2*4*64, lo + 2*4*64) fragments; the lo half starts 6*4*64 fragments behind the hi half.
//   Per sequence, wave w:
//            x rows of its 16 frames --split--> Q_h (2 M-tiles) * 32^-0.5 --split--> qh, ql in registers;
//            for key tiles kt = w, w + nwaves, .. < NK: the 16 mem rows of the tile --split--> K_h | V_h (4 M-tiles)
//            -> LDS, K rows at the kKRow pitch, V^T at the kAttnVtRow pitch in vt_slot order, hi and lo.  With fewer
//            query tiles than key tiles a wave projects several key tiles, with more some waves project none.
//            Every key row below 16 NK is written for every sequence: rows >= S read 0 from the descriptor, so they
//            hold the bias (finite) and are masked to -inf by the core.
//            barrier; attn_core_h3 below: scores, softmax, P.V, two 16-byte stores per lane.
//   LDS    : [blob 50 688 B][K hi | K lo | V^T hi | V^T lo] x 2 buffers = attn_qkv_lds_bytes(NK), 134 656 B at
//            NK = 8.  K, V are double-buffered exactly as in the sibling (one barrier per sequence: a buffer is
//            rewritten two sequences on, after a barrier every wave has passed its reads of).
// The next sequence's x rows and the wave's first memory tile are requested before this sequence's MFMAs.  All
// global accesses are buffer instructions: rows >= T or >= S read 0, stores of rows >= T are dropped, and a
// sequence past the batch gets an empty descriptor; nothing is predicated per lane.  A sequence's output depends
// on its own rows only, whichever slot, pass or buffer handles it.
struct AttnCrossArgs {
    const float* x;        // (B*T, 128) query rows: the decoder layer's norm1 output
    const float* mem;      // (B*S, 128) encoder memory
    float* out;            // (B*T, 128) attention output, head h -> columns 32h ..
    const float* blob[kTencHeads]; // per head, of multihead_attn.in_proj: AttnQkvArgs::blob's layout
    int T, S;
    int64_t B;
};

// From "K and V of the sequence complete in LDS" to the output stores: score tiles S^T = K . Q^T (lo.hi + hi.lo +
// hi.hi), the mask of keys >= Tk, softmax over the keys inside the lane quartet (v_exp_f32), O^T = V^T . P^T with
// the score registers as the B operand, the normalisation and the two stores of query row tq (attn_store_out).  Up to
// the stores this is the tail of b2h_attn_qkv_h3 (kernel_tenc.h) line for line, with the key count Tk apart from the
// query count Tq.  It is a copy
// and not one function for both kernels because sharing it changed the sibling's code: with the tail moved into a
// force-inlined function, b2h_attn_qkv_h3<1> came out with 134 instead of 130 VGPRs and 7 more instructions and
// <5> with another register count, and TransformerEnc's kernels are not to change for this model (DESIGN.md
// section 12).
template <int NK>
__device__ __forceinline__ void attn_core_h3(const _Float16* Kh, const _Float16* Kl, const _Float16* Vh, const _Float16* Vl,
                                             const f16x8 qh, const f16x8 ql, int Tk, float* out, int Tq, int64_t b,
                                             int h, int tq, int col, int q) {
    constexpr int KS = (NK + 1) / 2; // k-steps of 32 keys
    f32x4 sc[2 * KS];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) {
        const f16x8 ah = *reinterpret_cast<const f16x8*>(Kh + (kt * 16 + col) * kKRow + 8 * q);
        const f16x8 al = *reinterpret_cast<const f16x8*>(Kl + (kt * 16 + col) * kKRow + 8 * q);
        f32x4 s4 = f32x4{0.f, 0.f, 0.f, 0.f};
        s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, qh, s4, 0, 0, 0);
        s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, ql, s4, 0, 0, 0);
        s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, qh, s4, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) { // D row 4q + r = key index within the tile; only the last tile can cross Tk
            if (kt == NK - 1 && kt * 16 + 4 * q + r >= Tk) s4[r] = -INFINITY;
            mx = fmaxf(mx, s4[r]);
        }
        sc[kt] = s4;
    }
    if (2 * KS > NK) sc[2 * KS - 1] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    mx = quad_max(mx);
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2 * KS; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sc[kt][r] = __expf(sc[kt][r] - mx); // v_exp_f32 (1 ulp); masked keys: exp(-inf) = 0
            l += sc[kt][r];
        }
    l = quad_sum(l);
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
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
    attn_store_out(out, b, Tq, tq, h, o, l);
}

template <int NK>
__global__ __launch_bounds__(64 * kAttnMaxTiles) void b2h_attn_cross_h3(AttnCrossArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_ax[];
    constexpr int KS = (NK + 1) / 2;                          // k-steps of 32 keys
    constexpr int kKBytes = attn_k_bytes(NK), kKV = attn_kv_bytes(NK);
    constexpr int kFragLo = kQkvMT * 4 * 64;                  // f16x8 fragments of the hi half
    const f16x8* whi = reinterpret_cast<const f16x8*>(smem_ax);
    const float* prm = reinterpret_cast<const float*>(smem_ax + 2 * kFragLo * 16);
    char* kvbase = smem_ax + kQkvBlobBytes;
    // which head, which sequences: blockIdx = 8 * (4 * slot + head) + xcd
    const int xcd = blockIdx.x & 7, inx = blockIdx.x >> 3, h = inx & 3, slot = inx >> 2;
    const int nslots = (int)((gridDim.x >> 3) >> 2);          // sequence slots per XCD
    const int64_t stride = 8 * (int64_t)nslots;
    int64_t b = (int64_t)slot * 8 + xcd;
    const int nthreads = __builtin_amdgcn_readfirstlane(blockDim.x);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = nthreads >> 6;
    const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const int tq = wave * 16 + col;
    // the head's weights: once per workgroup
    for (int i = threadIdx.x; i < kQkvBlobBytes / 16; i += nthreads)
        reinterpret_cast<uint4*>(smem_ax)[i] = reinterpret_cast<const uint4*>(a.blob[h])[i];
    if (b >= a.B) return; // (no barrier has been entered yet)
    // row `row` of sequence bb of a (B*n, 128) row set, features 16g + 4q .. +3; rows >= n and sequences >= B read 0
    auto load_rows = [&](f32x4 (&r)[8], const float* base, int n, int64_t bb, int row) {
        const bool on = bb < a.B;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(base + (on ? bb : 0) * n * kTencD, on ? n * kTencD * 4 : 0);
#pragma unroll
        for (int g = 0; g < 8; ++g) r[g] = chain_ld(rs, (uint32_t)(row * kTencD + 16 * g + 4 * q) * 4u);
    };
    f32x4 xr[8], mr[8];
    load_rows(xr, a.x, a.T, b, tq);
    if (wave < NK) load_rows(mr, a.mem, a.S, b, tq); // key tile `wave`, row 16 wave + col
    if (KS * 32 > NK * 16) { // odd NK: the last k-step's upper 16 key slots of V^T have no writer (both buffers)
        for (int i = threadIdx.x; i < 2 * kTencHd * 16; i += nthreads) {
            const int bufi = i / (kTencHd * 16), r = i % (kTencHd * 16);
            const int d = r >> 4, p = (KS - 1) * 32 + 8 * ((r >> 2) & 3) + 4 + (r & 3); // = vt_slot(NK, r & 15): tile NK's keys
            _Float16* Vh = reinterpret_cast<_Float16*>(kvbase + bufi * kKV + 2 * kKBytes);
            Vh[d * kAttnVtRow + p] = (_Float16)0.f;
            (Vh + kTencHd * kAttnVtRow)[d * kAttnVtRow + p] = (_Float16)0.f;
        }
    }
    __syncthreads(); // weights (and the V^T padding) in LDS
    int buf = 0;
#pragma unroll 1
    for (; b < a.B; b += stride, buf ^= 1) {
        _Float16* Kh = reinterpret_cast<_Float16*>(kvbase + buf * kKV);
        _Float16* Kl = Kh + NK * 16 * kKRow;
        _Float16* Vh = Kl + NK * 16 * kKRow;
        _Float16* Vl = Vh + kTencHd * kAttnVtRow;
        f16x8 bh[4], bl[4];
        f32x4 acc[8];
        // Q_h of this wave's 16 frames: M-tiles 0-1
        chain_split(xr, bh, bl);
        load_rows(xr, a.x, a.T, b + stride, tq); // the next sequence's rows travel under this one's work
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[mt] = *reinterpret_cast<const f32x4*>(prm + 16 * mt + 4 * q);
        chain_gemm_h3_at<4, 2>(whi, whi + kFragLo, lane, bh, bl, acc);
        f16x8 qh, ql;
        {
            float vq[8]; // slot (q, j) = dim 16 (j >> 2) + 4q + (j & 3) = accumulator (j >> 2, j & 3)
#pragma unroll
            for (int j = 0; j < 8; ++j) vq[j] = acc[j >> 2][j & 3] * kAttnQkScale; // torch scales q, not the scores
            split8(vq, qh, ql);
        }
        // K_h | V_h of this wave's key tiles: M-tiles 2-5
#pragma unroll 1
        for (int kt = wave; kt < NK; kt += nwaves) {
            chain_split(mr, bh, bl);
            // the wave's next key tile of this sequence, or its first one of the next sequence
            const bool more = kt + nwaves < NK;
            load_rows(mr, a.mem, a.S, more ? b : b + stride, (more ? kt + nwaves : wave) * 16 + col);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = *reinterpret_cast<const f32x4*>(prm + kTencHd + 16 * mt + 4 * q);
            chain_gemm_h3_at<4, 4>(whi + 2 * 4 * 64, whi + kFragLo + 2 * 4 * 64, lane, bh, bl, acc);
            float vk[8], vv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                vk[j] = acc[j >> 2][j & 3];
                vv[j] = acc[2 + (j >> 2)][j & 3];
            }
            f16x8 kh, kl, vh, vl;
            split8(vk, kh, kl);
            split8(vv, vh, vl);
            const int key = kt * 16 + col, vslot = vt_slot(kt, col);
            *reinterpret_cast<f16x8*>(Kh + key * kKRow + 8 * q) = kh;
            *reinterpret_cast<f16x8*>(Kl + key * kKRow + 8 * q) = kl;
#pragma unroll
            for (int j = 0; j < 8; ++j) { // V[key][dim 16 (j >> 2) + 4q + (j & 3)] -> V^T[dim][slot of the key]
                const int d = 16 * (j >> 2) + 4 * q + (j & 3);
                Vh[d * kAttnVtRow + vslot] = vh[j];
                Vl[d * kAttnVtRow + vslot] = vl[j];
            }
        }
        __syncthreads(); // K, V of this sequence complete (the other buffer is free again two sequences on)
        attn_core_h3<NK>(Kh, Kl, Vh, Vl, qh, ql, a.S, a.out, a.T, b, h, tq, col, q);
    }
}

} // namespace b2h
