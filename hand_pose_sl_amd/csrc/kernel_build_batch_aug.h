// A training batch with data augmentation (b2h_build_batch_aug, include/b2h.h): every sequence of
// a batch is scaled, rotated and mirrored about its own chest and its input joints are jittered, drawn and applied
// inside the build launch.  The reference has no augmentation: the definition is this project's own, stated so that
// tests/augment_ref.py (numpy float32) reproduces every output bit.
//
// Meaning: "augment the raw frame, then do what b2h_build_batch_k does".  For a live frame of the sequence with draw
// index p a VIRTUAL store row is formed; selection, padding, B2H_BATCH_DIF_ENCODING, B2H_BATCH_NORMALIZE and the
// `predict` gather apply to it unchanged.  Frames of zero padding stay zeros; B2H_BATCH_PAD_FRAME0 frames are live.
//
//   p       = *step * B + b with a step word (the plan entry, kernel_build_batch.h's rules), entry0 + b without.
//   Philox(c0, c1, c2, c3) is dm_philox of kernel_dropout_masks.h under key (seed lo, seed hi); {seed, epoch} are the two
//           device words `key`, only read.  Counter word c1 is the tag: 0 .. 4 are b2h_epoch_plan's, 16 and 17 these.
//   d(w)    = float(w >> 8) * 2^-24 * 2 - 1: in [-1, 1), exact in fp32.
//   sequence block (p, 16, epoch lo, epoch hi): word 0 the scale, word 1 the rotation, word 2 the mirror, word 3 unused.
//           s = 1 + scale * d(w0);  t = rotate_tan * d(w1);  t2 = t * t;  den = 1 + t2;  c = (1 - t2) / den;
//           sn = (t + t) / den: the rational form of the rotation by theta with tan(theta / 2) = t -- no sinf / cosf,
//           whose bits differ between device and host.  mirror = w2 < ceil(double(mirror_p) * 2^32), in 64 bits.
//   virtual joint q reads store joint q' = mirror ? M(q) : q, its confidence copied.  M swaps the hand blocks joint for
//           joint and the body's sides: [0, 1, 5, 6, 7, 2, 3, 4, 9, 8, 11, 10] (n_body 8: the first eight).  With
//           (cx, cy) the frame's raw chest (body joint 1, which M fixes):
//           dx = x - cx;  dy = y - cy;  if (mirror) dx = -dx;  rx = c * dx - sn * dy;  ry = sn * dx + c * dy;
//           x' = cx + s * rx;  y' = cy + s * ry.
//           A joint OpenPose missed (0, 0, conf 0) is transformed like any other: the reference's own transforms treat
//           it no differently.
//   jitter  on input_kp only, after the difference encoding and before the division by factor: input joint j of frame
//           t (the output frame, also for a PAD_FRAME0 copy) takes words 2 (j & 1) and 2 (j & 1) + 1 of the block
//           (p, 17 | t << 8, epoch lo, j >> 1):  v.x = v.x + jitter * d(w_x);  v.y = v.y + jitter * d(w_y).  The epoch
//           enters the jitter with its LOW 32 bits only (c3 carries the joint pair); t < 2^24 by the limit on T.
//
// A stage whose parameters are zero is not run, so that it changes no bit (x' = cx + (x - cx) is not x in fp32, and
// v + 0 * d turns a -0 into +0): with scale and rotate_tan both 0 the rotation-and-scale stage is skipped -- y' = y, and
// x' = x, or cx + dx under a mirror --; with jitter 0 nothing is added.  All four 0 is b2h_build_batch_k bit for bit.
//
// Every fp32 operation above is one correctly rounded operation: each function with arithmetic switches contraction off
// and writes it with the plain operators -- hipcc's __fmul_rn and __fadd_rn are header functions compiled under the
// default contraction, and inlined here their product and sum fuse into one v_fma_f32 whatever pragma the caller has --
// and / is the correctly rounded division hipcc gives by default, as in kernel_build_batch.h.
//
// The kernel is bb_run of kernel_build_batch.h, the body it shares with b2h_build_batch_k -- the grid's five block runs,
// one float2 per lane, every output word written exactly once, padding, the difference encoding, the division -- with
// BaLane below for the three things that differ: the value of a live joint, the joint whose confidence is copied, and
// the jitter.  The sequence block is recomputed per lane (one Philox block and about ten operations), the jitter block
// only on the input_kp run.  No LDS, no atomics, no scratch; ordinary vector stores.
#pragma once
#include "kernel_build_batch.h"
#include "kernel_dropout_masks.h"

namespace b2h {

constexpr uint32_t kBaTagSequence = 16, kBaTagJitter = 17;   // counter word c1; 0 .. 4 are kernel_epoch_plan.h's

struct BaArgs {
    BbArgs b;
    const uint64_t* key;      // device {seed, epoch}, only read
    int64_t entry0;           // the draw index of sequence 0 without a step word
    uint64_t mirror_thr;      // ceil(mirror_p * 2^32), 0 .. 2^32
    float scale, rotate_tan, jitter;
    int spin;                 // scale or rotate_tan is not 0: the rotation-and-scale stage runs
};

struct BaSeq {                // one sequence's draws
    float s, c, sn;
    bool mirror;
};

__device__ __forceinline__ float ba_unit(uint32_t w) {    // d(w)
#pragma clang fp contract(off)
    return (float)(w >> 8) * 0x1p-24f * 2.f - 1.f;
}

__device__ __forceinline__ BaSeq ba_sequence(const BaArgs& g, uint32_t p, uint64_t seed, uint64_t epoch) {
#pragma clang fp contract(off)
    uint32_t w[4];
    dm_philox(p, kBaTagSequence, (uint32_t)epoch, (uint32_t)(epoch >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    BaSeq q;
    q.s = 1.f + g.scale * ba_unit(w[0]);
    const float t = g.rotate_tan * ba_unit(w[1]);
    const float t2 = t * t, den = 1.f + t2;
    q.c = (1.f - t2) / den;
    q.sn = (t + t) / den;
    q.mirror = (uint64_t)w[2] < g.mirror_thr;
    return q;
}

// M: the store joint that lands on joint q under a mirror.
__device__ __forceinline__ int ba_mirrored(int n_body, int q) {
    if (q >= n_body) return q < n_body + 21 ? q + 21 : q - 21;
    return q < 2 ? q : q < 5 ? q + 3 : q < 8 ? q - 3 : q ^ 1;
}

// Joint q of the virtual row of store row r.
__device__ __forceinline__ float2 ba_joint(const BaArgs& g, const BaSeq& d, const float* r, int J, int q) {
#pragma clang fp contract(off)
    const int from = d.mirror ? ba_mirrored(g.b.n_body, q) : q;
    const float x = r[from], y = r[J + from];
    if (!g.spin && !d.mirror) return make_float2(x, y);
    const float cx = r[1], cy = r[J + 1];
    float dx = x - cx;
    if (d.mirror) dx = -dx;
    if (!g.spin) return make_float2(cx + dx, y);
    const float dy = y - cy;
    const float rx = d.c * dx - d.sn * dy;
    const float ry = d.sn * dx + d.c * dy;
    return make_float2(cx + d.s * rx, cy + d.s * ry);
}

// The Lane of bb_run (kernel_build_batch.h) for the augmented build: the sequence's draws, the virtual row's joints,
// the mirrored confidence and the jitter.
struct BaLane {
    const BaArgs& g;
    uint32_t p;               // the draw index: the plan entry, or entry0 + b; below 2^32 by the host's shape rule
    uint64_t seed, epoch;
    BaSeq d;

    __device__ __forceinline__ void draw(const BbArgs& a, int64_t b, bool live) {
        p = (uint32_t)(a.step ? bb_entry(a, b) : g.entry0 + b);
        seed = g.key[0], epoch = g.key[1];                         // wave-uniform: two 8-byte scalar loads
        d = {1.f, 1.f, 0.f, false};
        if (live && (g.spin || g.mirror_thr)) d = ba_sequence(g, p, seed, epoch);
    }
    __device__ __forceinline__ int conf_joint(const BbArgs& a, int src) const {
        return d.mirror ? ba_mirrored(a.n_body, src) : src;
    }
    __device__ __forceinline__ float2 joint(const BbArgs&, const float* r, int J, int q) const {
        return ba_joint(g, d, r, J, q);
    }
    __device__ __forceinline__ void jitter(float2& v, int64_t t, int j) const {
#pragma clang fp contract(off)
        if (g.jitter == 0.f) return;
        uint32_t w[4];
        dm_philox(p, kBaTagJitter | (uint32_t)t << 8, (uint32_t)epoch, (uint32_t)(j >> 1), (uint32_t)seed,
                  (uint32_t)(seed >> 32), w);
        const uint32_t wx = (j & 1) ? w[2] : w[0], wy = (j & 1) ? w[3] : w[1];
        v.x = v.x + g.jitter * ba_unit(wx);
        v.y = v.y + g.jitter * ba_unit(wy);
    }
};

__global__ __launch_bounds__(kBbThreads) void b2h_build_batch_aug_k(const BaArgs g) { bb_run<const BbArgs&>(g.b, BaLane{g}); }

} // namespace b2h
