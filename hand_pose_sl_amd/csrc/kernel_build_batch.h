// A training batch from the device-resident store (b2h_build_batch, include/b2h.h): the reference builds it per
// utterance on the host -- frame selection, padding and clipping (dataloaders/text_pose_dataset.py:430-476, 652-688),
// WristDifference, ChestDifference, NormalizeFixedFactor and one Build*Item transform (steps/utils.py:180-277, in
// run.py:83-104's order) -- and torch's default collate stacks the items.  Here one launch gathers it.
//
// Store: rows (N, 3 J) fp32, J = n_body + 42, a row = [x * J | y * J | c * J] with the joints n_body body, 21 left
// hand, 21 right hand (n_body 8: the reference's HDF5 row); offsets (U + 1) int64, utterance u owns rows
// offsets[u] .. offsets[u + 1] - 1; tokens (U, S) int64 or none.
//
// The grid is five runs of 256-thread blocks, one per output, so a block serves one output and consecutive lanes store
// to consecutive addresses: input_kp and target_kp one float2 (a joint) per lane, target_conf one float, text_tokens
// and n_frames one int64.  Every output word is written by exactly one lane; nothing is read outside the rows of
// utt[b].  An id outside [0, n_utt), or offsets of it outside 0 <= lo <= hi <= n_rows, indexes nothing: that
// sequence's floats become quiet NaNs, its tokens -1, its n_frames 0.  No LDS, no atomics; indices are 64-bit.
// The body is bb_run below, which b2h_build_batch_aug_k (kernel_build_batch_aug.h) runs too, with a Lane of its own.
//
// b2h_build_batch_planned launches the same kernel with BbArgs::step set: utt and start are then the plan of a whole
// epoch (kernel_epoch_plan.h) and sequence b reads entry *step * B + b of it; a step below 0 or an entry at or past
// n_plan is an unknown utterance, so a replay past the end of the plan is loud.
#pragma once
#include "b2h_common.h"

namespace b2h {

constexpr int kBbThreads = 256;
constexpr int kBbDif = 1, kBbNorm = 2, kBbPadFrame0 = 4;   // B2H_BATCH_* of include/b2h.h

struct BbArgs {
    const float* rows;
    const int64_t* offsets;
    const int64_t* tokens;
    const int64_t* utt;
    const int64_t* start;     // may be NULL: every window starts at 0
    float* input_kp;
    float* target_kp;
    float* target_conf;       // may be NULL
    int64_t* text_tokens;     // NULL iff tokens is
    int64_t* n_frames;
    int64_t n_rows, n_utt, B, T, S;
    int64_t first[6];         // first block of input_kp, target_kp, target_conf, text_tokens, n_frames; the block count
    int n_body, predict, flags, ni, nt;   // ni, nt: joints of an input / a target frame
    float factor;
    // b2h_build_batch_planned: utt and start are an epoch's plan of n_plan entries and sequence b reads entry
    // *step * B + b.  NULL for b2h_build_batch: entry b.
    const int64_t* step;
    int64_t n_plan, n_steps;  // n_steps = ceil(n_plan / B): the steps that have an entry
};

// The entry of utt / start that sequence b reads, or -1 for a planned build whose step has none for it.
__device__ __forceinline__ int64_t bb_entry(const BbArgs& a, int64_t b) {
    if (!a.step) return b;
    const int64_t s = *a.step;                        // wave-uniform: one 8-byte scalar load
    if (s < 0 || s >= a.n_steps) return -1;           // before the product: s * B cannot overflow below n_steps
    const int64_t p = s * a.B + b;
    return p < a.n_plan ? p : -1;
}

// The rows of sequence b: lo = first row of the window, len = rows of the utterance; false for an id the store lacks.
__device__ __forceinline__ bool bb_window(const BbArgs& a, int64_t b, int64_t& lo, int64_t& len) {
    const int64_t e = bb_entry(a, b);
    const int64_t u = e < 0 ? -1 : a.utt[e];
    if (u < 0 || u >= a.n_utt) return false;
    const int64_t r0 = a.offsets[u], r1 = a.offsets[u + 1];
    if (r0 < 0 || r1 < r0 || r1 > a.n_rows) return false;
    len = r1 - r0;
    int64_t s = 0;
    if (len > a.T) {          // select_jsons, text_pose_dataset.py:52-68; a shorter utterance starts at 0
        s = a.start ? a.start[e] : 0;
        s = s < 0 ? 0 : (s > len - a.T ? len - a.T : s);
    }
    lo = r0 + s;
    return true;
}

// The store joint (0 .. J-1) behind joint j of an input frame (target = false) or a target frame.
__device__ __forceinline__ int bb_source(int n_body, int predict, bool target, int j) {
    const int hand = n_body + 21;                     // right-hand joint 0
    if (predict == 0) return target ? hand + j : j;                                       // BuildRightHandItem
    if (predict == 1)                                                                     // BuildIndexItem, n_body 12
        return target ? hand + 5 + j : (j < 12 ? j : (j < 17 ? hand + j - 12 : hand + j - 8));
    return target ? hand + 1 + j : (j < 8 ? hand + 13 + j : (j == 8 ? hand : j - 9));     // Build3fingerItem
}

// What b2h_build_batch_k and b2h_build_batch_aug_k (kernel_build_batch_aug.h) differ in, as the `Lane` of bb_run: the
// value of a live joint, the joint whose confidence is copied, and the jitter.  This one reads the store row as it is.
struct BbPlainLane {
    __device__ __forceinline__ void draw(const BbArgs&, int64_t, bool) {}
    __device__ __forceinline__ int conf_joint(const BbArgs&, int src) const { return src; }
    __device__ __forceinline__ float2 joint(const BbArgs&, const float* r, int J, int q) const {
        return make_float2(r[q], r[J + q]);
    }
    __device__ __forceinline__ void jitter(float2&, int64_t, int) const {}
};

// The body of both build kernels: the five block runs, the frame decomposition, padding, the difference encoding, the
// division and the text_tokens and n_frames runs.  Force-inlined into each __global__ entry point, which keeps its name.
// Contraction is off for the whole body because the augmented build's every operation is one rounding
// (kernel_build_batch_aug.h); the plain build has a subtraction and a division here and nothing that could fuse, with
// the pragma or without.  The pragma is lexical: a Lane's own arithmetic needs its own.
// `Args` is `const BbArgs` or `const BbArgs&`: each kernel hands its arguments over the way its body held them before
// the two were folded (the plain kernel by value, the augmented one as the `b` inside its BaArgs), which keeps hipcc's
// listing of the plain kernel the one it was (profiles/datapath_refactor/).
template <class Args, class Lane> __device__ __forceinline__ void bb_run(Args a, Lane lane) {
#pragma clang fp contract(off)
    const int64_t blk = blockIdx.x;
    const int seg = blk < a.first[1] ? 0 : blk < a.first[2] ? 1 : blk < a.first[3] ? 2 : blk < a.first[4] ? 3 : 4;
    const int64_t i = (blk - a.first[seg]) * kBbThreads + threadIdx.x;
    const float qnan = __int_as_float(0x7fc00000);
    if (seg <= 2) {
        const int nj = seg == 0 ? a.ni : a.nt;
        if (i >= a.B * a.T * nj) return;
        const int64_t f = i / nj;
        const int j = (int)(i - f * nj);
        const int64_t b = f / a.T, t = f - b * a.T;
        int64_t lo, len;
        const bool known = bb_window(a, b, lo, len);
        // frames at or past the utterance's end: zeros, or (B2H_BATCH_PAD_FRAME0) the window's first frame again
        const bool live = known && len > 0 && (t < len || (a.flags & kBbPadFrame0));
        const int64_t row = live ? lo + (t < len ? t : 0) : 0;
        const int J = a.n_body + 42;
        const float* r = a.rows + row * (3 * J);
        const int src = bb_source(a.n_body, a.predict, seg != 0, j);
        lane.draw(a, b, live);
        if (seg == 2) {
            a.target_conf[i] = !known ? qnan : live ? r[2 * J + lane.conf_joint(a, src)] : 0.f;
            return;
        }
        float2 v = make_float2(known ? 0.f : qnan, known ? 0.f : qnan);
        if (live) {
            v = lane.joint(a, r, J, src);
            if (a.flags & kBbDif) {     // the hand minus the RAW body wrist (4), the body minus the chest (1)
                const float2 ref = lane.joint(a, r, J, src < a.n_body ? 1 : 4);
                v.x = v.x - ref.x;
                v.y = v.y - ref.y;
            }
            if (seg == 0) lane.jitter(v, t, j);
            if (a.flags & kBbNorm) { v.x = v.x / a.factor; v.y = v.y / a.factor; }
        }
        reinterpret_cast<float2*>(seg == 0 ? a.input_kp : a.target_kp)[i] = v;
    } else if (seg == 3) {
        if (i >= a.B * a.S) return;
        const int64_t b = i / a.S, s = i - b * a.S;
        const int64_t e = bb_entry(a, b);
        const int64_t u = e < 0 ? -1 : a.utt[e];
        a.text_tokens[i] = (u >= 0 && u < a.n_utt) ? a.tokens[u * a.S + s] : -1;
    } else {
        if (i >= a.B) return;
        int64_t lo, len;
        a.n_frames[i] = bb_window(a, i, lo, len) ? (len < a.T ? len : a.T) : 0;
    }
}

__global__ __launch_bounds__(kBbThreads) void b2h_build_batch_k(const BbArgs a) { bb_run<const BbArgs>(a, BbPlainLane{}); }

} // namespace b2h
