// The inference half of the device-resident store (b2h_scatter_rows, b2h_joint_error, include/b2h.h): the reference's
// whole-store caller (infer_utterance_h5.py -> steps/traintest.py:332-391) runs a model over every utterance and writes
// the predictions out as store rows; it multiplies by the factor only and leaves "add the wrist back" as a TODO
// (traintest.py:275-279).  Here one launch writes a batch of predictions back into rows, the inverse of
// b2h_build_batch_k's target transform, and two small launches give the per-utterance, per-joint pixel error of one store
// against another.
//
// b2h_scatter_rows_k: one lane per (b, t, j) of pred (B, T, nt, 2); consecutive lanes load consecutive float2 and store
// to consecutive joints of a row.  The window of utt[b] is bb_window's, the destination joint bb_source's (target side),
// so a frame that b2h_build_batch_k read as target_kp[b, t, j] is the frame this kernel writes.  A lane writes iff the
// utterance is known, len > 0 and max(skip[b], 0) <= t < min(len, T): padded frames, frames an earlier window of the plan
// covered and unknown utterances write nothing.  v = pred, * factor (B2H_BATCH_NORMALIZE), + the raw wrist of the same row
// of `rows` (B2H_BATCH_DIF_ENCODING), each a separate correctly rounded fp32 operation (no contraction to an fma); three
// dword stores x, y, conf.  No LDS, no atomics; indices are 64-bit.
//
// The arithmetic of both kernels is stated as float32 operations that numpy repeats bit for bit.  hipcc's __fmul_rn,
// __fadd_rn and __fsub_rn are plain * + - here (its headers give the rounded OCML forms only under
// OCML_BASIC_ROUNDED_OPERATIONS), which -ffp-contract's default may still fuse, and its __fsqrt_rn is the native
// square root, one ulp off in places.  So each kernel body switches contraction off with the pragma -- that is what
// keeps the named intrinsics apart -- and the square root is sqrtf, which hipcc rounds correctly by default
// (-fhip-fp32-correctly-rounded-divide-sqrt, as kernel_build_batch.h relies on for its division).
//
// b2h_joint_error_k: one lane per (utterance, right-hand joint), the 21 joints of an utterance on neighbouring lanes
// reading neighbouring floats; rows in ascending order into one fp32 accumulator, so the sum has one order.
// b2h_joint_total_k: one lane per joint, utterances in ascending order into a double.  No atomics in either.
#pragma once
#include "kernel_build_batch.h"

namespace b2h {

struct SrArgs {
    BbArgs w;                 // the store, utt, start, B, T, n_body, predict, flags, nt, factor; step NULL
    const int64_t* skip;      // may be NULL: every window is written from its frame 0
    const float* pred;
    float* rows_out;
    float conf;
};

__global__ __launch_bounds__(kBbThreads) void b2h_scatter_rows_k(const SrArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kBbThreads + threadIdx.x;
    const int nt = a.w.nt;
    if (i >= a.w.B * a.w.T * nt) return;
    const int64_t f = i / nt;
    const int j = (int)(i - f * nt);
    const int64_t b = f / a.w.T, t = f - b * a.w.T;
    int64_t lo, len;
    if (!bb_window(a.w, b, lo, len)) return;
    const int64_t n = len < a.w.T ? len : a.w.T;
    int64_t first = a.skip ? a.skip[b] : 0;
    first = first < 0 ? 0 : first;
    if (len <= 0 || t < first || t >= n) return;
    const int J = a.w.n_body + 42;
    const int64_t row = lo + t;                       // < offsets[u + 1] <= n_rows: lo + T <= the utterance's end if len > T
    const int d = bb_source(a.w.n_body, a.w.predict, true, j);
    float2 v = reinterpret_cast<const float2*>(a.pred)[i];
    if (a.w.flags & kBbNorm) {
        v.x = __fmul_rn(v.x, a.w.factor);
        v.y = __fmul_rn(v.y, a.w.factor);
    }
    if (a.w.flags & kBbDif) {                         // the RAW body wrist (4) that b2h_build_batch_k subtracted
        const float* r = a.w.rows + row * (3 * J);
        v.x = __fadd_rn(v.x, r[4]);
        v.y = __fadd_rn(v.y, r[J + 4]);
    }
    float* o = a.rows_out + row * (3 * J);
    o[d] = v.x;
    o[J + d] = v.y;
    o[2 * J + d] = a.conf;
}

constexpr int kJeThreads = 256;
constexpr int kJeJoints = 21;

struct JeArgs {
    const float* rows_pred;
    const float* rows_true;
    const int64_t* offsets;
    float* utt_sum;           // (n_utt, 21)
    int32_t* utt_count;       // (n_utt, 21)
    double* total_sum;        // (21)
    int64_t* total_count;     // (21)
    int64_t n_rows, n_utt;
    int n_body;
};

__global__ __launch_bounds__(kJeThreads) void b2h_joint_error_k(const JeArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kJeThreads + threadIdx.x;
    if (i >= a.n_utt * kJeJoints) return;
    const int64_t u = i / kJeJoints;
    const int j = (int)(i - u * kJeJoints);
    int64_t r0 = a.offsets[u], r1 = a.offsets[u + 1];
    if (r0 < 0 || r1 < r0 || r1 > a.n_rows) r1 = r0 = 0;      // offsets that index nothing: an empty utterance
    const int J = a.n_body + 42;
    const int src = a.n_body + 21 + j;
    float sum = 0.f;
    int32_t count = 0;
    for (int64_t row = r0; row < r1; ++row) {
        const float* p = a.rows_pred + row * (3 * J);
        const float* q = a.rows_true + row * (3 * J);
        if (!(q[2 * J + src] > 0.f)) continue;                // OpenPose writes confidence 0 for a joint it did not find
        const float dx = __fsub_rn(p[src], q[src]), dy = __fsub_rn(p[J + src], q[J + src]);
        sum = __fadd_rn(sum, sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy))));
        ++count;
    }
    a.utt_sum[i] = sum;
    a.utt_count[i] = count;
}

__global__ __launch_bounds__(64) void b2h_joint_total_k(const JeArgs a) {
    const int j = threadIdx.x;
    if (j >= kJeJoints) return;
    double sum = 0.0;
    int64_t count = 0;
    for (int64_t u = 0; u < a.n_utt; ++u) {
        sum += (double)a.utt_sum[u * kJeJoints + j];
        count += a.utt_count[u * kJeJoints + j];
    }
    a.total_sum[j] = sum;
    a.total_count[j] = count;
}

} // namespace b2h
