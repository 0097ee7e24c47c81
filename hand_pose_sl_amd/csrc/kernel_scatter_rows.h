// The inference half of the device-resident store (b2h_scatter_rows, b2h_scatter_rows_blend, b2h_joint_error,
// include/b2h.h): the reference's whole-store caller (infer_utterance_h5.py -> steps/traintest.py:332-391) runs a
// model over every utterance and writes the predictions out as store rows; it multiplies by the factor only and leaves "add the wrist back" as a TODO
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
// dword stores x, y, conf.  No LDS, no atomics; indices are 64-bit.  b2h_scatter_rows_blend_k (below) is the same
// write-back for a plan of overlapping windows.
//
// The arithmetic of both kernels is stated as float32 operations that numpy repeats bit for bit.  hipcc's __fmul_rn,
// __fadd_rn and __fsub_rn are plain * + - here (its headers give the rounded OCML forms only under
// OCML_BASIC_ROUNDED_OPERATIONS), which -ffp-contract's default may still fuse, and its __fsqrt_rn is the native
// square root, one ulp off in places.  So each kernel body switches contraction off with the pragma -- that is what
// keeps the named intrinsics apart in the kernels' shared tail and in b2h_joint_error_k; the blend's
// fl(fl(wa pa) + fl(wb pb)) still came out as a packed fma with them, so it is written with plain operators, which the
// pragma covers lexically -- and the square root is sqrtf, which hipcc rounds correctly by default
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

// The tail both write-back kernels share: value v of target joint j into row `row` of rows_out.
__device__ __forceinline__ void sr_store(const SrArgs& a, int64_t row, int j, float2 v) {
#pragma clang fp contract(off)
    const int J = a.w.n_body + 42;
    const int d = bb_source(a.w.n_body, a.w.predict, true, j);
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
    // row lo + t < offsets[u + 1] <= n_rows: lo + T <= the utterance's end if len > T
    sr_store(a, lo + t, j, reinterpret_cast<const float2*>(a.pred)[i]);
}

// b2h_scatter_rows_blend_k: the write-back of a plan whose windows overlap (b2h_window_plan_overlap).  The batch holds
// entries entry0 .. entry0 + B - 1 of the plan in s.w.utt / s.w.start / s.skip (n_plan entries each); one lane per
// (b, t, j) as above.  Entry e's predecessor is e - 1 if it has the same utterance, its successor e + 1 likewise; their
// windows come from bb_window too, so every start is the clamped one.  A lane writes iff skip[e] <= t < end, end =
// min(len, T) without a successor, else the frame at which the successor's used frames begin: the tail that the
// successor blends is the successor's, so every row has one writer in one launch and the launches may run in any order.
// The first w = (predecessor's window end) - (first used row) used frames are the blend region: there the lane reads
// the predecessor's value of the same row, a second float2 stream at the fixed offset (start[e] - start[e-1] - T) frames
// in `pred`, or `before` (the predecessor's (T, nt, 2) block) for b == 0.  LINEAR: wb = fl((p + 1) / (w + 1)),
// wa = fl(1 - wb), v = fl(fl(wa pa) + fl(wb pb)); CENTRE: v = 2 p >= w ? pb : pa.  `before` NULL: entry0 is written as
// if it had no predecessor (nothing is read through it).
struct SbArgs {
    SrArgs s;
    const float* before;      // may be NULL
    int64_t entry0, n_plan;
    int blend;                // 0 linear, 1 centre
};

__global__ __launch_bounds__(kBbThreads) void b2h_scatter_rows_blend_k(const SbArgs a) {
#pragma clang fp contract(off)
    const BbArgs& w = a.s.w;
    const int64_t i = (int64_t)blockIdx.x * kBbThreads + threadIdx.x;
    const int nt = w.nt;
    if (i >= w.B * w.T * nt) return;
    const int64_t f = i / nt;
    const int j = (int)(i - f * nt);
    const int64_t b = f / w.T, t = f - b * w.T;
    const int64_t e = a.entry0 + b;                   // < n_plan: the host checked entry0 + B <= n_plan
    int64_t lo, len;
    if (!bb_window(w, e, lo, len)) return;
    const int64_t n = len < w.T ? len : w.T;
    int64_t first = a.s.skip[e];
    first = first < 0 ? 0 : first;
    if (len <= 0 || t < first || t >= n) return;
    const int64_t u = w.utt[e];
    int64_t lo2, len2;
    if (e + 1 < a.n_plan && w.utt[e + 1] == u && bb_window(w, e + 1, lo2, len2)) {
        const int64_t skip2 = a.s.skip[e + 1];
        if (t >= lo2 + (skip2 < 0 ? 0 : skip2) - lo) return;      // the successor's frame
    }
    float2 v = reinterpret_cast<const float2*>(a.s.pred)[i];
    if (e > 0 && (b > 0 || a.before) && w.utt[e - 1] == u && bb_window(w, e - 1, lo2, len2)) {
        const int64_t ta = t + (lo - lo2);            // this row's frame in the predecessor's window
        const int64_t width = lo2 + w.T - (lo + first), p = t - first;
        if (p < width && ta >= 0) {                   // p < width is ta < T
            const float2 pa = b > 0 ? reinterpret_cast<const float2*>(a.s.pred)[i + (lo - lo2 - w.T) * nt]
                                    : reinterpret_cast<const float2*>(a.before)[ta * nt + j];
            if (a.blend == 0) {
                // plain operators, which the pragma above covers: the __f*_rn functions are inlined from a header
                // it does not reach, and a product and a sum that both come from there fuse into one fma
                const float wb = (float)(p + 1) / (float)(width + 1);
                const float wa = 1.f - wb;
                const float ax = wa * pa.x, ay = wa * pa.y, bx = wb * v.x, by = wb * v.y;
                v.x = ax + bx;
                v.y = ay + by;
            } else if (2 * p < width) {
                v = pa;
            }
        }
    }
    sr_store(a.s, lo + t, j, v);
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
