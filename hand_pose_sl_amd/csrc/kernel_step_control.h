// What a training loop does between loss.backward() and optimizer.step() (b2h_step_prepare, include/b2h.h): the global
// L2 norm of every gradient, the clip coefficient of torch.nn.utils.clip_grad_norm_, the decision to skip an update
// whose gradients are not finite, and the warmup of the learning rate, all left in device words that
// b2h_adam_guarded_k (kernel_adam.h) reads, so that a captured step carries them.
//
//   b2h_grad_sumsq_k    partial sums of squares of up to kScMaxTensors gradient tensors.  One flat index runs over the
//                       16-byte chunks (4 floats) of all tensors of a CALL; a launch holds the tensors whose chunks are
//                       first[0] .. first[n] - 1 of it.  The flat index is cut into blocks of kScBlockChunks chunks, and
//                       block b gives partial[b] (fp64).  Inside a block thread j of 256 takes the chunks j, j + 256,
//                       j + 512, j + 768 in this order, each element x as acc = fma(x, x, acc) in double (the product of
//                       two floats is exact in double), x, y, z, w in this order; then a wave butterfly (xor 32, 16, 8,
//                       4, 2, 1), then the four waves' sums through LDS, added in wave order by thread 0.  Chunks of a
//                       block that belong to another launch add nothing here: the launch that holds the first chunk of
//                       a block stores partial[b], a later launch of the same call (stream-ordered after it) adds to
//                       it.  The grid strides over the blocks.  So partial[] is a function of the numel list and the
//                       values alone: not of the grid size, the stream, the device or the pointers' alignment.
//                       A tensor whose pointer is off the 16-byte grid, and the last partial chunk of a tensor, go
//                       element by element, never past numel; whole chunks of aligned tensors are dwordx4 loads.
//   b2h_step_control_k  one workgroup.  Thread j adds partial[j], partial[j + 256], ... in ascending order, then the
//                       same tree; thread 0 evaluates the words listed at b2h_step_prepare in double and stores them.
//
// Pointers, sizes and the chunk prefix travel by value in the kernel arguments (no device table, no copy: capture-safe),
// as AdArgs does.  No atomics: every partial has one writer per launch, every word one writer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "chunk_locator.h"

namespace b2h {

constexpr int kScMaxTensors = 80;     // tensors per launch: 80 * 24 B of tables, 2.0 KB of kernel arguments in all
constexpr int kScThreads = 256;
constexpr int kScBlockChunks = 1024;  // 4 chunks per thread: 4096 floats per partial
constexpr int kScMaxBlocks = 1024;    // larger launches stride over their blocks

enum { kSchedNone = 0, kSchedLinear = 1, kSchedInvSqrt = 2 }; // B2H_SCHED_* of b2h.h

struct SsArgs {
    const float* g[kScMaxTensors];
    int64_t numel[kScMaxTensors];
    int64_t first[kScMaxTensors + 1]; // first[i] = 16-byte chunks of the CALL's tensors before tensor i of this launch
    double* partial;                  // one per block of the call's flat index
    int n;                            // tensors in this launch, 1 .. kScMaxTensors
};
static_assert(sizeof(SsArgs) <= 4096, "the kernel arguments of b2h_grad_sumsq_k must fit in 4 KB");

struct ScArgs {
    const double* partial;
    int64_t n_partial;                // 0 when stage 1 did not run: the norm is then 0
    double max_norm;                  // <= 0: no clipping
    double base_lr;
    const float* base_lr_dev;         // or nullptr
    int64_t warmup;
    int64_t step;
    const int64_t* step_dev;          // or nullptr
    float* norm_out;                  // each output or nullptr
    float* scale_out;
    int64_t* apply_out;
    int64_t* skipped;
    float* lr_out;
    int guard, schedule;
};

// The sum of one value per thread of a 256-thread workgroup, in a fixed order: butterfly inside each wave, then the four
// waves in order.  Every thread calls it; thread 0's result is the sum.  `lds` holds 4 doubles and is free again after
// the caller's next __syncthreads().
__device__ __forceinline__ double sc_block_sum(double acc, double* lds) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ void __launch_bounds__(kScThreads) b2h_grad_sumsq_k(const SsArgs a) {
    __shared__ double lds[4];
    const int64_t lo = a.first[0], hi = a.first[a.n]; // this launch's chunks of the flat index; hi > lo
    const int64_t b0 = lo / kScBlockChunks, b1 = (hi - 1) / kScBlockChunks;
    for (int64_t b = b0 + blockIdx.x; b <= b1; b += gridDim.x) {
        double acc = 0.0;
        for (int k = 0; k < kScBlockChunks / kScThreads; ++k) {
            const int64_t c = b * kScBlockChunks + k * kScThreads + threadIdx.x;
            if (c < lo || c >= hi) continue;
            const int i = chunk_tensor(a.first, a.n, c); // lo = first[0] <= c < hi = first[n]
            const int64_t numel = a.numel[i], e0 = (c - a.first[i]) * 4; // e0 < numel
            const float* gp = a.g[i] + e0;
            if (((uintptr_t)a.g[i] & 15) == 0 && e0 + 4 <= numel) {
                const float4 g4 = *reinterpret_cast<const float4*>(gp);
                acc = fma((double)g4.x, (double)g4.x, acc);
                acc = fma((double)g4.y, (double)g4.y, acc);
                acc = fma((double)g4.z, (double)g4.z, acc);
                acc = fma((double)g4.w, (double)g4.w, acc);
            } else {
                const int count = (int)(numel - e0 < 4 ? numel - e0 : 4); // 1 .. 4
                for (int j = 0; j < count; ++j) {
                    const double x = (double)gp[j];
                    acc = fma(x, x, acc);
                }
            }
        }
        const double sum = sc_block_sum(acc, lds);
        if (threadIdx.x == 0) {
            // a block whose first chunk lies in an earlier launch of the call was stored by it: add to that
            const int64_t begin = b * kScBlockChunks;
            a.partial[b] = begin < lo ? a.partial[b] + sum : sum;
        }
        __syncthreads(); // lds is read by every thread above and written again in the next pass
    }
}

__global__ void __launch_bounds__(kScThreads) b2h_step_control_k(const ScArgs a) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < a.n_partial; j += kScThreads) acc += a.partial[j];
    const double total = sc_block_sum(acc, lds);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(total);
    const int64_t apply = a.guard ? (int64_t)(isfinite(total) ? 1 : 0) : 1;
    float scale = 1.f;
    if (a.max_norm > 0.0) {
        const double c = a.max_norm / (norm + 1e-6); // torch's clip_coef; NaN stays NaN through the clamp, as in torch
        scale = (float)(c >= 1.0 ? 1.0 : c);
    }
    if (!apply) scale = 0.f;
    const int64_t t = a.step + (a.step_dev ? *a.step_dev : 0); // the 1-based index of the update about to be made
    const double base = a.base_lr_dev ? (double)*a.base_lr_dev : a.base_lr, w = (double)a.warmup, td = (double)t;
    double f = 1.0;
    if (a.schedule == kSchedLinear)
        f = t >= a.warmup ? 1.0 : td / w;
    else if (a.schedule == kSchedInvSqrt)
        f = t <= a.warmup ? td / w : sqrt(w / td);
    if (a.norm_out) *a.norm_out = (float)norm;
    if (a.scale_out) *a.scale_out = scale;
    if (a.apply_out) *a.apply_out = apply;
    if (a.skipped) *a.skipped = *a.skipped + (apply ? 0 : 1);
    if (a.lr_out) *a.lr_out = (float)(base * f);
}

} // namespace b2h
