// optimizer.step() of the reference's training loop (b2h_adam_step, include/b2h.h): torch.optim.Adam with
// amsgrad = False, maximize = False and classic L2 weight decay, every tensor of a model in one launch
// (DESIGN.md section 21).
//
//   b2h_adam_step_k  per element, fp32, each line one rounding or one FMA (contraction is switched off inside ad_update
//                    and the FMAs are written out, so the listing is the source's):
//                      g' = fma(wd, p, g)                  only if wd != 0
//                      d  = g' - m;   m = fma(d, 1 - b1, m)
//                      a  = v * b2;   b = (1 - b2) * g';   v = fma(b, g', a)
//                      s  = sqrt(v);  q = s / bc2s;  den = q + eps      (IEEE sqrt and division)
//                      r  = m / den;  p = fma(-step_size, r, p)
//                    bc2s = sqrt(1 - b2^t) and step_size = lr / (1 - b1^t) come from ad_bias below, in double, rounded
//                    to float once; t = step + *step_dev.  The host evaluates them when neither step_dev nor lr_dev is
//                    given, else every thread does, once, before its loop.  Neither device word is written.
//
// A thread updates one 16-byte chunk (4 floats): dwordx4 loads of g, m, v, p and dwordx4 stores of p, m, v; the last
// partial chunk of a tensor, and every chunk of a tensor one of whose four pointers is not 16-byte aligned, goes
// element by element, never past numel.  One launch serves up to kAdMaxTensors tensors whose pointers, sizes and
// chunk-count prefix travel by value in the kernel arguments (no device table, no copy: capture-safe), and the grid
// walks ONE flat chunk index over all of them, as b2h_dropout_masks_k does; chunk_tensor (chunk_locator.h) finds the
// tensor of a chunk.  No LDS, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "chunk_locator.h"

namespace b2h {

constexpr int kAdMaxTensors = 80;  // tensors per launch: 80 * 48 B of tables, 3.9 KB of kernel arguments in all
constexpr int kAdThreads = 256;
constexpr int kAdMaxBlocks = 1024; // 4 workgroups of 4 waves per CU on 256 CUs; larger calls stride over the chunks

struct AdArgs {
    float* p[kAdMaxTensors];
    const float* g[kAdMaxTensors];
    float* m[kAdMaxTensors];
    float* v[kAdMaxTensors];
    int64_t numel[kAdMaxTensors];
    int64_t first[kAdMaxTensors + 1]; // first[i] = 16-byte chunks of the tensors before i; first[n] = all of them
    double b1, b2;                    // the betas as ad_bias takes them
    int64_t step;
    const int64_t* step_dev;          // or nullptr
    const float* lr_dev;              // or nullptr
    int n;                            // tensors in this launch, 1 .. kAdMaxTensors
    float w1, b2f, w2;                // float(1 - b1), float(b2), float(1 - b2)
    float eps, wd, lr;
    float bc2s, step_size;            // ad_bias on the host; used when step_dev and lr_dev are both nullptr
};
static_assert(sizeof(AdArgs) <= 4096, "the kernel arguments of b2h_adam_step_k must fit in 4 KB");

// b^t by squaring: multiplications only, so host and device round alike whatever either compiler contracts.
__host__ __device__ inline double ad_pow(double b, int64_t t) {
    double r = 1.0;
    for (; t > 0; t >>= 1, b *= b)
        if (t & 1) r *= b;
    return r;
}

// The two step-dependent scalars of Adam at step t >= 1: sqrt(bias_correction2) and lr / bias_correction1, in double
// as torch's Python evaluates them, each rounded to float once.
__host__ __device__ inline void ad_bias(double b1, double b2, double lr, int64_t t, float* bc2s, float* step_size) {
    const double bc1 = 1.0 - ad_pow(b1, t), bc2 = 1.0 - ad_pow(b2, t);
    *bc2s = (float)sqrt(bc2);
    *step_size = (float)(lr / bc1);
}

struct AdScalars {
    float w1, b2, w2, eps, wd, bc2s, neg_step;
};

__device__ __forceinline__ void ad_update(float& p, float g, float& m, float& v, const AdScalars& s) {
#pragma clang fp contract(off) // this function only: a pragma at file scope would reach the kernels included later
    if (s.wd != 0.f) g = __builtin_fmaf(s.wd, p, g);
    const float d = g - m;
    m = __builtin_fmaf(d, s.w1, m);
    const float a = v * s.b2;
    const float b = s.w2 * g;
    v = __builtin_fmaf(b, g, a);
    const float r = __builtin_sqrtf(v);
    const float q = r / s.bc2s;
    const float den = q + s.eps;
    const float u = m / den;
    p = __builtin_fmaf(s.neg_step, u, p);
}

// b2h_adam_step_guarded: the update above behind the two device words of b2h_step_prepare (kernel_step_control.h).
//   b2h_adam_guarded_k  the same listing per element through ad_update, after
//                         g <- g * *grad_scale_dev        one fp32 rounding, as g.mul_(clip_coef) in torch
//                       and every thread returns before it touches memory when *apply_dev == 0 (a wave-uniform read).
//                       Either word may be nullptr: no scaling, no guard.
struct AdGuard {
    const float* grad_scale_dev; // or nullptr
    const int64_t* apply_dev;    // or nullptr
};
static_assert(sizeof(AdArgs) + sizeof(AdGuard) <= 4096, "the kernel arguments of b2h_adam_guarded_k must fit in 4 KB");

__device__ __forceinline__ float ad_scale(float g, float s) {
#pragma clang fp contract(off) // the product is rounded before ad_update sees it
    return g * s;
}

// The loop of both kernels.  kMayScale is the compile-time half of "is the gradient scaled": false for
// b2h_adam_step_k, whose instantiation has no scale, no test of one and no multiply; true for b2h_adam_guarded_k, where
// `scaled` (is there a scale word) and gs (its value) are the run-time half.  Force-inlined into two __global__
// functions that keep their names: the tests and tools find them by mangled name, and a listing per entry point is what
// tests/test_adam_cpu.py and tests/test_step_control_cpu.py count loads, stores and divisions in.  `a` by value, as the
// kernels hold it: no copy is made (the table stays in the kernel arguments) and hipcc's prologue stays what it was.
template <bool kMayScale> __device__ __forceinline__ void ad_run(const AdArgs a, bool scaled, float gs) {
    const int64_t total = a.first[a.n], stride = (int64_t)gridDim.x * kAdThreads;
    AdScalars s{a.w1, a.b2f, a.w2, a.eps, a.wd, a.bc2s, -a.step_size};
    if (a.step_dev || a.lr_dev) { // wave-uniform reads of the two words
        const int64_t t = a.step + (a.step_dev ? *a.step_dev : 0);
        float step_size;
        ad_bias(a.b1, a.b2, (double)(a.lr_dev ? *a.lr_dev : a.lr), t, &s.bc2s, &step_size);
        s.neg_step = -step_size;
    }
    for (int64_t c = (int64_t)blockIdx.x * kAdThreads + threadIdx.x; c < total; c += stride) {
        const int i = chunk_tensor(a.first, a.n, c);
        const int64_t numel = a.numel[i], e0 = (c - a.first[i]) * 4; // e0 < numel: a chunk exists only where elements do
        float* pp = a.p[i] + e0;
        const float* gp = a.g[i] + e0;
        float* mp = a.m[i] + e0;
        float* vp = a.v[i] + e0;
        const bool aligned = (((uintptr_t)a.p[i] | (uintptr_t)a.g[i] | (uintptr_t)a.m[i] | (uintptr_t)a.v[i]) & 15) == 0;
        if (aligned && e0 + 4 <= numel) {
            float4 g4 = *reinterpret_cast<const float4*>(gp);
            float4 m4 = *reinterpret_cast<const float4*>(mp), v4 = *reinterpret_cast<const float4*>(vp),
                   p4 = *reinterpret_cast<const float4*>(pp);
            if (kMayScale && scaled)
                g4 = make_float4(ad_scale(g4.x, gs), ad_scale(g4.y, gs), ad_scale(g4.z, gs), ad_scale(g4.w, gs));
            ad_update(p4.x, g4.x, m4.x, v4.x, s);
            ad_update(p4.y, g4.y, m4.y, v4.y, s);
            ad_update(p4.z, g4.z, m4.z, v4.z, s);
            ad_update(p4.w, g4.w, m4.w, v4.w, s);
            *reinterpret_cast<float4*>(pp) = p4;
            *reinterpret_cast<float4*>(mp) = m4;
            *reinterpret_cast<float4*>(vp) = v4;
        } else {
            const int count = (int)(numel - e0 < 4 ? numel - e0 : 4); // 1 .. 4
            for (int j = 0; j < count; ++j) {
                float p = pp[j], m = mp[j], v = vp[j];
                ad_update(p, kMayScale && scaled ? ad_scale(gp[j], gs) : gp[j], m, v, s);
                pp[j] = p;
                mp[j] = m;
                vp[j] = v;
            }
        }
    }
}

__global__ void __launch_bounds__(kAdThreads) b2h_adam_step_k(const AdArgs a) { ad_run<false>(a, false, 1.f); }

__global__ void __launch_bounds__(kAdThreads) b2h_adam_guarded_k(const AdArgs a, const AdGuard w) {
    if (w.apply_dev && *w.apply_dev == 0) return;
    const bool scaled = w.grad_scale_dev != nullptr;
    ad_run<true>(a, scaled, scaled ? *w.grad_scale_dev : 1.f);
}

} // namespace b2h
