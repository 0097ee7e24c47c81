// The dropout keep-masks of a training step (b2h_dropout_masks, include/b2h.h): uint8, 1 = keep, drawn by a
// counter-based generator so that a byte depends on (seed, step, mask number, element, p) only -- never on the grid,
// on how many masks share a launch or on another mask's size.
//
//   b2h_dropout_masks_k  Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): element e of mask number k
//                        is output word e % 4 of the block with counter (b lo, b hi, k, s), b = e / 4, and key
//                        (seed lo, seed hi); keep = word >= thr, thr = ceil(p * 2^32) compared in 64 bits (2^32 at
//                        p = 1: nothing is kept).  s = step + *step_dev (mod 2^32), the device word only read.
//
// A thread makes one 16-byte chunk: four blocks, one 16-byte store; the last chunk of a mask whose size is no
// multiple of 16 is stored byte by byte up to numel.  One launch serves up to kDmMaxMasks masks whose pointers, sizes
// and chunk-count prefix travel by value in the kernel arguments (no device table, no copy: capture-safe).  The grid
// walks ONE flat chunk index over all masks of the launch, so a 20 MB attention mask and a 0.8 MB one share the
// machine instead of queueing.  No LDS, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "chunk_locator.h"

namespace b2h {

constexpr int kDmMaxMasks = 64;    // masks per launch: 3 * 64 * 8 B of tables in the kernel arguments
constexpr int kDmThreads = 256;
constexpr int kDmMaxBlocks = 1024; // 4 workgroups of 4 waves per CU on 256 CUs; larger calls stride over the chunks

struct DmArgs {
    uint8_t* ptr[kDmMaxMasks];
    int64_t numel[kDmMaxMasks];
    int64_t first[kDmMaxMasks + 1]; // first[i] = 16-byte chunks of the masks before i; first[n] = all of them
    int n;                          // masks in this launch, 1 .. kDmMaxMasks
    uint32_t number0;               // the mask number of ptr[0]
    uint32_t key0, key1;            // seed lo, hi
    uint64_t thr;                   // ceil(p * 2^32), 0 .. 2^32
    uint64_t step;
    const uint64_t* step_dev;       // or nullptr
};

// One Philox4x32-10 block: ten rounds, the key bumped between them.  (uint64_t)a * b is one v_mad_u64_u32, the high
// and the low half of a round's product together.
__device__ __forceinline__ void dm_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                          uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__global__ void __launch_bounds__(kDmThreads) b2h_dropout_masks_k(const DmArgs a) {
    const int64_t total = a.first[a.n], stride = (int64_t)gridDim.x * kDmThreads;
    const uint32_t s = (uint32_t)(a.step + (a.step_dev ? *a.step_dev : 0));
    for (int64_t c = (int64_t)blockIdx.x * kDmThreads + threadIdx.x; c < total; c += stride) {
        const int i = chunk_tensor(a.first, a.n, c); // the mask of chunk c
        const int64_t numel = a.numel[i], e0 = (c - a.first[i]) * 16;
        uint8_t* dst = a.ptr[i] + e0;
        const uint32_t number = a.number0 + (uint32_t)i;
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t b = (uint64_t)(e0 >> 2) + j;
            uint32_t r[4];
            dm_philox((uint32_t)b, (uint32_t)(b >> 32), number, s, a.key0, a.key1, r);
            w[j] = (uint32_t)(r[0] >= a.thr) | (uint32_t)(r[1] >= a.thr) << 8 | (uint32_t)(r[2] >= a.thr) << 16 |
                   (uint32_t)(r[3] >= a.thr) << 24;
        }
        if (e0 + 16 <= numel) {
            *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            const int tail = (int)(numel - e0); // 1 .. 15: a chunk exists only where the mask has bytes
#pragma unroll
            for (int j = 0; j < 15; ++j) // unrolled: w stays in registers
                if (j < tail) dst[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

} // namespace b2h
