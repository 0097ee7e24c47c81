// The tensor of a chunk.  The kernels that serve a LIST of tensors in one launch (b2h_adam_step_k, b2h_adam_guarded_k,
// b2h_grad_sumsq_k, b2h_dropout_masks_k) walk one flat index over the 16-byte chunks of all of them; first[i] is the
// number of chunks before tensor i and first[n] the number of all, a table of at most 81 entries in the kernel arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace b2h {

// The i with first[i] <= c < first[i + 1], for first[0] <= c < first[n].  The wave's lowest chunk (its first active lane)
// is searched with wave-uniform reads, then each lane steps past the few tensor ends inside the wave's 64 chunks: it
// ends at i <= n - 1 because c < first[n].  An empty tensor (first[i] == first[i + 1]) is never the answer.
__device__ __forceinline__ int chunk_tensor(const int64_t* first, int n, int64_t c) {
    const int64_t cw = ((int64_t)__builtin_amdgcn_readfirstlane((int)(c >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
    int lo = 0, hi = n; // first[lo] <= cw < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= cw)
            lo = mid;
        else
            hi = mid;
    }
    int i = lo;
    while (c >= first[i + 1]) ++i;
    return i;
}

} // namespace b2h
