// The key lengths of padded token rows: the reference pads every sentence to S ids with one pad
// value at the end, so a sentence's length is one past its last id that differs from it.
//
//   b2h_token_lengths_k   len[b] = 1 + (last s with tokens[b][s] != pad_id), 1 if every id is pad_id
//
// A pad_id inside the sentence (followed by another id) counts as a token.  One wave per sequence: lane l looks at the
// ids l, l + 64, .. and keeps the last one that is no pad, the wave takes the maximum, lane 0 stores it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace b2h {

// tokens (B, S) int64, len (B) int64.  grid ceil(B / 4), 256 threads (four sequences per workgroup).
__global__ __launch_bounds__(256) void b2h_token_lengths_k(const int64_t* __restrict__ tokens, int64_t B, int S, int64_t pad_id,
                                                         int64_t* __restrict__ len) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return; // (wave-uniform)
    const int64_t* row = tokens + b * S;
    int last = 0; // one past the lane's last id that is no pad
    for (int s = lane; s < S; s += 64)
        if (row[s] != pad_id) last = s + 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
    if (lane == 0) len[b] = last < 1 ? 1 : last;
}

} // namespace b2h
