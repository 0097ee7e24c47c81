// The order and the crop offsets of a whole training epoch, and the word that walks through them (b2h_epoch_plan,
// b2h_epoch_record, include/b2h.h): what torch.randperm and DeviceLoader.draw_starts give the
// eager loop, from a counter-based generator, so that an epoch of captured steps needs no host work between replays.
//
//   b2h_epoch_plan_k    one lane per plan entry i in [0, n_utt); no sort, no atomics, no LDS.
//     utt_plan[i]   = i without `shuffle`, else perm(i): a 4-round balanced Feistel network over [0, 2^(2h)), h the
//                     smallest value >= 1 with 2^(2h) >= n_utt, walked until the value is < n_utt (cycle walking: a
//                     bijection of [0, 2^(2h)) restricted to the orbit's first return to [0, n_utt) is a bijection of
//                     [0, n_utt)).  With mask = 2^h - 1 and x = i:
//                         L = x >> h, R = x & mask
//                         for r = 0 .. 3:  F = word0(Philox(R, 1 + r, epoch lo, epoch hi; seed lo, seed hi)) & mask
//                                          (L, R) = (R, L ^ F)
//                         x = L << h | R;  again while x >= n_utt
//                     2^(2h) < 4 n_utt (n_utt >= 2), so a walk takes fewer than 4 passes on average.
//     start_plan[i] = 0 without `random_crop`, else with len the row count of utterance utt_plan[i],
//                     room = max(len - T, 0) and w = word0(Philox(i, 0, epoch lo, epoch hi; seed lo, seed hi)):
//                     floor(w * (room + 1) / 2^32), uniform in [0, room], 0 when the utterance fits.
//     Philox(c0, c1, c2, c3; k0, k1) is dm_philox of kernel_dropout_masks.h (Philox4x32-10).  Counter word c1 is the
//     tag: 1 .. 4 the Feistel rounds, 0 the crop draws, so no round shares a block with a crop draw.  n_utt <= 2^30:
//     c0 holds R or i in 32 bits.
//
//   b2h_epoch_record_k  one work-item: s = *step; losses[s] = *loss if 0 <= s < n_losses; *step = s + 1.  The only
//                       writer of the step word inside a step, stream-ordered after everything that read it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_dropout_masks.h"

namespace b2h {

constexpr int kEpThreads = 256;
constexpr uint32_t kEpTagCrop = 0, kEpTagRound0 = 1;   // counter word c1: the crop draw; Feistel round r is 1 + r

struct EpArgs {
    const int64_t* offsets;   // (n_utt + 1); read only with random_crop
    int64_t* utt_plan;        // (n_utt)
    int64_t* start_plan;      // (n_utt), or NULL
    int64_t n_utt, T;
    uint32_t key0, key1;      // seed lo, hi
    uint32_t epoch0, epoch1;  // epoch lo, hi
    int h;                    // half width of the Feistel domain, 1 .. 15
    int shuffle, random_crop;
};

__global__ __launch_bounds__(kEpThreads) void b2h_epoch_plan_k(const EpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kEpThreads + threadIdx.x;
    if (i >= a.n_utt) return;
    uint32_t x = (uint32_t)i;
    if (a.shuffle) {
        const uint32_t mask = (1u << a.h) - 1u;
        do {   // ends: the orbit of i under a permutation returns to i < n_utt at the latest
            uint32_t L = x >> a.h, R = x & mask;
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) {
                uint32_t w[4];
                dm_philox(R, kEpTagRound0 + r, a.epoch0, a.epoch1, a.key0, a.key1, w);
                const uint32_t next = L ^ (w[0] & mask);
                L = R;
                R = next;
            }
            x = L << a.h | R;
        } while (x >= (uint64_t)a.n_utt);
    }
    a.utt_plan[i] = (int64_t)x;
    if (!a.start_plan) return;
    int64_t s = 0;
    if (a.random_crop) {
        const int64_t len = a.offsets[(int64_t)x + 1] - a.offsets[x];
        const int64_t room = len > a.T ? len - a.T : 0;
        if (room > 0) {
            uint32_t w[4];
            dm_philox((uint32_t)i, kEpTagCrop, a.epoch0, a.epoch1, a.key0, a.key1, w);
            // floor(w * m / 2^32) with m = room + 1 split in two halves: exact for every m < 2^63
            const uint64_t m = (uint64_t)room + 1u;
            s = (int64_t)((uint64_t)w[0] * (m >> 32) + (((uint64_t)w[0] * (m & 0xffffffffu)) >> 32));
        }
    }
    a.start_plan[i] = s;
}

__global__ void b2h_epoch_record_k(const float* loss, float* losses, int64_t n_losses, int64_t* step) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t s = *step;
    if (s >= 0 && s < n_losses) losses[s] = *loss;
    *step = (int64_t)((uint64_t)s + 1u);   // wraps instead of overflowing
}

} // namespace b2h
