"""The epoch plan of b2h_epoch_plan (include/b2h.h, kernel_epoch_plan.h) restated in plain Python integers on top of
tests/philox_ref.py, for tests/test_graph_trainer_*.py.  A helper module, not a conftest.py: the tests import it by name.

P(c, tag) = word 0 of the Philox4x32-10 block with counter (c, tag, epoch lo, epoch hi) and key (seed lo, seed hi);
tags 1 .. 4 are the four Feistel rounds, tag 0 the crop draws."""
import numpy as np

import philox_ref

TAG_CROP, TAG_ROUND0 = 0, 1
_M = 0xFFFFFFFF


def half_width(n):
    """The smallest h >= 1 with 2^(2h) >= n."""
    h = 1
    while (1 << (2 * h)) < n:
        h += 1
    return h


def _p(c, tag, seed, epoch):
    c = np.asarray(c, dtype=np.uint64)
    full = lambda v: np.full(c.shape, v, np.uint64)
    return philox_ref.philox4x32_10(c, full(tag), full(epoch & _M), full((epoch >> 32) & _M), seed & _M, (seed >> 32) & _M)[0]


def _pass(x, h, seed, epoch):
    """One pass of the 4-round balanced Feistel network over the uint64 array x of values below 2^(2h)."""
    mask = np.uint64((1 << h) - 1)
    L, R = x >> np.uint64(h), x & mask
    for r in range(4):
        L, R = R, L ^ (_p(R, TAG_ROUND0 + r, seed, epoch) & mask)
    return (L << np.uint64(h)) | R


def order(n, shuffle, seed, epoch):
    """utt_plan: a list of n ints."""
    if not shuffle or n == 0:
        return list(range(n))
    h = half_width(n)
    x = _pass(np.arange(n, dtype=np.uint64), h, seed, epoch)
    for _ in range(4 << (2 * h)):                 # cycle walking: an orbit is no longer than the domain
        out = x >= np.uint64(n)
        if not out.any():
            return [int(v) for v in x]
        x[out] = _pass(x[out], h, seed, epoch)
    raise AssertionError("cycle walking did not end: the network is not a bijection")


def starts(offsets, utt_plan, T, random_crop, seed, epoch):
    """start_plan: a list of len(utt_plan) ints; `offsets` the store's (n_utt + 1) ascending ints."""
    n = len(utt_plan)
    if not random_crop or n == 0:
        return [0] * n
    w = _p(np.arange(n, dtype=np.uint64), TAG_CROP, seed, epoch)
    out = []
    for i, u in enumerate(utt_plan):
        room = max(int(offsets[u + 1]) - int(offsets[u]) - T, 0)
        out.append((int(w[i]) * (room + 1)) >> 32)
    return out


def plan(offsets, n, T, shuffle, random_crop, seed, epoch):
    utt = order(n, shuffle, seed, epoch)
    return utt, starts(offsets, utt, T, random_crop, seed, epoch)
