"""The generator of b2h_dropout_masks (include/b2h.h, kernel_dropout_masks.h) restated in numpy, for
tests/test_dropout_masks_*.py.  A helper module, not a conftest.py: the tests import it by name.

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the constants of its
Random123 library).  Element e of mask number k: word e % 4 of the block with counter (b lo, b hi, k, s), b = e // 4,
s = step mod 2^32, key (seed lo, seed hi); keep = word >= ceil(float32(p) * 2^32)."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U = np.uint64
_LOW = _U(0xFFFFFFFF)
_S32 = _U(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words (uint64 arrays holding 32-bit values) of counter (c0, c1, c2, c3) under key (k0, k1);
    the counter words may be arrays of one length, or scalars."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = _U(M0) * c0, _U(M1) * c2                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ _U(k0)) & _LOW, p1 & _LOW, ((p0 >> _S32) ^ c3 ^ _U(k1)) & _LOW, p0 & _LOW
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def words(numel, number, step, seed):
    """The 32-bit words of the `numel` elements of mask `number` (a uint64 array)."""
    nb = (numel + 3) // 4
    b = np.arange(nb, dtype=np.uint64)
    w = philox4x32_10(b & _LOW, b >> _S32, np.full(nb, number, np.uint64), np.full(nb, step & 0xFFFFFFFF, np.uint64),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack(w, 1).reshape(-1)[:numel]


def threshold(p):
    """ceil(double(float(p)) * 2^32): exact, both factors are doubles and the product has at most 24 + 1 bits."""
    return math.ceil(float(np.float32(p)) * 2.0 ** 32)


def mask(numel, number, step, seed, p):
    """The keep-mask as b2h_dropout_masks writes it: uint8 (numel,), 1 = keep."""
    return (words(numel, number, step, seed) >= _U(threshold(p))).astype(np.uint8)


def masks(sizes, step, seed, p, first_index=0):
    return [mask(n, first_index + i, step, seed, p) for i, n in enumerate(sizes)]
