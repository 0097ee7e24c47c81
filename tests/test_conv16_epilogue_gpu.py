"""The ReLU layers' epilogue and tile schedule of the persistent bf16/f16 kernel (kernel_mfma16.h): ReLU is taken on
the packed 16-bit pairs after the cast, the last tile's padding mask on the packed dwords, and the order of a
tile's MFMAs, epilogue, write and fragment reads is pinned, with the address registers advancing inside the loop
body.  A crafted model makes every intermediate a small dyadic number (exact in bf16 and f16, so the fp32 oracle's
output is exact and the kernel must EQUAL it) and makes every frame depend on whether the frames before 0 and from
T on were zero: a wrong mask, a ReLU that lets a negative through, or a fragment read on the wrong side of the
write it depends on each change an integer."""
import functools

import numpy as np
import pytest
import torch

import oracle
from poison import POISON
from test_gpu_parity import _model, _poisoned

gpu = pytest.mark.gpu

PRECS = ["bf16", "f16"]
C = 30
BIASES = [-3.0, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 2.0, 3.0]
# every tail length of a two-tile and of a four-tile loop body, whole (<= 208) and split sequences
LENGTHS = [1, 2, 3, 15, 16, 17, 31, 33, 47, 49, 63, 65, 81, 97, 113, 129, 200, 207, 208, 209, 385]


def _crafted_state():
    """Layer 1: zero weights, the biases above in turn (so the input does not matter, unless it is read under a
    zero weight as NaN); layers 2 and 3: each channel the sum of its own five taps, bias -1 and 0; head: output o
    is channel o % 30 at the centre tap."""
    w1 = np.zeros((C, 24, 5), np.float32)
    b1 = np.array([BIASES[c % len(BIASES)] for c in range(C)], np.float32)
    w = np.zeros((C, C, 5), np.float32)
    w[np.arange(C), np.arange(C), :] = 1.0
    w4 = np.zeros((42, C, 5), np.float32)
    w4[np.arange(42), np.arange(42) % C, 2] = 1.0
    return {"conv1.weight": w1, "conv1.bias": b1,
            "conv2.weight": w, "conv2.bias": np.full(C, -1.0, np.float32),
            "conv3.weight": w.copy(), "conv3.bias": np.zeros(C, np.float32),
            "conv4.weight": w4, "conv4.bias": np.zeros(42, np.float32)}


REC = {"C": C, "pos_emb": False, "state": _crafted_state()}


def _input(B, T, seed):
    return torch.rand((B, T, 12, 2), generator=torch.Generator().manual_seed(seed)) - 0.5


@functools.lru_cache(maxsize=None)
def _expected(T):
    """The fp32 oracle on three sequences of length T (computed once per length; read-only)."""
    y = oracle.forward_from_state(_input(3, T, 5000 + T).numpy(), REC["state"])
    y.setflags(write=False)
    return y


def _all_written(y):
    return not bool((y.view(torch.int32) == torch.tensor(POISON, dtype=torch.int32)).any())


@pytest.mark.parametrize("T", [1, 2, 3, 17, 200, 209])
def test_oracle_output_is_dyadic(T):
    """(CPU) What the GPU cases compare with: the oracle alone gives integers or halves, at most 70, the same for
    every sequence, and the sequence ends show in it."""
    y = _expected(T)
    assert np.array_equal(y * 2, np.round(y * 2)) and y.min() >= 0 and y.max() <= 70
    assert np.array_equal(y[0], y[1]) and np.array_equal(y[0], y[2])
    # channel 8 (bias 3): layer 2 = 3 n2 - 1 and layer 3 its sum over the taps inside [0, T)
    n2 = np.array([min(t + 2, T - 1) - max(t - 2, 0) + 1 for t in range(T)])
    l2 = np.maximum(3.0 * n2 - 1.0, 0.0)
    l3 = np.array([l2[max(t - 2, 0):min(t + 2, T - 1) + 1].sum() for t in range(T)])
    assert np.array_equal(y[0].reshape(T, 42)[:, 8], l3)
    assert np.array_equal(y[0].reshape(T, 42)[:, 38], l3)      # output 38 = channel 8 again
    assert not y[0].reshape(T, 42)[:, :5].any()                # biases <= 0 stay 0 through the ReLUs


@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("T", LENGTHS)
def test_exact_relu_and_padding(T, prec, cuda_device):
    """B = 3 into a poisoned buffer: every row written and equal to the oracle bit for bit."""
    m = _model(REC, prec, cuda_device)
    x = _input(3, T, 5000 + T).to(cuda_device)
    with torch.no_grad():
        y = m.forward_into(x, _poisoned(torch.empty((3, T, 21, 2), device=cuda_device)))
    assert _all_written(y), (prec, T)
    y = y.cpu().numpy()
    want = _expected(T)
    bad = np.argwhere(y != want)
    assert np.array_equal(y, want), (prec, T, len(bad), bad[:4].tolist())


@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("T", [5, 40])
def test_image_reuse_across_chunks(T, poison, prec, cuda_device):
    """8 192 sequences in a static launch: four chunks per wave, one after the other in the wave's one LDS image.
    Every clean sequence equals the B = 3 result row for row, also when a random half of the others is all NaN
    and +-Inf -- layer 1 multiplies them by zero weights, so a read on the wrong side of a write shows as NaN."""
    B = 8192
    g = torch.Generator().manual_seed(31 * T + poison)
    x = torch.rand((B, T, 12, 2), generator=g) - 0.5
    bad = torch.zeros(B, dtype=torch.bool)
    if poison:
        bad = torch.rand(B, generator=g) < 0.5
        n_bad = int(bad.sum())
        assert 0 < n_bad < B
        x[bad] = torch.tensor([float("nan"), float("inf"), float("-inf")])[torch.randint(0, 3, (n_bad, T, 12, 2), generator=g)]
    m = _model(REC, prec, cuda_device)
    with torch.no_grad():
        small = m(_input(3, T, 5000 + T).to(cuda_device))
        y = m.forward_into(x.to(cuda_device), _poisoned(torch.empty((B, T, 21, 2), device=cuda_device)))
    assert _all_written(y), (prec, T)
    assert np.array_equal(small.cpu().numpy(), _expected(T)), (prec, T)
    clean = y[(~bad).to(cuda_device)]
    assert bool(torch.isfinite(clean).all()), (prec, T)
    assert torch.equal(clean, small[:1].expand_as(clean)), (prec, T)
