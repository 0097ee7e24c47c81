"""TransformerEnc training without a GPU: the new C ABI entry points are declared, typed and exported; the
checker of the GPU tests (tenc_train_ref.port_forward) is pinned to the reference class through the fixtures
(tests/golden/train/tenc_grad_*.npz, p = 0) and to the inference vectors (tenc_cases.npz, eval mode), and its
dropout follows torch's definition; the new kernels compile without scratch or spills."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from kernel_remarks import kernel_remarks
from tenc_train_ref import (NAMES, leaf_state, load_tenc, masked_l1, param_keys, port_forward, seeded_state,
                            tenc_cases)

NEW = ["b2h_tenc_train_bytes", "b2h_tenc_train_forward", "b2h_tenc_backward"]


def test_symbols_declared_typed_exported():
    from hand_pose_sl_amd import _lib
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/b2h.h"
        assert n in _lib.SYMBOLS, f"{n} not typed in _lib.SYMBOLS"
        assert hasattr(lib, n), f"{n} not exported by libb2h.so"
    for cite in ("HandPoseModels.py:154-178", "traintest.py:87-121", "steps/utils.py:309-312"):
        assert cite in header


def test_entry_points_reject_null_arguments_without_gpu():
    from hand_pose_sl_amd import _lib
    lib = _lib.load()
    ptrs = (ctypes.c_void_p * 17)()
    assert lib.b2h_tenc_train_forward(None, ptrs, None, None, 0.0, None, None, 0, 1, 1, None) == _lib.ERR_INVALID
    assert lib.b2h_tenc_train_forward(None, None, None, None, 0.0, None, None, 0, 1, 1, None) == _lib.ERR_INVALID
    assert lib.b2h_tenc_backward(None, ptrs, None, 0.0, None, None, 0, None, ptrs, None, 0, 1, 1, None) == _lib.ERR_INVALID
    assert lib.b2h_tenc_train_bytes(None, 1, 1, 0) == 0 and lib.b2h_tenc_train_bytes(None, 1, 1, 1) == 0


@pytest.mark.parametrize("name", tenc_cases())
def test_port_reproduces_reference_fixture(name):
    """Float64 autograd through port_forward at p = 0 == the reference class in .train() with dropout 0."""
    r = load_tenc(name)
    st = leaf_state(r["state"], torch.float64)
    x = torch.from_numpy(r["x"]).double().requires_grad_(True)
    y = port_forward(x, st, {}, 0.0, torch.float64)
    loss = masked_l1(y, torch.from_numpy(r["target"]).double(), r["lengths"])
    loss.backward()
    assert abs(loss.item() - float(r["loss64"])) <= 1e-12 * abs(float(r["loss64"]))
    for k in param_keys(r["nlayers"]):
        g64 = r["g64_" + k]
        # rtol 1e-9 per element, plus a floor of 1e-12 of the tensor's largest gradient (as test_train_cpu.py has it):
        # the key third of in_proj_bias has a gradient that is exactly zero in mathematics (a bias on every key
        # shifts a softmax row by a constant), so both float64 runs hold rounding noise of ~1e-20 there, which no
        # relative bound can compare (measured without the floor: 127 of 384 elements off, the largest by 6.8e-20)
        np.testing.assert_allclose(st[k].grad.numpy(), g64, rtol=1e-9, atol=1e-12 * np.abs(g64).max(), err_msg=k)
        assert 0 < float(r["err32_" + k]) < 1e-3 * np.abs(g64).max() + 1e-12
    np.testing.assert_allclose(x.grad.numpy(), r["dx64"], rtol=1e-9, atol=1e-12 * np.abs(r["dx64"]).max())
    assert st["pos_encoder.pe"].grad is None


def test_fixture_names():
    assert tenc_cases() == ["tenc_grad_l1_b3_t17", "tenc_grad_l2_b2_t100"]


def test_port_in_eval_mode_reproduces_inference_vectors():
    w = np.load(os.path.join(GOLDEN, "tenc_weights.npz"))
    state = {k[4:]: torch.from_numpy(w[k]) for k in w.files}
    c = np.load(os.path.join(GOLDEN, "tenc_cases.npz"))
    for n in ("b2_t100", "b3_t37", "b1_t1", "b5_t16", "b2_t17"):
        y = port_forward(torch.from_numpy(c["x_" + n]), state, {}, 0.0, torch.float32)
        assert float((y - torch.from_numpy(c["y_" + n])).abs().max()) <= 5e-6, n


def _cpu_masks(B, T, nlayers, p, seed, ones=False):
    g = torch.Generator().manual_seed(seed)

    def draw(*shape):
        return torch.ones(shape, dtype=torch.uint8) if ones else (torch.rand(shape, generator=g) >= p).to(torch.uint8)

    masks = {"pos": draw(B, T, 24)}
    for l in range(nlayers):
        masks[(l, "attn")] = draw(B, 4, T, T)
        for n in NAMES[1:]:
            masks[(l, n)] = draw(B, T, 128)
    return masks


def test_port_dropout_semantics():
    B, T, L = 2, 9, 2
    state = {k: v.double() for k, v in seeded_state(L, 5).items()}
    x = torch.randn((B, T, 12, 2), generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    t0 = {}
    y0 = port_forward(x, state, {}, 0.0, torch.float64, t0)
    for p in (0.1, 0.5):
        masks, tr = _cpu_masks(B, T, L, p, 7), {}
        y = port_forward(x, state, masks, p, torch.float64, tr)
        assert float((y - y0).abs().max()) > 1e-3                      # the masks act
        # the dropped input is the kept part of the p = 0 input times 1 / (1 - p): linear in 1 / (1 - p)
        torch.testing.assert_close(tr["x0"] * (1 - p), t0["x0"] * masks["pos"], rtol=1e-12, atol=1e-14)
        # layer 0's probabilities see the same scale on top of a softmax whose rows summed to 1
        pd = tr[(0, "probs")]
        assert not pd[masks[(0, "attn")] == 0].any()
        s = pd * (1 - p)                                               # the kept softmax values
        assert float(s.max()) <= 1.0 and float(s.sum(-1).max()) <= 1.0 + 1e-12
    # all-ones masks: y is the p = 0 result in the limit p -> 0, and the scale acts at p = 0.5
    ones = _cpu_masks(B, T, L, 0.0, 0, ones=True)
    torch.testing.assert_close(port_forward(x, state, ones, 1e-13, torch.float64), y0, rtol=1e-9, atol=1e-10)
    tr = {}
    port_forward(x, state, ones, 0.5, torch.float64, tr)
    torch.testing.assert_close(tr["x0"], 2.0 * t0["x0"], rtol=1e-15, atol=0)
    # p = 1 drops everything, as torch does: the output is a function of the biases and LayerNorms alone
    z = _cpu_masks(B, T, L, 1.0, 1)
    assert not any(m.any() for m in z.values())
    y1 = port_forward(x, state, z, 1.0, torch.float64)
    assert torch.isfinite(y1).all() and torch.equal(y1, port_forward(x * 3, state, z, 1.0, torch.float64))


def test_new_kernels_have_no_scratch_or_spills():
    kernels, _ = kernel_remarks()
    new = {n: r for n, r in kernels.items() if "b2h_tt_" in n}
    # posenc, linear, linear_dx, linear_dw, reduce, layernorm, layernorm_bwd, sdpa, sdpa_bwd
    assert len(new) == 9, sorted(new)
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
