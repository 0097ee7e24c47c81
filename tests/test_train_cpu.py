"""Training path without a GPU: the new C ABI entry points are declared, typed and exported; the
training fixtures (tests/golden/train/) reproduce through float64 autograd of the oracle's torch port,
which pins the checker the GPU tests use; the new kernels compile without scratch or spills."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from train_ref import KEYS, load_train, port_grads, reference_loss, train_cases
from kernel_remarks import kernel_remarks

NEW = ["b2h_train_forward", "b2h_backward_workspace_bytes", "b2h_backward", "b2h_masked_l1_backward",
       "b2h_weighted_l1_backward"]


def test_training_symbols_declared_typed_exported():
    from hand_pose_sl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "b2h.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/b2h.h"
        assert n in _lib.SYMBOLS, f"{n} not typed in _lib.SYMBOLS"
        assert hasattr(lib, n), f"{n} not exported by libb2h.so"
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    for cite in ("HandPoseModels.py:40-64", "steps/utils.py:413-452", "traintest.py:111-121"):
        assert cite in header


def test_training_entry_points_reject_bad_arguments_without_gpu():
    import ctypes
    from hand_pose_sl_amd import _lib
    lib = _lib.load()
    ptrs = (ctypes.c_void_p * 8)()
    assert lib.b2h_train_forward(None, ptrs, None, None, 1, 1, None) == _lib.ERR_INVALID
    assert lib.b2h_backward(None, ptrs, None, None, None, ptrs, 1, 1, None, 0, None) == _lib.ERR_INVALID
    assert lib.b2h_backward_workspace_bytes(None, 1, 1) == 0
    assert lib.b2h_masked_l1_backward(None, None, None, 1, 1, None, None, None) == _lib.ERR_INVALID
    assert lib.b2h_weighted_l1_backward(None, None, None, None, 1, 1, None, None, None) == _lib.ERR_INVALID


def test_training_path_documented_and_inference_guard_gone():
    import hand_pose_sl_amd as hps
    assert "training" in hps.ConvModel.__doc__ and "exact fp32" in hps.ConvModel.__doc__
    src = open(os.path.join(ROOT, "hand_pose_sl_amd", "conv_model.py")).read()
    assert "is inference-only: call model.eval()" not in src


@pytest.mark.parametrize("name", train_cases("grad_"))
def test_grad_fixture_reproduces_through_torch_port(name):
    r = load_train(name)
    x = torch.from_numpy(r["x"]).double().requires_grad_(True)
    st = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in r["state"].items()}
    from train_ref import _port64
    from oracle.torch_port import torch_forward
    y = _port64(x, st) if r["pos_emb"] else torch_forward(x, st, False)
    loss = reference_loss(y, torch.from_numpy(r["target"]).double(), r["lengths"],
                          torch.from_numpy(r["scores"]).double(), str(r["loss_kind"]))
    loss.backward()
    np.testing.assert_equal(np.isnan(loss.item()), np.isnan(float(r["loss64"])))
    if not np.isnan(float(r["loss64"])):
        assert abs(loss.item() - float(r["loss64"])) <= 1e-12 * max(1.0, abs(float(r["loss64"])))
    for k in KEYS:
        g64 = r["g64_" + k.replace(".", "_")]
        np.testing.assert_allclose(st[k].grad.numpy(), g64, rtol=1e-9, atol=1e-12 * np.abs(g64).max(), err_msg=k)
        assert 0 < float(r["err32_" + k.replace(".", "_")]) < 1e-3 * max(np.abs(g64).max(), 1e-30) + 1e-12
    np.testing.assert_allclose(x.grad.numpy(), r["dx64"], rtol=1e-9, atol=1e-12 * np.abs(r["dx64"]).max())


def test_trajectory_fixture_reproduces_through_torch_port():
    r = load_train("traj_c30_b4_t64")
    from oracle.torch_port import torch_forward
    st = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in r["state"].items()}
    opt = torch.optim.Adam([st[k] for k in KEYS], lr=float(r["lr"]))
    x, t = torch.from_numpy(r["x"]).double(), torch.from_numpy(r["target"]).double()
    losses = []
    for _ in range(int(r["steps"])):
        loss = reference_loss(torch_forward(x, st, False), t, r["lengths"], None, "L1")
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    np.testing.assert_allclose(losses, r["losses64"], rtol=1e-10)
    for k in KEYS:
        np.testing.assert_allclose(st[k].detach().numpy(), r["final64_" + k.replace(".", "_")], rtol=0, atol=1e-10)


def test_new_kernels_have_no_scratch_or_spills():
    kernels, _ = kernel_remarks()
    new = {n: r for n, r in kernels.items() if "b2h_train_" in n or "b2h_l1_backward" in n}
    assert len(new) == 6, sorted(new)    # b2h_train_conv<0|1|2>, b2h_train_reduce, b2h_l1_backward_kernel<2>
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
