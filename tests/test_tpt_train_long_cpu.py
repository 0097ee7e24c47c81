"""TextPoseTransformer training beyond 128 frames without a GPU: the fixture of the reference class at the
trainer's default length (tests/golden/tpt/long_train_e2_d2_b2_s40_t200.npz, written by
tests/golden/tpt/make_golden_tpt_train_long.py) pins the GPU tests' checker (tpt_train_ref.port_forward) at
T = 200; the blocked attention kernels (kernel_train_attn_long.h) compile for gfx950 without scratch or spills;
the C ABI answers without a device at T = 200."""
import ctypes
import os

import numpy as np
import torch

import tpt_ref
from conftest import ROOT
from tpt_train_ref import leaf_state, load_train, masked_l1, param_keys, port_forward
from kernel_remarks import kernel_remarks

LONG_CASE = "long_train_e2_d2_b2_s40_t200"
LONG_KERNELS = ["b2h_lt_sdpaE", "b2h_lt_sdpa_bwd_kvE", "b2h_lt_sdpa_bwd_qE"]   # as the mangled names spell them


def test_fixture_shape_recipe_and_size():
    files = sorted(f for f in os.listdir(tpt_ref.TPT) if f.startswith("long_train_") and f.endswith(".npz"))
    assert sorted({f.split(".")[0] for f in files}) == [LONG_CASE]
    assert all(os.path.getsize(os.path.join(tpt_ref.TPT, f)) <= 1000 * 1024 for f in files)
    r = load_train(LONG_CASE)
    assert (r["B"], r["S"], r["T"], r["n_enc"], r["n_dec"]) == (2, 40, 200, 2, 2)
    assert r["lengths"].tolist() == [200, 130] and r["x"].shape == (2, 200, 12, 2)
    assert float(np.abs(r["x"]).max()) < 5.0 / 1280 * 1.5             # inputs at the scale 1 / 1280
    keys = param_keys(r["n_enc"], r["n_dec"])
    sums = [r["state"][k].double().sum().item() for k in keys]
    np.testing.assert_allclose(sums, r["sums"], rtol=1e-12, atol=1e-12)
    for k in keys:                                                    # small=True: the keys of the (2, 40, 100) fixture
        assert "err32_" + k in r
        assert ("g64_" + k in r) == (r["state"][k].dim() == 1 or not k.startswith("transformer."))


def test_port_reproduces_reference_fixture_at_200_frames():
    """Float64 autograd through port_forward at p = 0 == the reference class in .train() with dropout 0, at the
    tolerances of test_tpt_train_cpu.py::test_port_reproduces_reference_fixture."""
    r = load_train(LONG_CASE)
    st = leaf_state(r["state"], torch.float64)
    x = torch.from_numpy(r["x"]).double().requires_grad_(True)
    y = port_forward(torch.from_numpy(r["tokens"]), x, st, {}, 0.0, torch.float64)
    loss = masked_l1(y, torch.from_numpy(r["target"]).double(), r["lengths"])
    loss.backward()
    assert abs(loss.item() - float(r["loss64"])) <= 1e-12 * abs(float(r["loss64"]))
    checked = 0
    for k in param_keys(r["n_enc"], r["n_dec"]):
        if "g64_" + k not in r:
            continue
        g64 = r["g64_" + k]
        np.testing.assert_allclose(st[k].grad.numpy(), g64, rtol=1e-9, atol=1e-12 * np.abs(g64).max(), err_msg=k)
        checked += 1
    assert checked >= 30
    np.testing.assert_allclose(x.grad.numpy(), r["dx64"], rtol=1e-9, atol=1e-12 * np.abs(r["dx64"]).max())


def test_long_kernels_have_no_scratch_or_spills():
    kernels, _ = kernel_remarks()
    new = {n: r for n, r in kernels.items() if "b2h_lt_" in n}
    assert len(new) == 3 and all(any(k in n for n in new) for k in LONG_KERNELS), sorted(new)
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)   # dynamic LDS only; the caps are raised at creation
        print(name, res)


def test_entry_points_answer_without_gpu_at_200_frames():
    from hand_pose_sl_amd import _lib
    lib = _lib.load()
    ptrs = (ctypes.c_void_p * 39)()
    assert all(lib.b2h_tpt_train_bytes(None, 128, 40, 200, which) == 0 for which in (0, 1))
    assert lib.b2h_tpt_train_forward(None, ptrs, None, None, None, 0.0, None, None, 0, 2, 40, 200, None) == _lib.ERR_INVALID
    assert lib.b2h_tpt_backward(None, ptrs, None, None, 0.0, None, None, 0, None, ptrs, None, 0, 2, 40, 200, None) == _lib.ERR_INVALID
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    assert "kernel_train_attn_long.h" in header and "B*T * 32*n_dec_layers" in header and "which = 1, B*T * 32" in header
