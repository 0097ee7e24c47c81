"""TextPoseTransformer training without a GPU: the new C ABI entry points are declared, typed and exported; the
checker of the GPU tests (tpt_train_ref.port_forward) is pinned to the reference class through the fixtures
(tests/golden/tpt/train_*.npz, p = 0) and to the mirror's own nn.Transformer modules (tpt_ref.Checker), and its
dropout follows torch's definition; the new kernels compile without scratch or spills."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tpt_ref
from conftest import ROOT
from kernel_remarks import kernel_remarks
from tpt_train_ref import (TRAIN_CASES, cpu_masks, leaf_state, load_train, mask_shapes, masked_l1, param_keys,
                           port_forward, recipe_state, tokens_with_padding)

NEW = ["b2h_tpt_train_bytes", "b2h_tpt_train_forward", "b2h_tpt_backward"]


def test_symbols_declared_typed_exported():
    from hand_pose_sl_amd import _lib
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/b2h.h"
        assert n in _lib.SYMBOLS, f"{n} not typed in _lib.SYMBOLS"
        assert hasattr(lib, n), f"{n} not exported by libb2h.so"
    for cite in ("HandPoseModels.py:201-222", "traintest.py:105-121"):
        assert cite in header


def test_entry_points_reject_null_arguments_without_gpu():
    from hand_pose_sl_amd import _lib
    lib = _lib.load()
    ptrs = (ctypes.c_void_p * 39)()
    assert lib.b2h_tpt_train_forward(None, ptrs, None, None, None, 0.0, None, None, 0, 1, 1, 1, None) == _lib.ERR_INVALID
    assert lib.b2h_tpt_train_forward(None, None, None, None, None, 0.0, None, None, 0, 1, 1, 1, None) == _lib.ERR_INVALID
    assert lib.b2h_tpt_backward(None, ptrs, None, None, 0.0, None, None, 0, None, ptrs, None, 0, 1, 1, 1, None) == _lib.ERR_INVALID
    assert all(lib.b2h_tpt_train_bytes(None, 1, 1, 1, which) == 0 for which in (0, 1))


def test_fixture_names_and_recipe():
    """The two fixtures exist, no file exceeds 1000 KiB, and the mirror built by the recipe holds the weights the
    reference class held when the fixture was written (per-tensor float64 sums)."""
    files = sorted(f for f in os.listdir(tpt_ref.TPT) if f.startswith("train_") and f.endswith(".npz"))
    assert sorted({f.split(".")[0] for f in files}) == TRAIN_CASES
    assert all(os.path.getsize(os.path.join(tpt_ref.TPT, f)) <= 1000 * 1024 for f in files)
    for name in TRAIN_CASES:
        r = load_train(name)
        keys = param_keys(r["n_enc"], r["n_dec"])
        sums = [r["state"][k].double().sum().item() for k in keys]
        np.testing.assert_allclose(sums, r["sums"], rtol=1e-12, atol=1e-12)
        full = name == TRAIN_CASES[0]
        for k in keys:
            assert "err32_" + k in r
            assert ("g64_" + k in r) == (full or r["state"][k].dim() == 1 or not k.startswith("transformer."))


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_port_reproduces_reference_fixture(name):
    """Float64 autograd through port_forward at p = 0 == the reference class in .train() with dropout 0."""
    r = load_train(name)
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
        # rtol 1e-9 per element plus a floor of 1e-12 of the tensor's largest gradient: the key third of every
        # in_proj_bias has a gradient that is zero in mathematics, so both float64 runs hold rounding noise there
        np.testing.assert_allclose(st[k].grad.numpy(), g64, rtol=1e-9, atol=1e-12 * np.abs(g64).max(), err_msg=k)
        checked += 1
    assert checked >= 30
    np.testing.assert_allclose(x.grad.numpy(), r["dx64"], rtol=1e-9, atol=1e-12 * np.abs(r["dx64"]).max())


def test_port_equals_the_mirrors_own_torch_modules():
    """p = 0, float64: the functional restatement == nn.Transformer between the mirror's embedding and projections."""
    for (n_enc, n_dec), (B, S, T) in (((1, 1), (2, 9, 17)), ((2, 3), (2, 17, 5))):
        model = tpt_ref.recipe_model(20 + n_dec, 50, n_enc, n_dec)
        state = {k: v.double() for k, v in model.state_dict().items()}
        tok, pose = tpt_ref.inputs(B, S, T, 50, 21)
        want = tpt_ref.Checker(model, torch.float64)(tok, pose)
        got = port_forward(tok, pose.double(), state, {}, 0.0, torch.float64)
        torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-12)


def test_port_dropout_semantics():
    B, S, T, ne, nd = 2, 5, 9, 1, 2
    state = {k: v.double() for k, v in recipe_state(5, 50, ne, nd).items()}
    g = torch.Generator().manual_seed(6)
    tok = tokens_with_padding(B, S, 50, g)
    x = torch.randn((B, T, 12, 2), generator=g, dtype=torch.float64)
    t0 = {}
    y0 = port_forward(tok, x, state, {}, 0.0, torch.float64, t0)
    for p in (0.1, 0.5):
        masks, tr = cpu_masks(B, S, T, ne, nd, p, 7), {}
        assert [(k, tuple(v.shape)) for k, v in masks.items()] == mask_shapes(B, S, T, ne, nd)
        y = port_forward(tok, x, state, masks, p, torch.float64, tr)
        assert float((y - y0).abs().max()) > 1e-3                      # the masks act
        # the first attention of each stack sees the p = 0 input: its probabilities are the kept p = 0 ones / (1 - p)
        for key, mk in ((("enc", 0, "probs"), ("enc", 0, "attn")), (("dec", 0, "self_probs"), ("dec", 0, "self_attn"))):
            torch.testing.assert_close(tr[key] * (1 - p), t0[key] * masks[mk], rtol=1e-12, atol=1e-15)
        # dropped probabilities are zero; the kept ones are softmax values times 1 / (1 - p)
        for l in range(nd):
            pd = tr[("dec", l, "cross_probs")]
            assert pd.shape == (B, 4, T, S) and not pd[masks[("dec", l, "cross_attn")] == 0].any()
            s = pd * (1 - p)
            assert float(s.max()) <= 1.0 and float(s.sum(-1).max()) <= 1.0 + 1e-12
    # all-ones masks: y is the p = 0 result in the limit p -> 0, and the scale acts at p = 0.5
    ones = cpu_masks(B, S, T, ne, nd, 0.0, 0, ones=True)
    torch.testing.assert_close(port_forward(tok, x, state, ones, 1e-13, torch.float64), y0, rtol=1e-9, atol=1e-10)
    tr = {}
    port_forward(tok, x, state, ones, 0.5, torch.float64, tr)
    torch.testing.assert_close(tr[("enc", 0, "probs")], 2.0 * t0[("enc", 0, "probs")], rtol=1e-15, atol=0)
    # p = 1 drops every sublayer's contribution, as torch does: y is finite and independent of the tokens (the
    # memory reaches y through the dropped cross-attention alone) and of everything but the residual stream of
    # pose2hidden_projection, which no dropout touches in this model
    z = cpu_masks(B, S, T, ne, nd, 1.0, 1)
    assert not any(m.any() for m in z.values())
    tr = {}
    y1 = port_forward(tok, x, state, z, 1.0, torch.float64, tr)
    assert torch.isfinite(y1).all() and not tr[("dec", 0, "cross_probs")].any()
    assert torch.equal(y1, port_forward((tok + 7) % 50, x, state, z, 1.0, torch.float64))
    h = tr["tgt"]
    for l in range(nd):
        for i in (1, 2, 3):
            pre = f"transformer.decoder.layers.{l}.norm{i}"
            h = torch.nn.functional.layer_norm(h, (128,), state[pre + ".weight"], state[pre + ".bias"], 1e-5)
    h = torch.nn.functional.layer_norm(h, (128,), state["transformer.decoder.norm.weight"], state["transformer.decoder.norm.bias"], 1e-5)
    want = torch.nn.functional.linear(h, state["hidden2pose_projection.weight"], state["hidden2pose_projection.bias"])
    torch.testing.assert_close(y1, want.reshape(B, T, 21, 2), rtol=1e-12, atol=1e-13)


def test_new_kernels_have_no_scratch_or_spills():
    kernels, _ = kernel_remarks()
    new = {n: r for n, r in kernels.items() if "b2h_tptt_" in n}
    assert len(new) == 1, sorted(new)                                  # embed_bwd; the attentions are b2h_tt_sdpa*
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
