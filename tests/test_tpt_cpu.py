"""TextPoseTransformer without a GPU: the C ABI entry points are declared, typed, exported and refuse bad
arguments; the mirror's constructor, state_dict and seeded init equal the reference's (through the fixtures of
tests/golden/tpt/); the Python-side errors; the checker of the GPU tests (tpt_ref.Checker) reproduces the
reference's outputs; the new kernels compile without scratch or spills."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from tpt_ref import CASES, Checker, build, case_model, load_case, recipe_model
from kernel_remarks import kernel_remarks

NEW = ["b2h_tpt_create", "b2h_tpt_destroy", "b2h_tpt_load_weights", "b2h_tpt_workspace_bytes", "b2h_tpt_forward"]


def test_symbols_declared_typed_exported():
    from hand_pose_sl_amd import _lib
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/b2h.h"
        assert n in _lib.SYMBOLS, f"{n} not typed in _lib.SYMBOLS"
        assert hasattr(lib, n), f"{n} not exported by libb2h.so"
    for cite in ("HandPoseModels.py:181-230", "traintest.py:105-107", "run.py:148-151"):
        assert cite in header
    assert lib.b2h_version() == 100


def test_entry_points_reject_null_arguments_without_gpu():
    from hand_pose_sl_amd import _lib
    lib = _lib.load()
    ptrs = (ctypes.c_void_p * 129)()
    buf = ctypes.c_void_p(4096)  # never dereferenced: the model is NULL
    assert lib.b2h_tpt_forward(None, buf, buf, buf, 1, 1, 1, buf, 1 << 20, None) == _lib.ERR_INVALID
    assert lib.b2h_tpt_forward(None, None, None, None, 1, 1, 1, None, 0, None) == _lib.ERR_INVALID
    assert lib.b2h_tpt_load_weights(None, ptrs, 129, 0) == _lib.ERR_INVALID
    assert lib.b2h_tpt_load_weights(None, None, 129, 0) == _lib.ERR_INVALID
    assert lib.b2h_tpt_workspace_bytes(None, 1, 1, 1) == 0
    assert lib.b2h_tpt_create(1000, 24, 4, 128, 42, 4, 4, None) == _lib.ERR_INVALID
    assert lib.b2h_tpt_destroy(None) == _lib.OK


@pytest.mark.parametrize("geom", [(1000, 24, 4, 64, 42, 4, 4), (1000, 24, 8, 128, 42, 4, 4), (1000, 24, 4, 128, 42, 0, 4),
                                  (1000, 24, 4, 128, 42, 4, 0), (1000, 24, 4, 128, 42, 17, 4), (1000, 24, 4, 128, 42, 4, 17),
                                  (0, 24, 4, 128, 42, 4, 4), (1000, 26, 4, 128, 42, 4, 4), (1000, 24, 4, 128, 40, 4, 4)])
def test_create_refuses_other_geometries(geom):
    from hand_pose_sl_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p(1)
    assert lib.b2h_tpt_create(*geom, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert h.value is None                                   # nothing handed out
    assert "TextPoseTransformer" in _lib.last_error()


def test_constructor_signature():
    import hand_pose_sl_amd as hps
    p = inspect.signature(hps.TextPoseTransformer.__init__).parameters
    assert list(p) == ["self", "n_tokens", "n_joints", "joints_dim", "nhead", "nhid", "nout", "n_enc_layers", "n_dec_layers",
                       "dropout", "precision"]
    assert p["dropout"].default == 0.5 and p["precision"].default == "fp32"
    assert p["precision"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "TextPoseTransformer" in hps.__all__


@pytest.mark.parametrize("name", ["default_b3_s40_t100", "small_weights_b2_s9_t20"])
def test_state_dict_and_seeded_init_equal_the_reference(name):
    """Keys, order, shapes, and -- through float64 checksums of every tensor -- the values of a model built by the
    generator's recipe: the construction order and the init are the reference's."""
    r = load_case(name)
    sd = recipe_model(r["seed"], r["n_tokens"], r["n_enc"], r["n_dec"]).state_dict()
    assert list(sd) == r["keys"]
    assert [tuple(v.shape) for v in sd.values()] == r["shapes"]
    assert np.array_equal(np.array([v.double().sum().item() for v in sd.values()]), r["sums"])
    assert np.array_equal(np.array([v.double().abs().sum().item() for v in sd.values()]), r["abs_sums"])
    if name.startswith("default"):
        assert len(sd) == 131 and sum(1 for k in sd if k.endswith(".pe")) == 2
        assert [tuple(sd[k].shape) for k in ("token_pos_encoder.pe", "pose_pos_encoder.pe")] == [(40, 1, 128), (100, 1, 128)]


def test_load_state_dict_round_trip_from_stored_arrays():
    r = load_case("small_weights_b2_s9_t20")
    model = case_model("small_weights_b2_s9_t20")
    for i, (k, v) in enumerate(model.state_dict().items()):
        assert k == r["keys"][i] and np.array_equal(v.numpy(), r[f"w{i:03d}"]), k
    # the stored arrays are the recipe's model: the two ways to the weights agree
    again = recipe_model(r["seed"], r["n_tokens"], r["n_enc"], r["n_dec"]).state_dict()
    assert all(torch.equal(v, again[k]) for k, v in model.state_dict().items())
    with pytest.raises(RuntimeError):
        build(51, 1, 1).load_state_dict(model.state_dict())  # another vocabulary: a shape mismatch, as in torch


def test_python_side_errors():
    model = build(50, 1, 1).eval()
    tok, pose = torch.zeros((2, 5), dtype=torch.int64), torch.zeros((2, 7, 12, 2))
    with pytest.raises(RuntimeError, match="MI355X"):
        model(tok, pose)                                     # parameters on the CPU: no CPU path
    with pytest.raises(ValueError, match="precision"):
        build(50, 1, 1, precision="f16x3")
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
        build(50, 1, 1).train()(tok, pose)                   # dropout 0.5 would apply here
    with pytest.raises(RuntimeError, match="12, 2"):
        model(tok, torch.zeros((2, 7, 24)))
    with pytest.raises(RuntimeError, match="12, 2"):
        model(tok, torch.zeros((2, 7, 13, 2)))
    with pytest.raises(RuntimeError, match=r"\(B, S\)"):
        model(torch.zeros((2, 5, 1), dtype=torch.int64), pose)
    with pytest.raises(RuntimeError, match="batch size"):
        model(torch.zeros((3, 5), dtype=torch.int64), pose)
    for bad in (50, -1):
        t = tok.clone()
        t[1, 3] = bad
        with pytest.raises(IndexError):
            model(t, pose)                                   # host ids are checked on the host, like nn.Embedding
    # train mode with p = 0 is not refused for its mode (it then fails for the missing GPU, like eval mode)
    with pytest.raises(RuntimeError, match="MI355X"):
        build(50, 1, 1, dropout=0.0).train()(tok, pose)


def test_package_never_imports_oracle():
    code = ("import sys; import hand_pose_sl_amd as h; m = h.TextPoseTransformer(50, 12, 2, 4, 128, 42, 1, 1); "
            "assert not [n for n in sys.modules if n == 'oracle' or n.startswith('oracle.')], sorted(sys.modules)")
    r = subprocess.run([sys.executable, "-W", "ignore", "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    pkg = os.path.join(ROOT, "hand_pose_sl_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            assert not re.search(r"^\s*(import|from)\s+oracle\b", open(os.path.join(pkg, f)).read(), flags=re.M), f


@pytest.mark.parametrize("name", CASES)
def test_checker_reproduces_reference_fixture(name):
    """The checker of the GPU tests against the reference's stored outputs, and the condition that keeps the GPU
    bound meaningful: the reference's own fp32 result is within 2e-6 of its float64 copy on every fixture."""
    r = load_case(name)
    model = case_model(name)
    y32 = Checker(model, torch.float32)(r["tokens"], r["pose"]).numpy()
    y64 = Checker(model, torch.float64)(r["tokens"], r["pose"]).numpy()
    print(f"{name}: checker32 vs y32 {np.abs(y32 - r['y32']).max():.2e}  checker64 vs y64 {np.abs(y64 - r['y64']).max():.2e}  "
          f"reference y32 vs y64 {np.abs(r['y32'] - r['y64']).max():.2e}")
    assert y32.shape == r["y32"].shape == (r["B"], r["T"], 21, 2)
    assert np.abs(y32 - r["y32"]).max() <= 1e-6
    assert np.abs(y64 - r["y64"]).max() <= 1e-12
    assert np.abs(r["y32"] - r["y64"]).max() <= 2e-6
    assert 1.0 < np.abs(r["y64"]).max() < 4.0                # outputs of order 2: absolute bounds mean something


def test_new_kernels_have_no_scratch_or_spills():
    kernels, _ = kernel_remarks()
    new = {n: r for n, r in kernels.items() if "b2h_tpt_" in n or "b2h_attn_f32" in n}
    # embed, layernorm, and the fp32 attention over described rows (self and cross) by key tiles 1..8 (not 8 x 8: the
    # query tiles are the block size), each with and without as many query tiles; "b2h_attn_f32" is no substring of
    # "b2h_attn_long_f32"
    assert len(new) == 18, sorted(new)
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
