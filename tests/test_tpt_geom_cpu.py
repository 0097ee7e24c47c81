"""TextPoseTransformer in every geometry the reference's CLIs build, without a GPU: b2h_tpt_create accepts
n_joints*joints_dim in {16, 24, 42, 58} x nout in {8, 24, 42} and goes on refusing everything else; the new entry
points are declared, typed and exported and check their arguments; the mirror's state_dict in the three new reference
pairs equals the reference's (fixtures of tests/golden/make_golden_tpt_geom.py); the Python-side errors; the checker
of the GPU tests reproduces the fixtures; `infer --predict` argument handling."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tpt_geom_ref as G
from conftest import ROOT

NEW = ["b2h_tpt_info", "b2h_tpt_build_item", "b2h_masked_l1_joints", "b2h_weighted_l1_joints",
       "b2h_masked_l1_joints_backward", "b2h_weighted_l1_joints_backward"]


def test_symbols_declared_typed_exported():
    from hand_pose_sl_amd import _lib
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/b2h.h"
        assert n in _lib.SYMBOLS, f"{n} not typed in _lib.SYMBOLS"
        assert hasattr(lib, n), f"{n} not exported by libb2h.so"
    for cite in ("run.py:92-93", "run.py:96-97", "run.py:100-101", "infer_utterance.py:79-80"):
        assert cite in header


@pytest.mark.parametrize("combo", G.NEW_COMBOS, ids=lambda c: "j%d_o%d" % c)
def test_create_accepts_the_reference_geometries(combo):
    """No longer B2H_ERR_UNSUPPORTED: the call gets as far as looking for a device.  (With a GPU it succeeds.)"""
    from hand_pose_sl_amd import _lib
    lib = _lib.load()
    n_joints, nout = combo
    h = ctypes.c_void_p()
    rc = lib.b2h_tpt_create(60, 2 * n_joints, 4, 128, nout, 1, 1, ctypes.byref(h))
    assert rc != _lib.ERR_UNSUPPORTED, _lib.last_error()
    if rc == _lib.OK:
        ninp, no, has = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(7)
        assert lib.b2h_tpt_info(h, None, ctypes.byref(ninp), ctypes.byref(no), None, None, ctypes.byref(has)) == _lib.OK
        assert (ninp.value, no.value, has.value) == (2 * n_joints, nout, 0)
        assert lib.b2h_tpt_destroy(h) == _lib.OK
    else:
        assert rc in (_lib.ERR_NO_DEVICE, _lib.ERR_HIP), _lib.last_error()
        assert h.value is None


@pytest.mark.parametrize("geom", [(60, 26, 4, 128, 42, 1, 1), (60, 24, 4, 128, 40, 1, 1), (60, 40, 4, 128, 42, 1, 1),
                                  (60, 60, 4, 128, 8, 1, 1), (60, 58, 4, 128, 16, 1, 1), (60, 42, 4, 128, 21, 1, 1),
                                  (60, 8, 4, 128, 42, 1, 1), (60, 58, 8, 128, 8, 1, 1), (60, 42, 4, 64, 24, 1, 1)])
def test_create_still_refuses_everything_else(geom):
    from hand_pose_sl_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p(1)
    assert lib.b2h_tpt_create(*geom, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert h.value is None and "TextPoseTransformer" in _lib.last_error()


def test_new_entry_points_check_their_arguments_without_gpu():
    from hand_pose_sl_amd import _lib
    lib = _lib.load()
    buf = ctypes.c_void_p(4096)  # never dereferenced
    assert lib.b2h_tpt_info(None, None, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.b2h_tpt_build_item(buf, buf, buf, 1, 1, 0, 0, 1.0, None) == _lib.ERR_INVALID      # right_hand: no item to build
    assert lib.b2h_tpt_build_item(buf, buf, buf, 1, 1, 3, 0, 1.0, None) == _lib.ERR_INVALID
    assert lib.b2h_tpt_build_item(buf, buf, buf, 1, 1, 1, 4, 1.0, None) == _lib.ERR_INVALID      # a POST flag
    assert lib.b2h_tpt_build_item(buf, buf, buf, 1, 1, 2, 2, 0.0, None) == _lib.ERR_INVALID      # factor
    assert lib.b2h_tpt_build_item(buf, buf, buf, -1, 1, 1, 0, 1.0, None) == _lib.ERR_SHAPE
    assert lib.b2h_tpt_build_item(None, None, None, 0, 5, 1, 0, 1.0, None) == _lib.OK            # empty: a no-op
    for J in (0, -1, 1025):
        assert lib.b2h_masked_l1_joints(buf, buf, None, 1, 1, J, buf, buf, None) == _lib.ERR_SHAPE
        assert lib.b2h_weighted_l1_joints_backward(buf, buf, buf, None, 1, 1, J, buf, buf, None) == _lib.ERR_SHAPE
    assert lib.b2h_weighted_l1_joints(buf, buf, None, None, 1, 1, 4, buf, buf, None) == _lib.ERR_INVALID


@pytest.mark.parametrize("case", G.CASES + [G.LONG_CASE], ids=G.case_id)
def test_state_dict_equals_the_reference(case):
    """Keys, order, shapes and float64 checksums of a mirror built by the generator's recipe in the reference's
    other three constructor calls: a checkpoint of the reference's own trainer has these shapes and loads."""
    r = G.load_case(*case)
    sd = G.case_model(*case).state_dict()
    assert list(sd) == r["keys"]
    assert [tuple(v.shape) for v in sd.values()] == r["shapes"]
    assert np.array_equal(np.array([v.double().sum().item() for v in sd.values()]), r["sums"])
    assert np.array_equal(np.array([v.double().abs().sum().item() for v in sd.values()]), r["abs_sums"])
    assert tuple(sd["pose2hidden_projection.weight"].shape) == (128, 2 * r["n_joints"])
    assert tuple(sd["hidden2pose_projection.weight"].shape) == (r["nout"], 128)


def test_the_mirror_takes_a_state_dict_of_eight_joints():
    """run.py's default `--predict right_hand` trains (8, 42): its pose2hidden_projection.weight is (128, 16).  Only the
    torch containers are checked here; that b2h_tpt_load_weights packs such weights is the (8, 42) parity test on the GPU
    (tests/test_tpt_geom_gpu.py::test_parity_with_the_reference)."""
    src = G.recipe_model(3, 60, 8, 42, 1, 1)
    dst = G.build(60, 8, 42, 1, 1)
    dst.load_state_dict(src.state_dict())
    assert tuple(dst.state_dict()["pose2hidden_projection.weight"].shape) == (128, 16)
    with pytest.raises(RuntimeError):
        G.build(60, 12, 42, 1, 1).load_state_dict(src.state_dict())   # the default geometry: a shape mismatch, as in torch


@pytest.mark.parametrize("case", G.CASES + [G.LONG_CASE], ids=G.case_id)
def test_checker_reproduces_reference_fixture(case):
    r = G.load_case(*case)
    model = G.case_model(*case)
    y32 = G.Checker(model, torch.float32)(r["tokens"], r["pose"]).numpy()
    y64 = G.Checker(model, torch.float64)(r["tokens"], r["pose"]).numpy()
    assert y32.shape == r["y32"].shape == (r["B"], r["T"], r["nout"] // 2, 2)
    assert r["pose"].shape == (r["B"], r["T"], r["n_joints"], 2)
    assert np.abs(y32 - r["y32"]).max() <= 1e-6
    assert np.abs(y64 - r["y64"]).max() <= 1e-12
    assert np.abs(r["y32"] - r["y64"]).max() <= 2e-6         # make_golden_tpt.MAX_REF_ERR
    assert 0.5 < np.abs(r["y64"]).max() < 4.0                # outputs of order 1: absolute bounds mean something


def test_python_side_errors():
    tok = torch.zeros((2, 5), dtype=torch.int64)
    for n_joints, nout in G.NEW_COMBOS:
        model = G.build(50, n_joints, nout, 1, 1).eval()
        assert (model.ninp, model.nout) == (2 * n_joints, nout)
        with pytest.raises(RuntimeError, match=rf"\(B, T, {n_joints}, 2\)"):     # the model's own joint count
            model(tok, torch.zeros((2, 7, n_joints + 1, 2)))
        with pytest.raises(RuntimeError, match="MI355X"):
            model(tok, torch.zeros((2, 7, n_joints, 2)))                          # a right shape: no CPU path
    default = G.build(50, 12, 42, 1, 1).eval()
    with pytest.raises(RuntimeError, match="12, 2"):
        default(tok, torch.zeros((2, 7, 8, 2)))
    body, hand = torch.zeros((2, 7, 12, 2)), torch.zeros((2, 7, 21, 2))
    for n_joints in (21, 29):                                                     # composite: right_hand is required
        model = G.build(50, n_joints, 8, 1, 1).eval()
        with pytest.raises(ValueError, match="right_hand"):
            model.forward_fused(tok, body)
        with pytest.raises(RuntimeError, match=r"\(B, T, 12, 2\)"):
            model.forward_fused(tok, torch.zeros((2, 7, n_joints, 2)), right_hand=hand)
        with pytest.raises(RuntimeError, match="right_hand of shape"):
            model.forward_fused(tok, body, right_hand=torch.zeros((2, 6, 21, 2)))
    for n_joints in (8, 12):                                                      # body only: right_hand is refused
        model = G.build(50, n_joints, 42, 1, 1).eval()
        with pytest.raises(ValueError, match="right_hand"):
            model.forward_fused(tok, torch.zeros((2, 7, n_joints, 2)), right_hand=hand)
        with pytest.raises(ValueError, match="composite"):
            model.build_item(body, hand)


def test_infer_predict_arguments(tmp_path):
    from hand_pose_sl_amd import infer
    assert infer.PREDICT_GEOMETRY == {"right_hand": (12, 42), "right_index": (29, 8), "right_3fingers": (21, 24)}
    base = ["--data", str(tmp_path), "--model-checkpoint", "none.pth", "--output-folder", str(tmp_path / "out")]
    for model in ("Conv", "TransformerEnc"):
        with pytest.raises(SystemExit, match="needs --model TextPoseTransformer"):
            infer.main(base + ["--model", model, "--predict", "right_index"])
    with pytest.raises(SystemExit):                                               # argparse: not one of the choices
        infer.main(base + ["--model", "TextPoseTransformer", "--predict", "left_hand", "--tokens", "t.json"])
    with pytest.raises(SystemExit, match="token ids"):                            # the text model still needs its ids
        infer.main(base + ["--model", "TextPoseTransformer", "--predict", "right_3fingers"])
    with pytest.raises(SystemExit, match="no \\*.json frames"):                   # accepted: fails later, for the data
        infer.main(base + ["--model", "TextPoseTransformer", "--predict", "right_3fingers", "--tokens", "t.json"])


def test_port_reproduces_the_training_fixture():
    """tpt_geom_ref.port_forward, the float64 reference of the GPU training tests, against the reference class's own
    loss and gradients in the (29, 8) geometry (mask_output + maskedPoseL1, traintest.py:105-121)."""
    from tpt_train_ref import leaf_state, masked_l1, param_keys
    r = G.load_train()
    assert (r["n_joints"], r["nout"]) == (29, 8)
    assert np.array_equal(np.array([v.double().sum().item() for k, v in r["state"].items() if not k.endswith(".pe")]), r["sums"])
    st = leaf_state(r["state"], torch.float64)
    x = torch.from_numpy(r["x"]).double().requires_grad_(True)
    lengths = [int(n) for n in r["lengths"]]
    y = G.port_forward(r["tokens"], x, st, {}, 0.0, torch.float64)
    assert y.shape == (3, 17, 4, 2)
    loss = masked_l1(y, torch.from_numpy(r["target"]).double(), lengths)
    loss.backward()
    assert abs(loss.item() - float(r["loss64"])) <= 1e-12
    assert np.abs(x.grad.numpy() - r["dx64"]).max() <= 1e-12 * max(1.0, np.abs(r["dx64"]).max())
    stored = [k for k in param_keys(1, 1) if "g64_" + k in r]
    assert len(stored) == 5
    for k in stored:
        assert np.abs(st[k].grad.numpy() - r["g64_" + k]).max() <= 1e-12 * max(1.0, np.abs(r["g64_" + k]).max()), k


@pytest.mark.parametrize("predict,joints", [("right_index", slice(5, 9)), ("right_3fingers", slice(1, 13)), ("right_hand", slice(0, 21))])
def test_merged_file_writer_rewrites_only_the_predicted_joints(tmp_path, predict, joints):
    """write_merged_predictions(predict=), the merged-file end of `infer --predict`: the 4 or 12 predicted joints land
    on joints 5..8 or 1..12 of every frame's 63-float right hand and nothing else moves."""
    import json

    from conftest import load_golden
    from hand_pose_sl_amd import openpose
    frames = json.loads(str(load_golden("openpose_long_n30_m20")["frames_json"]))[:3]
    entries = [{"id": f"utt_{i:012d}_keypoints", "data": fr} for i, fr in enumerate(frames)]
    J = joints.stop - joints.start
    pred = np.arange(5 * J * 2, dtype=np.float32).reshape(5, J, 2) + 0.5        # more rows than frames, like the CLI's
    out = openpose.write_merged_predictions(entries, pred, str(tmp_path / "out" / "utt.json"), predict=predict)
    back = openpose.load_merged_utterance(out)
    assert [e["id"] for e in back] == [e["id"] for e in entries]
    for i, e in enumerate(back):
        got = np.array(e["data"]["people"][0]["hand_right_keypoints_2d"])
        before = np.array(frames[i]["people"][0]["hand_right_keypoints_2d"]).reshape(21, 3)
        assert got.shape == (63,)
        got = got.reshape(21, 3)
        keep = [j for j in range(21) if not joints.start <= j < joints.stop]
        assert np.array_equal(got[keep], before[keep])
        assert np.array_equal(got[joints, :2], pred[i]) and (got[joints, 2] == 1.0).all()
        assert e["data"]["people"][0]["pose_keypoints_2d"] == frames[i]["people"][0]["pose_keypoints_2d"]
