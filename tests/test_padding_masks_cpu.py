"""Key-padding masks without a GPU: the masked port of tests/padding_ref.py against torch's own
nn.Transformer with src / tgt / memory key-padding masks in float64, the properties the GPU tests pin bit for bit
(checked here on the oracle itself), the numpy reference of token_lengths, the declarations, and every refusal that
needs no GPU work."""
import os
import types

import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
import padding_ref as ref
import tpt_ref
from hand_pose_sl_amd import _lib
from kernel_remarks import ROOT, kernel_remarks

NEW = ("b2h_token_lengths", "b2h_tpt_forward_masked", "b2h_tpt_train_forward_masked", "b2h_tpt_backward_masked")


def _state64(name):
    return {k: v.double() for k, v in ref.case_state(name).items() if not k.endswith(".pe")}


# ---- the port against nn.Transformer with masks ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["whole", "deep"])
def test_port_equals_nn_transformer_with_masks(name):
    tok, x, dy, tl, fl = ref.case_data(name)
    st = _state64(name)
    valid = ref.valid_frames(fl, x.shape[1])
    with torch.no_grad():
        a = ref.oracle_forward(tok, x.double(), st, tl, fl)
        b = ref.port_forward_masked(tok, x.double(), st, {}, 0.0, torch.float64, tl, fl)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()        # padded query rows attend to the valid keys
    assert float((a - b)[valid].abs().max()) <= 1e-12
    # and its gradients
    state = ref.case_state(name)
    _, ga, dxa = ref.grads_of(lambda t, xx, s: ref.oracle_forward(t, xx, s, tl, fl), tok, x, state, dy, torch.float64)
    _, gb, dxb = ref.grads_of(lambda t, xx, s: ref.port_forward_masked(t, xx, s, {}, 0.0, torch.float64, tl, fl), tok, x,
                              state, dy, torch.float64)
    for u, v in zip(ga + [dxa], gb + [dxb]):
        assert float((u - v).abs().max()) <= 1e-12 * max(1.0, float(u.abs().max()))


def test_only_one_length_given():
    tok, x, _, tl, fl = ref.case_data("whole")
    st = _state64("whole")
    valid = ref.valid_frames(fl, x.shape[1])
    with torch.no_grad():
        for a, b in ((tl, None), (None, fl)):
            u = ref.oracle_forward(tok, x.double(), st, a, b)
            v = ref.port_forward_masked(tok, x.double(), st, {}, 0.0, torch.float64, a, b)
            assert float((u - v)[valid].abs().max()) <= 1e-12
        full = ref.port_forward_masked(tok, x.double(), st, {}, 0.0, torch.float64, [9, 9, 9], [17, 17, 17])
        none = ref.port_forward_masked(tok, x.double(), st, {}, 0.0, torch.float64)
        assert torch.equal(full, none)


def test_the_oracle_has_the_properties_the_gpu_tests_pin():
    """Padding content does not reach a valid frame, and the gradient of a padded frame row is exactly 0."""
    tok, x, dy, tl, fl = ref.case_data("whole")
    tok2, x2 = ref.repadded("whole")
    assert not torch.equal(tok, tok2) and not torch.equal(x, x2)
    st = _state64("whole")
    valid = ref.valid_frames(fl, x.shape[1])
    with torch.no_grad():
        a = ref.oracle_forward(tok, x.double(), st, tl, fl)
        b = ref.oracle_forward(tok2, x2.double(), st, tl, fl)
    assert torch.equal(a[valid], b[valid])
    _, _, dx, _, _ = ref.case_reference("whole")
    assert not dx[~valid].any() and dx[valid].any()


def test_clamp_of_the_reference():
    assert ref.clamp_lengths([0, -3, 5, 20], 17) == [1, 1, 5, 17]
    assert ref.pad_mask([0, 20], 4).tolist() == [[False, True, True, True], [False] * 4]


# ---- token_lengths -----------------------------------------------------------------------------------------------
TOKEN_ROWS = np.array([[5, 6, 7, 8, 9, 1, 2, 3, 4],        # no padding
                       [0, 0, 0, 0, 0, 0, 0, 0, 0],        # all padding -> 1
                       [3, 0, 4, 0, 0, 0, 0, 0, 0],        # an interior 0 followed by another id
                       [-1, -1, 0, 0, 0, 0, 0, 0, 0],      # ids of -1
                       [7, 7, 7, 2, 7, 7, 7, 7, 7]], dtype=np.int64)


def test_token_lengths_numpy_reference():
    assert ref.token_lengths_ref(TOKEN_ROWS).tolist() == [9, 1, 3, 2, 9]
    assert ref.token_lengths_ref(TOKEN_ROWS, pad_id=7).tolist() == [9, 9, 9, 9, 4]
    assert ref.token_lengths_ref(TOKEN_ROWS, pad_id=-1).tolist() == [9, 9, 9, 9, 9]
    assert ref.token_lengths_ref(np.zeros((2, 1), np.int64)).tolist() == [1, 1]


@pytest.mark.parametrize("tokens,message", [
    (torch.zeros((2, 3), dtype=torch.int32), "int64"),
    (torch.zeros(3, dtype=torch.int64), r"\(B, S\)"),
    (torch.zeros((2, 0), dtype=torch.int64), "S >= 1"),
    ([[1, 2]], "int64"),
    (torch.zeros((2, 3), dtype=torch.int64), "MI355X"),
])
def test_token_lengths_refusals(tokens, message):
    with pytest.raises(RuntimeError, match=message):
        hps.token_lengths(tokens)


# ---- declarations -----------------------------------------------------------------------------------------------
def test_entry_points_declared_typed_and_exported():
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert f"int {name}(" in header and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "token_lengths" in hps.__all__
    # the masked lists are their parents' plus the two length pointers
    for parent, masked in (("b2h_tpt_train_forward", "b2h_tpt_train_forward_masked"), ("b2h_tpt_backward", "b2h_tpt_backward_masked"),
                           ("b2h_tpt_forward_fused", "b2h_tpt_forward_masked")):
        assert len(_lib.SYMBOLS[masked][1]) == len(_lib.SYMBOLS[parent][1]) + 2


@pytest.mark.parametrize("kw,status,message", [
    (dict(B=-1), _lib.ERR_SHAPE, "B >= 0"),
    (dict(S=0), _lib.ERR_SHAPE, "S >= 1"),
    (dict(tokens=None), _lib.ERR_INVALID, "NULL"),
    (dict(lengths=None), _lib.ERR_INVALID, "NULL"),
    (dict(tokens=0x1004), _lib.ERR_INVALID, "8-byte aligned"),
    (dict(lengths=0x2004), _lib.ERR_INVALID, "8-byte aligned"),
    (dict(lengths=0x1008), _lib.ERR_INVALID, "overlaps"),
])
def test_token_lengths_host_refusals(kw, status, message):
    """Refused before any launch: the pointers are never dereferenced."""
    a = dict(tokens=0x1000, B=2, S=3, pad=0, lengths=0x2000)
    a.update(kw)
    lib = _lib.load()
    assert lib.b2h_token_lengths(a["tokens"], a["B"], a["S"], a["pad"], a["lengths"], None) == status
    assert message in _lib.last_error()


def test_token_lengths_of_an_empty_batch_is_a_no_op():
    assert _lib.load().b2h_token_lengths(None, 0, 3, 0, None, None) == _lib.OK


def test_new_kernels_have_no_scratch_or_spills():
    kernels, _ = kernel_remarks()
    new = {n: r for n, r in kernels.items() if "b2h_token_lengths_k" in n or "b2h_attn_klen_f32" in n or "b2h_attn_long_klen_f32" in n}
    assert len(new) == 1 + 16 + 8, sorted(new)
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)


# ---- Python-side refusals ---------------------------------------------------------------------------------------
def _cpu_model():
    return tpt_ref.build(ref.N_TOKENS, 1, 1).eval()


@pytest.mark.parametrize("kw,message", [
    (dict(text_lengths=[9, 4]), r"text_lengths of shape \(3,\), got \(2,\)"),
    (dict(frame_lengths=torch.ones((3, 1), dtype=torch.int64)), r"frame_lengths of shape \(3,\), got \(3, 1\)"),
    (dict(text_lengths=[1, 2, 3], frame_lengths=5), r"frame_lengths of shape \(3,\), got \(\)"),
])
@pytest.mark.parametrize("method", ["__call__", "forward_long", "forward_fused"])
def test_wrong_length_shapes_are_refused_before_the_device_is_needed(method, kw, message):
    m = _cpu_model()
    tok, x, _, _, _ = ref.case_data("whole")
    with pytest.raises(RuntimeError, match=message):
        getattr(m, method)(tok, x, **kw)


@pytest.mark.parametrize("method", ["__call__", "forward_long", "forward_fused"])
def test_f16x3_refuses_lengths_and_names_the_remedy(method):
    m = _cpu_model().set_precision("f16x3")
    tok, x, _, tl, fl = ref.case_data("whole")
    for kw in (dict(text_lengths=tl), dict(frame_lengths=fl)):
        with pytest.raises(RuntimeError, match=r"F16X3 takes no key lengths.*b2h_tpt_set_kernel\(fp32\)"):
            getattr(m, method)(tok, x, **kw)


def test_the_c_abi_refusal_of_f16x3_names_the_remedy_too():
    src = open(os.path.join(ROOT, "hand_pose_sl_amd", "csrc", "b2h_api.hip")).read()
    i = src.index("B2H_TENC_F16X3 takes no key lengths")
    assert "B2H_ERR_UNSUPPORTED" in src[i - 200:i] and "b2h_tpt_set_kernel(fp32)" in src[i:i + 300]


def test_mask_padding_needs_a_text_model():
    conv = hps.ConvModel(30, "ReLU", False)
    enc = hps.TransformerEnc(ninp=24, nhead=4, nhid=128, nout=42, nlayers=1)
    opt = types.SimpleNamespace()
    for m in (conv, enc):
        for call in (lambda: hps.train_epoch(m, [], loss="L1", optimizer=opt, mask_padding=True),
                     lambda: hps.validate(m, [], loss="L1", mask_padding=True),
                     lambda: hps.GraphTrainer(m, None, None, loss="L1", mask_padding=True),
                     lambda: hps.predict_dataset(m, None, mask_padding=True)):
            with pytest.raises(ValueError, match="mask_padding=True hands key-padding masks to a TextPoseTransformer"):
                call()
    # without the flag each makes the refusals it always made
    with pytest.raises(ValueError, match="DeviceLoader"):
        hps.GraphTrainer(conv, None, None, loss="L1")
    with pytest.raises(ZeroDivisionError):
        hps.validate(conv, [], loss="L1")


def test_cli_refuses_mask_padding_without_a_text_model_or_with_f16x3(tmp_path):
    from hand_pose_sl_amd import infer
    base = ["--data", str(tmp_path), "--model-checkpoint", "x", "--output-folder", str(tmp_path / "out"), "--mask-padding"]
    with pytest.raises(SystemExit, match="--mask-padding needs --model TextPoseTransformer"):
        infer.main(base)
    with pytest.raises(SystemExit, match="--mask-padding runs with --precision fp32"):
        infer.main(base + ["--model", "TextPoseTransformer", "--precision", "f16x3", "--tokens", "t.json"])
