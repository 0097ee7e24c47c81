"""Helpers of the TransformerEnc training tests (tests/test_tenc_train_*.py): the training-mode forward restated
with plain torch ops on the CPU (`port_forward`, taking the dropout keep-masks as inputs, so float64 autograd
through it is an exact reference for every gradient), the fixtures under tests/golden/train/tenc_grad_*.npz and
float64 / float32 gradients of the port.  A helper module, not a conftest.py: the tests import it by name.

The accuracy bar is train_ref.bar: per tensor max|g - g64| <= 4 * max|g32_ref - g64| + 1e-6 * max|g64|."""
import glob
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from train_ref import TRAIN, assert_within_bar, bar  # noqa: F401  (re-exported: the project's one accuracy rule)

NAMES = ("attn", "drop1", "ff", "drop2")


def param_keys(nlayers):
    """state_dict names of the parameters in the order of TransformerEnc._tensors() (without the buffer pe)."""
    keys = ["pose2hidden_projection.weight", "pose2hidden_projection.bias"]
    for l in range(nlayers):
        pre = f"transformer_encoder.layers.{l}."
        keys += [pre + n for n in ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
                                   "self_attn.out_proj.bias", "linear1.weight", "linear1.bias", "linear2.weight",
                                   "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")]
    return keys + ["hidden2pose_projection.weight", "hidden2pose_projection.bias"]


def _drop(h, keep, p):
    """torch's dropout with the mask given: h * keep / (1 - p); identity at p = 0, all dropped at p = 1."""
    if p == 0:
        return h
    if p == 1:
        return h * 0
    return h * (keep.to(h.dtype) / (1 - p))


def port_forward(x, state, masks, p, dtype, trace=None):
    """TransformerEnc.forward in .train() mode (HandPoseModels.py:154-178; torch's post-norm
    nn.TransformerEncoderLayer with ReLU, no attention mask), batch first, in `dtype` on the CPU.
    state: name -> tensor (already of `dtype`; may require grad); masks: {} at p = 0, else the dict of
    TransformerEnc._draw_dropout_masks (CPU).  `trace`: a dict that receives intermediates."""
    B, T = x.shape[0], x.shape[1]
    nlayers = sum(1 for k in state if k.endswith("self_attn.in_proj_weight"))
    h = x.reshape(B, T, 24).to(dtype) + state["pos_encoder.pe"][:T, 0].to(dtype).unsqueeze(0)
    h = _drop(h, masks.get("pos"), p)
    if trace is not None:
        trace["x0"] = h
    h = F.linear(h, state["pose2hidden_projection.weight"], state["pose2hidden_projection.bias"])
    for l in range(nlayers):
        w = lambda n: state[f"transformer_encoder.layers.{l}.{n}"]  # noqa: E731
        qkv = F.linear(h, w("self_attn.in_proj_weight"), w("self_attn.in_proj_bias"))
        q, k, v = (t.reshape(B, T, 4, 32).transpose(1, 2) for t in qkv.split(128, dim=-1))
        s = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(32.0), dim=-1)
        pd = _drop(s, masks.get((l, "attn")), p)
        if trace is not None:
            trace[(l, "probs")] = pd
        o = (pd @ v).transpose(1, 2).reshape(B, T, 128)
        a = F.linear(o, w("self_attn.out_proj.weight"), w("self_attn.out_proj.bias"))
        h = F.layer_norm(h + _drop(a, masks.get((l, "drop1")), p), (128,), w("norm1.weight"), w("norm1.bias"), 1e-5)
        f = _drop(F.relu(F.linear(h, w("linear1.weight"), w("linear1.bias"))), masks.get((l, "ff")), p)
        f = F.linear(f, w("linear2.weight"), w("linear2.bias"))
        h = F.layer_norm(h + _drop(f, masks.get((l, "drop2")), p), (128,), w("norm2.weight"), w("norm2.bias"), 1e-5)
    y = F.linear(h, state["hidden2pose_projection.weight"], state["hidden2pose_projection.bias"])
    return y.reshape(B, T, 21, 2)


def leaf_state(state, dtype):
    return {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(k != "pos_encoder.pe") for k, v in state.items()}


def port_grads(x, state, masks, p, dy, dtype):
    """y, the parameter gradients (order of param_keys) and dx of sum(y * dy) through port_forward in `dtype`."""
    st = leaf_state(state, dtype)
    xx = torch.as_tensor(x).detach().to(dtype).clone().requires_grad_(True)
    y = port_forward(xx, st, masks, p, dtype)
    (y * torch.as_tensor(dy).to(dtype)).sum().backward()
    nlayers = sum(1 for k in st if k.endswith("self_attn.in_proj_weight"))
    return y.detach(), [st[k].grad for k in param_keys(nlayers)], xx.grad


def seeded_state(nlayers, seed, max_len=100):
    """The state_dict of a default-initialised TransformerEnc under torch.manual_seed(seed): bit-identical to the
    reference class's (test_transformer_enc.py::test_mirror_state_dict_and_seeded_init_equal_reference)."""
    import hand_pose_sl_amd as hps
    torch.manual_seed(seed)
    m = hps.TransformerEnc(24, 4, 128, 42, nlayers, dropout=0.0)
    if max_len != 100:
        m.pos_encoder = hps.PositionalEncoding(24, 0.0, max_len=max_len)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def tenc_cases():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(TRAIN, "tenc_grad_*.npz"))
                  if ".part" not in os.path.basename(p))


def load_tenc(name):
    """One fixture: `name`.npz plus its continuation files `name`.part*.npz (a committed file stays below 1 MiB)."""
    rec = {}
    for path in [os.path.join(TRAIN, name + ".npz")] + sorted(glob.glob(os.path.join(TRAIN, name + ".part*.npz"))):
        d = np.load(path)
        rec.update({k: d[k] for k in d.files})
    B, T, nlayers, seed = [int(v) for v in rec["meta"]]
    rec.update(B=B, T=T, nlayers=nlayers, seed=seed, state=seeded_state(nlayers, seed))
    return rec


def masked_l1(pred, target, lengths):
    """maskedPoseL1 after mask_output (steps/utils.py:309-312,413-428), restated with torch ops."""
    from train_ref import reference_loss
    return reference_loss(pred, target, lengths, None, "L1")
