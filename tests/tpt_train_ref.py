"""Helpers of the TextPoseTransformer training tests (tests/test_tpt_train_*.py): the training-mode forward
restated with plain torch ops on the CPU (`port_forward`, taking the dropout keep-masks as inputs, so float64
autograd through it is an exact reference for every gradient), the fixtures tests/golden/tpt/train_*.npz
(written by tests/golden/tpt/make_golden_tpt_train.py from the reference class) and float64 / float32 gradients
of the port.  A helper module, not a conftest.py: the tests import it by name.

The accuracy bar is train_ref.bar: per tensor max|g - g64| <= 4 * max|g32_ref - g64| + 1e-6 * max|g64|."""
import functools
import glob
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import tpt_ref
from train_ref import assert_within_bar, bar, reference_loss  # noqa: F401  (re-exported: the project's one accuracy rule)

ENC_NAMES = ("attn", "drop1", "ff", "drop2")
DEC_NAMES = ("self_attn", "drop1", "cross_attn", "drop2", "ff", "drop3")
TRAIN_CASES = ["train_e1_d1_b3_s9_t17", "train_e2_d2_b2_s40_t100"]
_ATTN = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")
_FF = ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias")


def param_keys(n_enc, n_dec):
    """state_dict names of the parameters in the order of TextPoseTransformer._tensors() (b2h_tpt_load_weights)."""
    keys = []
    for l in range(n_enc):
        pre = f"transformer.encoder.layers.{l}."
        keys += [pre + "self_attn." + n for n in _ATTN] + [pre + n for n in _FF]
        keys += [pre + f"norm{i}.{n}" for i in (1, 2) for n in ("weight", "bias")]
    keys += ["transformer.encoder.norm.weight", "transformer.encoder.norm.bias"]
    for l in range(n_dec):
        pre = f"transformer.decoder.layers.{l}."
        keys += [pre + "self_attn." + n for n in _ATTN] + [pre + "multihead_attn." + n for n in _ATTN] + [pre + n for n in _FF]
        keys += [pre + f"norm{i}.{n}" for i in (1, 2, 3) for n in ("weight", "bias")]
    keys += ["transformer.decoder.norm.weight", "transformer.decoder.norm.bias"]
    return keys + ["token_embedding.weight", "hidden2pose_projection.weight", "hidden2pose_projection.bias",
                   "pose2hidden_projection.weight", "pose2hidden_projection.bias"]


def layer_counts(state):
    return (sum(1 for k in state if k.startswith("transformer.encoder.layers.") and k.endswith("self_attn.in_proj_weight")),
            sum(1 for k in state if k.startswith("transformer.decoder.layers.") and k.endswith("self_attn.in_proj_weight")))


def mask_shapes(B, S, T, n_enc, n_dec):
    """(key, shape) of the keep-masks in the documented order (include/b2h.h, _draw_dropout_masks)."""
    order = []
    for l in range(n_enc):
        order += [(("enc", l, n), (B, 4, S, S) if n == "attn" else (B, S, 128)) for n in ENC_NAMES]
    for l in range(n_dec):
        order += [(("dec", l, n), (B, 4, T, T) if n == "self_attn" else (B, 4, T, S) if n == "cross_attn" else (B, T, 128))
                  for n in DEC_NAMES]
    return order


def cpu_masks(B, S, T, n_enc, n_dec, p, seed, ones=False):
    """Keep-masks drawn on the CPU with a generator of their own; {} at p = 0 (unless `ones`)."""
    if p == 0 and not ones:
        return {}
    g = torch.Generator().manual_seed(seed)
    return {k: torch.ones(s, dtype=torch.uint8) if ones else (torch.rand(s, generator=g) >= p).to(torch.uint8)
            for k, s in mask_shapes(B, S, T, n_enc, n_dec)}


def _drop(h, keep, p):
    """torch's dropout with the mask given: h * keep / (1 - p); identity at p = 0, all dropped at p = 1."""
    if p == 0:
        return h
    if p == 1:
        return h * 0
    return h * (keep.to(h.dtype) / (1 - p))


def _attention(xq, xkv, w, b, wo, bo, keep, p, trace, key):
    """nn.MultiheadAttention(128, 4) without masks, batch first: queries of xq (B, Tq, 128), keys and values of
    xkv (B, Tk, 128); dropout on the softmax probabilities."""
    B, Tq, Tk = xq.shape[0], xq.shape[1], xkv.shape[1]
    q = F.linear(xq, w[:128], b[:128]).reshape(B, Tq, 4, 32).transpose(1, 2)
    k, v = (t.reshape(B, Tk, 4, 32).transpose(1, 2) for t in F.linear(xkv, w[128:], b[128:]).split(128, dim=-1))
    pd = _drop(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(32.0), dim=-1), keep, p)
    if trace is not None:
        trace[key] = pd
    return F.linear((pd @ v).transpose(1, 2).reshape(B, Tq, 128), wo, bo)


def port_forward(tokens, pose, state, masks, p, dtype, trace=None):
    """TextPoseTransformer.forward in .train() mode (HandPoseModels.py:201-222; torch's post-norm nn.Transformer
    with ReLU, no mask of any kind, no positional encoding), batch first, in `dtype` on the CPU.
    state: name -> tensor (already of `dtype`; may require grad); masks: {} at p = 0, else the dict of
    TextPoseTransformer._draw_dropout_masks (CPU).  `trace`: a dict that receives intermediates."""
    B, T = pose.shape[0], pose.shape[1]
    n_enc, n_dec = layer_counts(state)

    def ln(h, pre):
        return F.layer_norm(h, (128,), state[pre + ".weight"], state[pre + ".bias"], 1e-5)

    def ff(h, pre, keep):
        f = _drop(F.relu(F.linear(h, state[pre + "linear1.weight"], state[pre + "linear1.bias"])), keep, p)
        return F.linear(f, state[pre + "linear2.weight"], state[pre + "linear2.bias"])

    def attn(xq, xkv, pre, keep, key):
        return _attention(xq, xkv, state[pre + "in_proj_weight"], state[pre + "in_proj_bias"], state[pre + "out_proj.weight"],
                          state[pre + "out_proj.bias"], keep, p, trace, key)

    mem = F.embedding(torch.as_tensor(tokens).long(), state["token_embedding.weight"])
    for l in range(n_enc):
        pre, mk = f"transformer.encoder.layers.{l}.", lambda n: masks.get(("enc", l, n))  # noqa: E731
        mem = ln(mem + _drop(attn(mem, mem, pre + "self_attn.", mk("attn"), ("enc", l, "probs")), mk("drop1"), p), pre + "norm1")
        mem = ln(mem + _drop(ff(mem, pre, mk("ff")), mk("drop2"), p), pre + "norm2")
    mem = ln(mem, "transformer.encoder.norm")
    h = F.linear(pose.reshape(B, T, 24).to(dtype), state["pose2hidden_projection.weight"], state["pose2hidden_projection.bias"])
    if trace is not None:
        trace["memory"], trace["tgt"] = mem, h
    for l in range(n_dec):
        pre, mk = f"transformer.decoder.layers.{l}.", lambda n: masks.get(("dec", l, n))  # noqa: E731
        h = ln(h + _drop(attn(h, h, pre + "self_attn.", mk("self_attn"), ("dec", l, "self_probs")), mk("drop1"), p), pre + "norm1")
        h = ln(h + _drop(attn(h, mem, pre + "multihead_attn.", mk("cross_attn"), ("dec", l, "cross_probs")), mk("drop2"), p),
               pre + "norm2")
        h = ln(h + _drop(ff(h, pre, mk("ff")), mk("drop3"), p), pre + "norm3")
    h = ln(h, "transformer.decoder.norm")
    y = F.linear(h, state["hidden2pose_projection.weight"], state["hidden2pose_projection.bias"])
    return y.reshape(B, T, 21, 2)


def leaf_state(state, dtype):
    """The parameters of `state` (the two pe buffers are dropped) as leaves of `dtype` that require a gradient."""
    return {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()
            if not k.endswith(".pe")}


def port_grads(tokens, pose, state, masks, p, dy, dtype):
    """y, the parameter gradients (order of param_keys) and dx of sum(y * dy) through port_forward in `dtype`."""
    st = leaf_state(state, dtype)
    xx = torch.as_tensor(pose).detach().to(dtype).clone().requires_grad_(True)
    y = port_forward(tokens, xx, st, masks, p, dtype)
    (y * torch.as_tensor(dy).to(dtype)).sum().backward()
    return y.detach(), [st[k].grad for k in param_keys(*layer_counts(st))], xx.grad


@functools.lru_cache(maxsize=None)
def recipe_state(seed, n_tokens, n_enc, n_dec):
    """The state_dict of tpt_ref.recipe_model (the generators' weight recipe); shared, so leave it unchanged."""
    return {k: v.detach().clone() for k, v in tpt_ref.recipe_model(seed, n_tokens, n_enc, n_dec).state_dict().items()}


def train_model(state, p, dev=None):
    """The mirror with dropout p holding `state`, in training mode [on `dev`]."""
    n_enc, n_dec = layer_counts(state)
    m = tpt_ref.build(state["token_embedding.weight"].shape[0], n_enc, n_dec, dropout=p)
    m.load_state_dict(state)
    return (m.to(dev) if dev is not None else m).train()


def tokens_with_padding(B, S, n_tokens, gen):
    """Shaped like the dataset's rows (text_pose_dataset.py:467-470): a prefix of ids in [1, n_tokens - 1), then
    id 0 to the end of the row (at least one 0 where S > 1).  Id n_tokens - 1 is never used (n_tokens > 2)."""
    tok = torch.zeros((B, S), dtype=torch.int64)
    for b in range(B):
        n = int(torch.randint(1, S, (1,), generator=gen)) if S > 1 else 1
        if n_tokens > 1:
            tok[b, :n] = torch.randint(1, max(2, n_tokens - 1), (n,), generator=gen)
    return tok


@functools.lru_cache(maxsize=None)
def load_train(name):
    """One fixture: `name`.npz plus its continuation files `name`.part*.npz (a committed file stays below 1 MiB)."""
    rec = {}
    for path in [os.path.join(tpt_ref.TPT, name + ".npz")] + sorted(glob.glob(os.path.join(tpt_ref.TPT, name + ".part*.npz"))):
        with np.load(path) as d:
            rec.update({k: d[k] for k in d.files})
    B, S, T, n_tokens, n_enc, n_dec, seed = [int(v) for v in rec["meta"]]
    rec.update(B=B, S=S, T=T, n_tokens=n_tokens, n_enc=n_enc, n_dec=n_dec, seed=seed,
               state=recipe_state(seed, n_tokens, n_enc, n_dec))
    return rec


def masked_l1(pred, target, lengths):
    """maskedPoseL1 after mask_output (steps/utils.py:309-312,413-428), restated with torch ops."""
    return reference_loss(pred, target, lengths, None, "L1")
