"""Shared pieces of the tests of TextPoseTransformer's other geometries (tests/test_tpt_geom_*.py; a helper module,
not a conftest.py): tpt_ref's and tpt_train_ref's helpers with (n_joints, nout) as parameters, and the fixtures
tests/golden/tpt/geom_*.npz, geom_train_*.npz and tests/golden/metric_j*.npz written by
tests/golden/make_golden_tpt_geom.py from the reference classes.

The reference's CLIs build the class in four geometries (n_joints, nout): (12, 42), (8, 42), (29, 8) and (21, 24);
the library takes every pairing of n_joints in {8, 12, 21, 29} with nout in {8, 24, 42}."""
import copy
import functools
import os
import warnings

import numpy as np
import torch
import torch.nn.functional as F

import tpt_ref
from conftest import GOLDEN
from tpt_train_ref import _attention, _drop, layer_counts

N_JOINTS = (8, 12, 21, 29)
NOUTS = (8, 24, 42)
DEFAULT = (12, 42)
COMBOS = [(j, o) for j in N_JOINTS for o in NOUTS]
NEW_COMBOS = [c for c in COMBOS if c != DEFAULT]                               # the 11 the library used to refuse
REFERENCE_PAIRS = [(8, 42), (29, 8), (21, 24)]                                 # run.py:100-101, :92-93, :96-97
SHAPES = [(3, 9, 17, 1, 1), (2, 17, 33, 4, 4)]                                 # (B, S, T, n_enc, n_dec)
CASES = [(j, o) + s for j, o in REFERENCE_PAIRS for s in SHAPES]
LONG_CASE = (29, 8, 2, 40, 130, 2, 2)
NO_FIXTURE = [c for c in COMBOS if c not in REFERENCE_PAIRS]                   # nine, the default pair among them
TRAIN_CASE = "geom_train_j29_o8_b3_s9_t17"


def case_name(n_joints, nout, B, S, T, n_enc, n_dec):
    return f"geom_j{n_joints}_o{nout}_b{B}_s{S}_t{T}_e{n_enc}_d{n_dec}"


def case_id(c):
    return "j%d_o%d_b%d_s%d_t%d_e%d_d%d" % tuple(c)


@functools.lru_cache(maxsize=None)
def load_case(*case):
    with np.load(os.path.join(tpt_ref.TPT, case_name(*case) + ".npz")) as d:
        rec = {k: d[k] for k in d.files}
    names = ("B", "S", "T", "n_tokens", "n_enc", "n_dec", "seed", "n_joints", "nout", "input_seed")
    rec.update({n: int(v) for n, v in zip(names, rec["meta"])})
    rec["keys"] = [str(k) for k in rec["keys"]]
    rec["shapes"] = [tuple(int(d) for d in str(s).split(",")) for s in rec["shapes"]]
    return rec


def build(n_tokens, n_joints, nout, n_enc, n_dec, **kw):
    import hand_pose_sl_amd as hps
    with warnings.catch_warnings():  # torch notes that seq-first layers skip its nested-tensor path
        warnings.simplefilter("ignore", UserWarning)
        return hps.TextPoseTransformer(n_tokens, n_joints, 2, 4, 128, nout, n_enc, n_dec, **kw)


def recipe_model(seed, n_tokens, n_joints, nout, n_enc, n_dec, **kw):
    """tpt_ref.recipe_model (the generators' weight recipe) with the geometry as a parameter."""
    torch.manual_seed(seed)
    model = build(n_tokens, n_joints, nout, n_enc, n_dec, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, p in model.named_parameters():
            p += 0.05 * torch.randn(p.shape, generator=g)
    return model.eval()


def case_model(*case):
    r = load_case(*case)
    return recipe_model(r["seed"], r["n_tokens"], r["n_joints"], r["nout"], r["n_enc"], r["n_dec"])


class Checker(tpt_ref.Checker):
    """tpt_ref.Checker for any head width."""

    def __call__(self, tokens, pose):
        tokens, pose = torch.as_tensor(tokens).cpu(), torch.as_tensor(pose).cpu().to(self.dtype)
        B, T = pose.shape[0], pose.shape[1]
        with torch.no_grad():
            src = self.emb(tokens).permute(1, 0, 2)
            tgt = self.p2h(pose.reshape(B, T, -1)).permute(1, 0, 2)
            return self.h2p(self.tr(src, tgt)).permute(1, 0, 2).reshape(B, T, -1, 2)


def inputs(B, S, T, n_tokens, n_joints, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_tokens, (B, S), generator=g), torch.rand((B, T, n_joints, 2), generator=g) - 0.5


def tol(y64):
    """The project's fp32 transformer bar (tpt_ref.BAR = 2e-5), relative to outputs above 1."""
    return tpt_ref.BAR * max(1.0, float(torch.as_tensor(y64).abs().max()))


# ---- training --------------------------------------------------------------------------------------------------
def port_forward(tokens, pose, state, masks, p, dtype):
    """tpt_train_ref.port_forward for any geometry: the widths follow from the two projections' shapes."""
    B, T = pose.shape[0], pose.shape[1]
    n_enc, n_dec = layer_counts(state)

    def ln(h, pre):
        return F.layer_norm(h, (128,), state[pre + ".weight"], state[pre + ".bias"], 1e-5)

    def ff(h, pre, keep):
        f = _drop(F.relu(F.linear(h, state[pre + "linear1.weight"], state[pre + "linear1.bias"])), keep, p)
        return F.linear(f, state[pre + "linear2.weight"], state[pre + "linear2.bias"])

    def attn(xq, xkv, pre, keep):
        return _attention(xq, xkv, state[pre + "in_proj_weight"], state[pre + "in_proj_bias"], state[pre + "out_proj.weight"],
                          state[pre + "out_proj.bias"], keep, p, None, None)

    mem = F.embedding(torch.as_tensor(tokens).long(), state["token_embedding.weight"])
    for l in range(n_enc):
        pre, mk = f"transformer.encoder.layers.{l}.", lambda n: masks.get(("enc", l, n))  # noqa: E731
        mem = ln(mem + _drop(attn(mem, mem, pre + "self_attn.", mk("attn")), mk("drop1"), p), pre + "norm1")
        mem = ln(mem + _drop(ff(mem, pre, mk("ff")), mk("drop2"), p), pre + "norm2")
    mem = ln(mem, "transformer.encoder.norm")
    h = F.linear(pose.reshape(B, T, -1).to(dtype), state["pose2hidden_projection.weight"], state["pose2hidden_projection.bias"])
    for l in range(n_dec):
        pre, mk = f"transformer.decoder.layers.{l}.", lambda n: masks.get(("dec", l, n))  # noqa: E731
        h = ln(h + _drop(attn(h, h, pre + "self_attn.", mk("self_attn")), mk("drop1"), p), pre + "norm1")
        h = ln(h + _drop(attn(h, mem, pre + "multihead_attn.", mk("cross_attn")), mk("drop2"), p), pre + "norm2")
        h = ln(h + _drop(ff(h, pre, mk("ff")), mk("drop3"), p), pre + "norm3")
    h = ln(h, "transformer.decoder.norm")
    y = F.linear(h, state["hidden2pose_projection.weight"], state["hidden2pose_projection.bias"])
    return y.reshape(B, T, -1, 2)


def port_grads(tokens, pose, state, masks, p, dy, dtype):
    """y, the parameter gradients (order of tpt_train_ref.param_keys) and dx of sum(y * dy) through the port."""
    from tpt_train_ref import leaf_state, param_keys
    st = leaf_state(state, dtype)
    xx = torch.as_tensor(pose).detach().to(dtype).clone().requires_grad_(True)
    y = port_forward(tokens, xx, st, masks, p, dtype)
    (y * torch.as_tensor(dy).to(dtype)).sum().backward()
    return y.detach(), [st[k].grad for k in param_keys(*layer_counts(st))], xx.grad


@functools.lru_cache(maxsize=None)
def recipe_state(seed, n_tokens, n_joints, nout, n_enc, n_dec):
    """The state_dict of recipe_model; shared, so leave it unchanged."""
    return {k: v.detach().clone() for k, v in recipe_model(seed, n_tokens, n_joints, nout, n_enc, n_dec).state_dict().items()}


def train_model(state, p, dev=None):
    """The mirror with dropout p holding `state` (whose projections carry the geometry), in training mode [on `dev`]."""
    n_enc, n_dec = layer_counts(state)
    m = build(state["token_embedding.weight"].shape[0], state["pose2hidden_projection.weight"].shape[1] // 2,
              state["hidden2pose_projection.weight"].shape[0], n_enc, n_dec, dropout=p)
    m.load_state_dict(copy.deepcopy(state))
    return (m.to(dev) if dev is not None else m).train()


@functools.lru_cache(maxsize=None)
def load_train():
    with np.load(os.path.join(tpt_ref.TPT, TRAIN_CASE + ".npz")) as d:
        rec = {k: d[k] for k in d.files}
    names = ("B", "S", "T", "n_tokens", "n_enc", "n_dec", "seed", "n_joints", "nout")
    rec.update({n: int(v) for n, v in zip(names, rec["meta"])})
    rec["state"] = recipe_state(rec["seed"], rec["n_tokens"], rec["n_joints"], rec["nout"], rec["n_enc"], rec["n_dec"])
    return rec


@functools.lru_cache(maxsize=None)
def load_metric(J):
    with np.load(os.path.join(GOLDEN, f"metric_j{J}_b5_t60.npz")) as d:
        return {k: d[k] for k in d.files}
