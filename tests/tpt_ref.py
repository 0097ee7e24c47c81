"""Shared pieces of the TextPoseTransformer tests (a helper module, not a conftest.py): the fixtures under
tests/golden/tpt/ (written by tests/golden/make_golden_tpt.py from the reference class), the weight recipe they
share with that generator, and the checker -- the mirror's own torch modules called directly on the CPU, in
float32 or float64, composed as the reference's forward composes them (HandPoseModels.py:201-222)."""
import copy
import functools
import os
import warnings

import numpy as np
import torch

from conftest import GOLDEN

TPT = os.path.join(GOLDEN, "tpt")
CASES = ["default_b3_s40_t100", "default_b2_s17_t33", "default_b2_s1_t1", "small_weights_b2_s9_t20"]
BAR = 2e-5   # max|y - y64|: the project's fp32 transformer bar (DESIGN.md sections 2, 9, 12)


@functools.lru_cache(maxsize=None)
def load_case(name):
    with np.load(os.path.join(TPT, name + ".npz")) as d:
        rec = {k: d[k] for k in d.files}
    part2 = os.path.join(TPT, name + ".part2.npz")
    if os.path.exists(part2):
        with np.load(part2) as d:
            rec.update({k: d[k] for k in d.files})
    B, S, T, n_tokens, n_enc, n_dec, seed = [int(v) for v in rec["meta"]]
    rec.update(B=B, S=S, T=T, n_tokens=n_tokens, n_enc=n_enc, n_dec=n_dec, seed=seed)
    rec["keys"] = [str(k) for k in rec["keys"]]
    rec["shapes"] = [tuple(int(d) for d in str(s).split(",")) for s in rec["shapes"]]
    return rec


def build(n_tokens, n_enc, n_dec, **kw):
    import hand_pose_sl_amd as hps
    with warnings.catch_warnings():  # torch notes that seq-first layers skip its nested-tensor path
        warnings.simplefilter("ignore", UserWarning)
        return hps.TextPoseTransformer(n_tokens, 12, 2, 4, 128, 42, n_enc, n_dec, **kw)


def recipe_model(seed, n_tokens, n_enc, n_dec):
    """The generator's recipe (make_golden_tpt.py) on the mirror: seeded default init, then seeded noise on every
    parameter so that attention biases and LayerNorm gains and biases are non-default; eval mode."""
    torch.manual_seed(seed)
    model = build(n_tokens, n_enc, n_dec)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, p in model.named_parameters():
            p += 0.05 * torch.randn(p.shape, generator=g)
    return model.eval()


def case_model(name):
    """The mirror holding the weights of fixture `name`: by recipe, or from the stored arrays."""
    r = load_case(name)
    if "w000" not in r:
        return recipe_model(r["seed"], r["n_tokens"], r["n_enc"], r["n_dec"])
    model = build(r["n_tokens"], r["n_enc"], r["n_dec"])
    model.load_state_dict({k: torch.from_numpy(r[f"w{i:03d}"]) for i, k in enumerate(r["keys"])})
    return model.eval()


class Checker:
    """TextPoseTransformer.forward on the CPU through deep copies of the model's torch modules in `dtype`."""

    def __init__(self, model, dtype=torch.float64):
        self.dtype = dtype
        M = model._modules
        self.tr, self.emb, self.h2p, self.p2h = (
            copy.deepcopy(M[n]).to(device="cpu", dtype=dtype).eval()
            for n in ("transformer", "token_embedding", "hidden2pose_projection", "pose2hidden_projection"))

    def __call__(self, tokens, pose):
        tokens, pose = torch.as_tensor(tokens).cpu(), torch.as_tensor(pose).cpu().to(self.dtype)
        B, T = pose.shape[0], pose.shape[1]
        with torch.no_grad():
            src = self.emb(tokens).permute(1, 0, 2)
            tgt = self.p2h(pose.reshape(B, T, -1)).permute(1, 0, 2)
            return self.h2p(self.tr(src, tgt)).permute(1, 0, 2).reshape(B, T, 21, 2)


def inputs(B, S, T, n_tokens, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_tokens, (B, S), generator=g), torch.rand((B, T, 12, 2), generator=g) - 0.5
