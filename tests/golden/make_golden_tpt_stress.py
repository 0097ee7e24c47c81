#!/usr/bin/env python3
"""Generate tests/golden/tpt/stress_e2_d2.npz from the *reference* TextPoseTransformer under trained-like weights.

Runs only where the reference checkout is present, like make_golden_tpt.py, whose weight recipe and loader helpers it
uses.  The reference's class (body2hand/src/models/HandPoseModels.py:181-230) is built by that recipe, its state_dict
goes through the recipes of tests/tpt_stress_ref.py (`peaked`, `offset`, `lnvar`, `lnvar_mild`: the very functions the
tests apply to the mirror's state) and is loaded back; the class then runs on the CPU in float32 and, as a deep copy in
`.double()`, in float64.  Nothing of the reference (source or bytecode) is copied: the .npz holds data only.

Stored per inference case `<recipe>_<shape>_<kind>`: tokens, pose, y32, y64.  Stored for the one training case (the
class in .train() mode with dropout = 0.0, loss = sum(y * dy)): tokens, x, dy, y64, `err32_<name>` (the float32 run's
max-abs error) of every parameter and of dx, dx64, and the float64 gradient `g64_<name>` of the 1-D parameters, the
embedding and the two projections.  Weights are NOT stored: recipe_state(SEED) and the recipes regenerate them; `sums`
(float64 sum of every state_dict entry of every stressed state) pins that.

    python tests/golden/make_golden_tpt_stress.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                # tests/: tpt_stress_ref and its helpers
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import REF, _load, _stub_fairseq  # noqa: E402
from make_golden_tpt import recipe_model  # noqa: E402
import tpt_stress_ref as sr  # noqa: E402

OUT = os.path.join(HERE, "tpt", "stress_e2_d2.npz")
INFER = [("peaked", sr.SHAPES[0], "plain"), ("offset", sr.SHAPES[0], "plain"), ("lnvar", sr.SHAPES[0], "plain"),
         ("lnvar_mild", sr.SHAPES[0], "plain"), ("offset", sr.SHAPES[3], "ramp")]
TRAIN = ("offset", sr.SHAPES[0], "plain")


def stressed(cls, recipe, dropout=None):
    """The reference class holding RECIPES[recipe] of its own recipe-built state_dict."""
    kw = {} if dropout is None else {"dropout": dropout}
    torch.manual_seed(sr.SEED)
    model = cls(sr.N_TOKENS, 12, 2, 4, 128, 42, *sr.LAYERS, **kw)
    model.load_state_dict(recipe_model(cls, sr.SEED, sr.N_TOKENS, *sr.LAYERS).state_dict())
    state = sr.RECIPES[recipe]({k: v.detach().clone() for k, v in model.state_dict().items()})
    model.load_state_dict(state)
    return model, state


def main():
    _stub_fairseq()
    cls = _load(os.path.join(REF, "models", "HandPoseModels.py"), "ref_hpm").TextPoseTransformer
    rec = {"meta": np.array([sr.N_TOKENS, *sr.LAYERS, sr.SEED], np.int64)}
    for recipe in sr.RECIPES:
        _, state = stressed(cls, recipe)
        rec["sums_" + recipe] = np.array([v.double().sum().item() for v in state.values()])
    for case in INFER:
        recipe, shape, kind = case
        model, _ = stressed(cls, recipe)
        model.eval()
        tokens, pose = sr.case_inputs(recipe, shape, kind)
        with torch.no_grad():
            y32 = model(tokens, pose).contiguous()
            y64 = copy.deepcopy(model).double()(tokens, pose.double()).contiguous()
        name = sr.case_id(case)
        rec.update({"tokens_" + name: tokens.numpy(), "pose_" + name: pose.numpy(), "y32_" + name: y32.numpy(),
                    "y64_" + name: y64.numpy()})
        print(f"{name}: the reference's fp32 error {float((y32.double() - y64).abs().max()):.2e}")
    recipe, shape, kind = TRAIN
    model, _ = stressed(cls, recipe, dropout=0.0)
    model.train()
    tokens, x = sr.case_inputs(recipe, shape, kind)
    dy = torch.randn((shape[0], shape[2], 21, 2), generator=torch.Generator().manual_seed(sr.SEED + 2))
    out = {}
    for dtype in (torch.float64, torch.float32):
        m = copy.deepcopy(model).to(dtype).train()
        xx = x.to(dtype).clone().requires_grad_(True)
        y = m(tokens, xx)
        (y * dy.to(dtype)).sum().backward()
        out[dtype] = (y.detach(), {k: v.grad.double().numpy() for k, v in m.named_parameters()}, xx.grad.double().numpy())
    y64, g64, dx64 = out[torch.float64]
    _, g32, dx32 = out[torch.float32]
    rec.update(train_tokens=tokens.numpy(), train_x=x.numpy(), train_dy=dy.numpy(), train_y64=y64.numpy(), train_dx64=dx64,
               train_err32_dx=np.array(np.abs(dx32 - dx64).max()))
    for k, a in g64.items():
        rec["train_err32_" + k] = np.array(np.abs(g32[k] - a).max())
        rec["train_max64_" + k] = np.array(np.abs(a).max())
        if a.ndim == 1 or k.startswith(("token_embedding", "hidden2pose", "pose2hidden")):
            rec["train_g64_" + k] = a
    np.savez_compressed(OUT, **rec)
    assert os.path.getsize(OUT) <= 1000 * 1024, os.path.getsize(OUT)
    print(f"{os.path.basename(OUT)}: {os.path.getsize(OUT)} B")


if __name__ == "__main__":
    main()
