#!/usr/bin/env python3
"""Generate the TextPoseTransformer training fixtures (tests/golden/tpt/train_*.npz) from the *reference* class.

Runs ONLY where the reference checkout is available, like ../make_golden_tpt.py, whose weight recipe it repeats,
and ../make_golden.py, whose loader helpers it imports.  It loads the reference's `TextPoseTransformer`
(body2hand/src/models/HandPoseModels.py:181-230, with the fairseq stub), `mask_output` and `maskedPoseL1`
(body2hand/src/steps/utils.py:309-312,413-428) by file path and runs the loop body of steps/traintest.py:105-121
up to loss.backward() in `.train()` mode with dropout = 0.0 -- the one setting in which the class itself is an
exact reference -- on seeded data, in float64 (the truth) and in float32 (the reference's own fp32 error).

Stored: tokens, x, target, lengths, meta = (B, S, T, n_tokens, n_enc, n_dec, seed), loss64, loss32, dx64,
`err32_<name>` (the float32 run's max-abs error) for every parameter and for dx, the float64 `sum` of every
parameter (`sums`, in named_parameters() order: pins the recipe), and the float64 gradient `g64_<name>` of every
parameter, or (`small=True`) of the 1-D parameters, the embedding and the two projections only.  The weights
are NOT stored: the recipe (tests/tpt_ref.recipe_model) regenerates them.  Every file stays below 1000 KiB: a
fixture continues in `<name>.partN.npz`.

    python tests/golden/tpt/make_golden_tpt_train.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the loader helpers of the inference fixtures)
from make_golden_tpt import dataset_tokens  # noqa: E402

LIMIT = 1000 * 1024   # bytes per committed file


def recipe_model(cls, seed, n_tokens, n_enc, n_dec):
    """make_golden_tpt.recipe_model with dropout = 0.0 (the constructor draws the same initial weights), .train()."""
    torch.manual_seed(seed)
    model = cls(n_tokens, 12, 2, 4, 128, 42, n_enc, n_dec, dropout=0.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, p in model.named_parameters():
            p += 0.05 * torch.randn(p.shape, generator=g)
    return model.train()


def _run(utils, model, tokens, x, target, lengths, dtype):
    m = copy.deepcopy(model).to(dtype).train()
    xx = torch.as_tensor(x).to(dtype).requires_grad_(True)
    prediction = m(torch.as_tensor(tokens), xx)
    prediction = utils.mask_output(prediction, lengths)
    loss = utils.maskedPoseL1()(prediction, torch.as_tensor(target).to(dtype), lengths)
    loss.backward()
    return loss.item(), {k: v.grad.numpy() for k, v in m.named_parameters()}, xx.grad.numpy()


def case(utils, cls, name, B, S, T, n_tokens, n_enc, n_dec, lengths, scale, seed, small):
    model = recipe_model(cls, seed, n_tokens, n_enc, n_dec)
    gen = torch.Generator().manual_seed(seed + 2)
    tokens = dataset_tokens(B, S, n_tokens, gen).numpy()
    x = (torch.randn((B, T, 12, 2), generator=gen) * scale).numpy()
    target = (torch.randn((B, T, 21, 2), generator=gen) * scale).numpy()
    loss64, g64, dx64 = _run(utils, model, tokens, x, target, lengths, torch.float64)
    loss32, g32, dx32 = _run(utils, model, tokens, x, target, lengths, torch.float32)
    rec = dict(tokens=tokens, x=x, target=target, lengths=np.array(lengths, np.int64),
               meta=np.array([B, S, T, n_tokens, n_enc, n_dec, seed], np.int64),
               sums=np.array([p.double().sum().item() for _, p in model.named_parameters()]),
               loss64=np.array(loss64), loss32=np.array(loss32), dx64=dx64,
               err32_dx=np.array(np.abs(dx32.astype(np.float64) - dx64).max()))
    for k, a in g64.items():
        rec["err32_" + k] = np.array(np.abs(g32[k].astype(np.float64) - a).max())
    keep = [k for k, a in g64.items() if not small or a.ndim == 1 or k.startswith(("token_embedding", "hidden2pose", "pose2hidden"))]
    parts, size = [rec], sum(v.nbytes for v in rec.values())
    for k in keep:
        a = g64[k]
        if size + a.nbytes > LIMIT:
            parts.append({})
            size = 0
        parts[-1]["g64_" + k] = a
        size += a.nbytes
    for i, part in enumerate(parts):
        path = os.path.join(HERE, name + (f".part{i + 1}" if i else "") + ".npz")
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path))
    print(f"{name}: loss {loss64:.6g}, {len(parts)} file(s)")


def main():
    mg._stub_fairseq()
    hpm = mg._load(os.path.join(mg.REF, "models", "HandPoseModels.py"), "ref_HandPoseModels")
    utils = mg._load(os.path.join(mg.REF, "steps", "utils.py"), "ref_steps_utils")
    cls = hpm.TextPoseTransformer
    case(utils, cls, "train_e1_d1_b3_s9_t17", 3, 9, 17, 50, 1, 1, [17, 5, 30], 1.0, 500, small=False)
    case(utils, cls, "train_e2_d2_b2_s40_t100", 2, 40, 100, 50, 2, 2, [100, 57], 1.0 / 1280, 501, small=True)


if __name__ == "__main__":
    main()
