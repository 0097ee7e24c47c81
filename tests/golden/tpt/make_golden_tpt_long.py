#!/usr/bin/env python3
"""Generate tests/golden/tpt/long_default_b2_s40_t200.npz from the *reference*: its `TextPoseTransformer`
(body2hand/src/models/HandPoseModels.py:181-230, with the fairseq stub) at the shape its own CLIs feed by default
(`--max-frames 200`, 40 tokens), inside the item pipeline of infer_utterance.py:62-69 and traintest.py:255-271.

Runs ONLY where the reference checkout is available, like ../make_golden_tpt.py, whose weight recipe (seed 7, 1000
tokens, 4 + 4 layers; tests/tpt_ref.recipe_model regenerates it, so no weights are stored) and token staging it
repeats.  Per setting the reference's transform classes (steps/utils.py:180-210) are applied to each utterance's
item, the model runs in eval mode, and the prediction is scaled with `prediction *= 1280`:

    y32_norm,  y64_norm    NormalizeFixedFactor(1280) only -- the CLI default
    y32_chest, y64_chest   ChestDifference + NormalizeFixedFactor(1280) (`--dif-encoding`), then
                           mask_output(prediction, n_frames) (steps/utils.py:309-312) before the scaling

in float32 (the reference's own error) and float64 (the truth).  Stored besides: raw pixel `body` (2, 200, 12, 2),
`tokens` (2, 40), `n_frames`, meta = (B, S, T, n_tokens, n_enc, n_dec, seed).  The float32 run must stay within
3e-6 of the float64 one in normalised units (asserted here).

    python tests/golden/tpt/make_golden_tpt_long.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the loader helpers of the inference fixtures)
from make_golden_tpt import dataset_tokens, recipe_model  # noqa: E402

NAME = "long_default_b2_s40_t200"
B, S, T, N_TOKENS, N_ENC, N_DEC, SEED = 2, 40, 200, 1000, 4, 4, 7
FACTOR = 1280


def pipeline(utils, model, tokens, body, n_frames, chest, mask, dtype):
    m = copy.deepcopy(model).to(dtype).eval()
    transforms = ([utils.ChestDifference()] if chest else []) + [utils.NormalizeFixedFactor(FACTOR)]
    items = []
    for b in range(body.shape[0]):
        item = {"body_kp": torch.as_tensor(body[b]).to(dtype), "right_hand_kp": torch.zeros((T, 21, 2), dtype=dtype),
                "left_hand_kp": torch.zeros((T, 21, 2), dtype=dtype)}
        for t in transforms:
            item = t(item)
        items.append(item["body_kp"])
    with torch.no_grad():
        prediction = m(torch.as_tensor(tokens), torch.stack(items))
        if mask:
            prediction = utils.mask_output(prediction, n_frames)
        prediction *= FACTOR
    return prediction.numpy()


def main():
    mg._stub_fairseq()
    hpm = mg._load(os.path.join(mg.REF, "models", "HandPoseModels.py"), "ref_HandPoseModels")
    utils = mg._load(os.path.join(mg.REF, "steps", "utils.py"), "ref_steps_utils")
    model = recipe_model(hpm.TextPoseTransformer, SEED, N_TOKENS, N_ENC, N_DEC)
    gen = torch.Generator().manual_seed(SEED + 200)
    tokens = dataset_tokens(B, S, N_TOKENS, gen).numpy()
    body = (torch.rand((B, T, 12, 2), generator=gen) * FACTOR).numpy()
    n_frames = [T, 137]
    rec = dict(tokens=tokens, body=body, n_frames=np.array(n_frames, np.int64),
               meta=np.array([B, S, T, N_TOKENS, N_ENC, N_DEC, SEED], np.int64))
    for key, chest, mask in (("norm", False, False), ("chest", True, True)):
        y32 = pipeline(utils, model, tokens, body, n_frames, chest, mask, torch.float32)
        y64 = pipeline(utils, model, tokens, body, n_frames, chest, mask, torch.float64)
        err = np.abs(y32.astype(np.float64) - y64).max() / FACTOR
        print(f"{key}: max|y32 - y64| / {FACTOR} = {err:.3e}, max|y64| / {FACTOR} = {np.abs(y64).max() / FACTOR:.3f}")
        assert err <= 3e-6, err
        rec["y32_" + key], rec["y64_" + key] = y32, y64
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) <= 1024 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
