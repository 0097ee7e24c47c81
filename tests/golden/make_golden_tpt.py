#!/usr/bin/env python3
"""Generate the TextPoseTransformer fixtures (tests/golden/tpt/*.npz) from the *reference* model.

Runs only where the reference checkout is present.  It imports the reference's `TextPoseTransformer`
(body2hand/src/models/HandPoseModels.py:181-230) by file path, with make_golden.py's stub for the absent
`fairseq` package, and runs it on the CPU in float32 and, as a deep copy in `.double()`, in float64.
Nothing of the reference (source or bytecode) is copied: the .npz files hold data only.

The default model's weights (4.8 MB) are not stored but reproduced by this recipe, which tests/tpt_ref.py
repeats for the mirror:
    1. torch.manual_seed(seed)
    2. construct the model
    3. g = torch.Generator().manual_seed(seed + 1)
    4. for every named_parameters() entry in order: p += 0.05 * torch.randn(p.shape, generator=g)
       (attention biases, LayerNorm gains and biases become non-default)
    5. eval()
Every fixture stores the float64 `sum` and `abs().sum()` of every state_dict entry, so a test can assert that
the mirror built by the same recipe holds the same weights.  One small model is stored whole.

    python tests/golden/make_golden_tpt.py          # rewrites tests/golden/tpt/*.npz
"""
import copy
import os

import numpy as np
import torch

from make_golden import REF, _load, _stub_fairseq

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tpt")
SEED = 7
MAX_REF_ERR = 2e-6     # the condition tests/test_tpt_cpu.py places on every fixture
PART_BYTES = 600_000   # weights of the stored model that go into the first of its two files


def recipe_model(cls, seed, n_tokens, n_enc, n_dec):
    torch.manual_seed(seed)
    model = cls(n_tokens, 12, 2, 4, 128, 42, n_enc, n_dec)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, p in model.named_parameters():
            p += 0.05 * torch.randn(p.shape, generator=g)
    return model.eval()


def dataset_tokens(B, S, n_tokens, gen):
    """Shaped like the dataset's (text_pose_dataset.py:467-470): a random-length prefix of ids, then zeros."""
    tok = torch.zeros((B, S), dtype=torch.int64)
    for b in range(B):
        n = int(torch.randint(1, S + 1, (1,), generator=gen))
        tok[b, :n] = torch.randint(1, n_tokens, (n,), generator=gen)
    return tok


def case(model, name, tokens, pose, geom, store_weights=False):
    """name -> (records of the fixture's files, the reference's own fp32 error)."""
    with torch.no_grad():
        y32 = model(tokens, pose).contiguous()
        y64 = copy.deepcopy(model).double()(tokens, pose.double()).contiguous()
    sd = model.state_dict()
    rec = {"tokens": tokens.numpy(), "pose": pose.numpy(), "y32": y32.numpy(), "y64": y64.numpy(),
           "meta": np.array(list(tokens.shape) + [pose.shape[1]] + list(geom), dtype=np.int64),  # B, S, T, n_tokens, n_enc, n_dec, seed
           "keys": np.array(list(sd)),
           "shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()]),
           "sums": np.array([v.double().sum().item() for v in sd.values()]),
           "abs_sums": np.array([v.double().abs().sum().item() for v in sd.values()])}
    files = {name: rec}
    if store_weights:  # w000, w001, ... in state_dict order, over two files: random floats do not compress
        files[name + ".part2"] = part2 = {}
        stored = 0
        for i, v in enumerate(sd.values()):
            (rec if stored < PART_BYTES else part2)[f"w{i:03d}"] = v.numpy()
            stored += 4 * v.numel()
    return files, float((y32.double() - y64).abs().max())


def write(files):
    os.makedirs(OUT, exist_ok=True)
    for name, rec in files.items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) <= 1 << 20, (name, os.path.getsize(path))
        print(f"{name}: {os.path.getsize(path)} B")


def main():
    _stub_fairseq()
    hpm = _load(os.path.join(REF, "models", "HandPoseModels.py"), "ref_hpm")
    cls = hpm.TextPoseTransformer
    model = recipe_model(cls, SEED, 1000, 4, 4)
    small = recipe_model(cls, SEED + 10, 50, 1, 1)
    geom = (1000, 4, 4, SEED)
    # The tests require max|y32 - y64| <= MAX_REF_ERR of every fixture, so that their GPU bound of 2e-5 against y64
    # stays at least ten times the reference's own fp32 error.  That error depends on the inputs (1.3e-6 .. 3.1e-6
    # over eight draws of the (3, 40, 100) case): the inputs are the first draw, counting generator seeds from 100,
    # for which all four cases meet the condition.
    for input_seed in range(100, 200):
        gen = torch.Generator().manual_seed(input_seed)
        cases = [
            case(model, "default_b3_s40_t100", dataset_tokens(3, 40, 1000, gen),
                 torch.rand((3, 100, 12, 2), generator=gen) - 0.5, geom),
            case(model, "default_b2_s17_t33", torch.randint(0, 1000, (2, 17), generator=gen),
                 0.3 * torch.randn((2, 33, 12, 2), generator=gen), geom),
            case(model, "default_b2_s1_t1", torch.randint(0, 1000, (2, 1), generator=gen),
                 torch.rand((2, 1, 12, 2), generator=gen) - 0.5, geom),
            case(small, "small_weights_b2_s9_t20", torch.randint(0, 50, (2, 9), generator=gen),
                 torch.rand((2, 20, 12, 2), generator=gen) - 0.5, (50, 1, 1, SEED + 10), store_weights=True)]
        errs = [e for _, e in cases]
        print(f"input seed {input_seed}: the reference's fp32 error per case", " ".join(f"{e:.2e}" for e in errs))
        if max(errs) <= MAX_REF_ERR:
            break
    else:
        raise SystemExit("no input draw meets the condition")
    for files, _ in cases:
        write(files)


if __name__ == "__main__":
    main()
