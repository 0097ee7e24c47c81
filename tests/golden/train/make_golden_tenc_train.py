#!/usr/bin/env python3
"""Generate the TransformerEnc training fixtures (tests/golden/train/tenc_grad_*.npz) from the *reference* class.

Runs ONLY where the reference checkout is available, like ../make_golden.py, whose loader helpers it imports.
It loads the reference's `TransformerEnc` (body2hand/src/models/HandPoseModels.py:118-178, with the fairseq
stub), `mask_output` and `maskedPoseL1` (body2hand/src/steps/utils.py:309-312,413-428) by file path and runs
the loop body of steps/traintest.py:94-121 up to loss.backward() in `.train()` mode with dropout = 0.0 -- the
one setting in which the class itself is an exact reference -- on seeded data, in float64 (the truth) and in
float32 (the reference's own fp32 error).

Stored: x, target, lengths, meta = (B, T, nlayers, seed), loss64, the float64 gradient of every parameter
(`g64_<name>`), dx64 and the float32 run's max-abs error per tensor (`err32_<name>`, `err32_dx`).  The state is
NOT stored: torch.manual_seed(seed) + the constructor regenerates it bit for bit.  A fixture whose float64
gradients exceed 1 MiB continues in `<name>.part2.npz`.

    python tests/golden/train/make_golden_tenc_train.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the loader helpers of the inference fixtures)

LIMIT = 1000 * 1024   # bytes per committed file


def _run(utils, hpm, nlayers, seed, x, target, lengths, dtype):
    torch.manual_seed(seed)
    m = hpm.TransformerEnc(ninp=24, nhead=4, nhid=128, nout=42, nlayers=nlayers, dropout=0.0).to(dtype).train()
    xx = torch.as_tensor(x).to(dtype).requires_grad_(True)
    prediction = m(xx)
    prediction = utils.mask_output(prediction, lengths)
    loss = utils.maskedPoseL1()(prediction, torch.as_tensor(target).to(dtype), lengths)
    loss.backward()
    return loss.item(), {k: v.grad.numpy() for k, v in m.named_parameters()}, xx.grad.numpy()


def case(utils, hpm, name, B, T, nlayers, lengths, scale, seed):
    gen = torch.Generator().manual_seed(seed + 1)
    x = (torch.randn((B, T, 12, 2), generator=gen) * scale).numpy()
    target = (torch.randn((B, T, 21, 2), generator=gen) * scale).numpy()
    loss64, g64, dx64 = _run(utils, hpm, nlayers, seed, x, target, lengths, torch.float64)
    loss32, g32, dx32 = _run(utils, hpm, nlayers, seed, x, target, lengths, torch.float32)
    rec = dict(x=x, target=target, lengths=np.array(lengths, np.int64), meta=np.array([B, T, nlayers, seed], np.int64),
               loss64=np.array(loss64), loss32=np.array(loss32), dx64=dx64,
               err32_dx=np.array(np.abs(dx32.astype(np.float64) - dx64).max()))
    for k, a in g64.items():
        rec["err32_" + k] = np.array(np.abs(g32[k].astype(np.float64) - a).max())
    parts, size = [rec], sum(v.nbytes for v in rec.values())
    for k, a in g64.items():
        if size + a.nbytes > LIMIT:
            parts.append({})
            size = 0
        parts[-1]["g64_" + k] = a
        size += a.nbytes
    for i, part in enumerate(parts):
        np.savez_compressed(os.path.join(HERE, name + (f".part{i + 1}" if i else "") + ".npz"), **part)
    print(f"{name}: loss {loss64:.6g}, {len(parts)} file(s)")


def main():
    mg._stub_fairseq()
    hpm = mg._load(os.path.join(mg.REF, "models", "HandPoseModels.py"), "ref_HandPoseModels")
    utils = mg._load(os.path.join(mg.REF, "steps", "utils.py"), "ref_steps_utils")
    case(utils, hpm, "tenc_grad_l1_b3_t17", 3, 17, 1, [17, 5, 30], 1.0, 400)
    case(utils, hpm, "tenc_grad_l2_b2_t100", 2, 100, 2, [100, 57], 1.0 / 1280, 401)


if __name__ == "__main__":
    main()
