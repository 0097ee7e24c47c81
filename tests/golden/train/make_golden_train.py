#!/usr/bin/env python3
"""Generate the training fixtures (tests/golden/train/*.npz) from the *reference* model and losses.

Runs ONLY where the reference checkout is available, like ../make_golden.py, whose loader helpers it
imports.  It loads the reference's `ConvModel` (body2hand/src/models/HandPoseModels.py:17-64),
`mask_output`, `maskedPoseL1` and `poderatedPoseL1` (body2hand/src/steps/utils.py:309-312,413-452) by
file path and runs the training loop body of steps/traintest.py:111-121 under autograd on seeded data:

* in float64 -- the truth -- and in float32 -- the reference's own fp32 error;
* gradient cases: the eight parameter gradients and dL/dx of one loss evaluation in float64, and the
  float32 run's max-abs error against them per tensor;
* one trajectory case: 10 steps of the loop body with torch.optim.Adam (lr 2e-4, run.py:43-44),
  the losses and the final state.

The .npz files hold data only (inputs, state, lengths, scores, gradients, losses).  The tests that read
them live in tests/test_train_*.py; the subdirectory keeps them out of conftest.CONV_CASES, which globs
tests/golden/*.npz.

    python tests/golden/train/make_golden_train.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the loader helpers of the inference fixtures)

KEYS = ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias",
        "conv4.weight", "conv4.bias"]
LR = 2e-4


def _model(hpm, C, pos_emb, state, dtype):
    torch.manual_seed(0)
    m = hpm.ConvModel(C, "ReLU", pos_emb)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    m = m.to(dtype).train()
    if pos_emb:
        m.pos_emb.pe = m.pos_emb.pe.to(dtype)
    return m


def _step(utils, m, x, target, lengths, scores, loss_kind):
    """One evaluation of the loop body up to the loss (traintest.py:94-110)."""
    prediction = m(x)
    prediction = utils.mask_output(prediction, lengths)
    if loss_kind == "L1":
        return utils.maskedPoseL1()(prediction, target, lengths)
    return utils.poderatedPoseL1()(prediction, target, lengths, scores)


def _grads(utils, hpm, C, pos_emb, state, x, target, lengths, scores, loss_kind, dtype):
    m = _model(hpm, C, pos_emb, state, dtype)
    xx = torch.as_tensor(x).to(dtype).requires_grad_(True)
    loss = _step(utils, m, xx, torch.as_tensor(target).to(dtype), lengths, torch.as_tensor(scores).to(dtype),
                 loss_kind)
    loss.backward()
    sd = dict(m.named_parameters())
    # float64 truth kept as float64, the float32 run's values stored exactly as float32
    return loss.item(), [sd[k].grad.numpy() for k in KEYS], xx.grad.numpy()


def grad_case(utils, hpm, name, B, T, C, pos_emb, lengths, loss_kind, scale, seed):
    torch.manual_seed(seed)
    ref = hpm.ConvModel(C, "ReLU", pos_emb)
    state = {k: v.detach().numpy().copy() for k, v in ref.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    x = (torch.randn((B, T, 12, 2), generator=gen) * scale).numpy()
    target = (torch.randn((B, T, 21, 2), generator=gen) * scale).numpy()
    scores = torch.rand((B, T, 21), generator=gen).numpy()
    rec = {k.replace(".", "_"): v for k, v in state.items()}
    rec.update(x=x, target=target, scores=scores, lengths=np.array(lengths, np.int64),
               meta=np.array([B, T, C, int(pos_emb), seed], np.int64), loss_kind=np.array(loss_kind))
    loss64, g64, dx64 = _grads(utils, hpm, C, pos_emb, state, x, target, lengths, scores, loss_kind, torch.float64)
    loss32, g32, dx32 = _grads(utils, hpm, C, pos_emb, state, x, target, lengths, scores, loss_kind, torch.float32)
    rec.update(loss64=np.array(loss64), loss32=np.array(loss32), dx64=dx64,
               err32_dx=np.array(np.abs(dx32.astype(np.float64) - dx64).max()))
    # the float32 gradients enter the tests only through their error against float64 (the accuracy bar),
    # stored as one number per tensor: the full tensors would double the size of the wide cases
    for k, a, b in zip(KEYS, g64, g32):
        rec["g64_" + k.replace(".", "_")] = a
        rec["err32_" + k.replace(".", "_")] = np.array(np.abs(b.astype(np.float64) - a).max())
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
    print(f"{name}: loss {float(rec['loss64']):.6g}")


def trajectory_case(utils, hpm, name, B, T, C, lengths, steps, seed):
    torch.manual_seed(seed)
    ref = hpm.ConvModel(C, "ReLU", False)
    state = {k: v.detach().numpy().copy() for k, v in ref.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    x = (torch.rand((B, T, 12, 2), generator=gen) - 0.5).numpy()
    target = ((torch.rand((B, T, 21, 2), generator=gen) - 0.5) * 0.2).numpy()
    rec = {k.replace(".", "_"): v for k, v in state.items()}
    rec.update(x=x, target=target, lengths=np.array(lengths, np.int64),
               meta=np.array([B, T, C, 0, seed], np.int64), lr=np.array(LR), steps=np.array(steps))
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        m = _model(hpm, C, False, state, dt)
        opt = torch.optim.Adam(m.parameters(), lr=LR)
        xx, tt = torch.as_tensor(x).to(dt), torch.as_tensor(target).to(dt)
        losses = []
        for _ in range(steps):
            loss = _step(utils, m, xx, tt, lengths, None, "L1")
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        rec["losses" + tag] = np.array(losses)
        for k, v in m.state_dict().items():
            rec["final" + tag + "_" + k.replace(".", "_")] = v.numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
    print(f"{name}: losses {rec['losses64'][0]:.6g} -> {rec['losses64'][-1]:.6g}")


def main():
    mg._stub_fairseq()
    hpm = mg._load(os.path.join(mg.REF, "models", "HandPoseModels.py"), "ref_HandPoseModels")
    utils = mg._load(os.path.join(mg.REF, "steps", "utils.py"), "ref_steps_utils")
    # ragged lengths: 0 (no gradient; NaN loss for maskedPoseL1), > T (clamped as slicing does)
    grad_case(utils, hpm, "grad_c8_b3_t1", 3, 1, 8, False, [1, 0, 5], "confL1", 1.0, 300)
    grad_case(utils, hpm, "grad_c8_b3_t5", 3, 5, 8, False, [5, 0, 9], "L1", 1.0, 301)
    grad_case(utils, hpm, "grad_c30_b3_t9", 3, 9, 30, False, [9, 4, 0], "confL1", 1.0, 302)
    grad_case(utils, hpm, "grad_c30_b3_t5", 3, 5, 30, False, [2, 7, 5], "L1", 1.0 / 1280, 306)
    grad_case(utils, hpm, "grad_c30_b2_t100_posemb", 2, 100, 30, True, [100, 57], "L1", 1.0 / 1280, 303)
    grad_case(utils, hpm, "grad_c30_b2_t201", 2, 201, 30, False, [201, 130], "L1", 1.0, 304)
    grad_case(utils, hpm, "grad_c64_b2_t100_posemb", 2, 100, 64, True, [64, 300], "confL1", 1.0, 305)
    trajectory_case(utils, hpm, "traj_c30_b4_t64", 4, 64, 30, [64, 40, 17, 64], 10, 310)


if __name__ == "__main__":
    main()
