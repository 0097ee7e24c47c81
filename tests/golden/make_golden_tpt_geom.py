#!/usr/bin/env python3
"""Generate the fixtures of TextPoseTransformer's other geometries from the *reference* classes:
tests/golden/tpt/geom_*.npz, tests/golden/tpt/geom_train_*.npz and tests/golden/metric_j*_b5_t60.npz.

Runs only where the reference checkout is present, like make_golden_tpt.py, whose weight recipe it repeats with
the geometry as a parameter (tests/tpt_geom_ref.py repeats it for the mirror), and make_golden.py, whose loader
helpers and `fairseq` stub it imports.  Nothing of the reference (source or bytecode) is copied: the .npz files
hold data only -- inputs, outputs and per-tensor float64 checksums; the weights are reproduced by the recipe.

The reference's CLIs build the class in four geometries (n_joints, nout): (12, 42) infer_utterance.py:79-80 -- the
one make_golden_tpt.py covers --, (8, 42) run.py:100-101, (29, 8) run.py:92-93 and (21, 24) run.py:96-97.

  geom_j<n_joints>_o<nout>_b<B>_s<S>_t<T>_e<n_enc>_d<n_dec>.npz
      tokens, pose, y32, y64, meta = (B, S, T, n_tokens, n_enc, n_dec, seed, n_joints, nout), keys, shapes, sums,
      abs_sums (of every state_dict entry, float64).  Every case meets make_golden_tpt.MAX_REF_ERR.
  geom_train_j29_o8_b3_s9_t17.npz
      the loop body of steps/traintest.py:105-121 up to loss.backward() with mask_output and maskedPoseL1, float64
      and float32, dropout 0.0: what make_golden_tpt_train.py stores, with the gradients of the two projections and of
      token_embedding.
  metric_j<J>_b5_t60.npz, J = 4 and 12
      maskedPoseL1 and poderatedPoseL1 (steps/utils.py:413-452) and L12Pixels(J, 1280) (:291-299) on ragged lengths
      with one empty sequence, whose mean the reference makes NaN (and the batch loss with it): `*_valid` are the
      same losses over the four non-empty sequences.

    python tests/golden/make_golden_tpt_geom.py
"""
import copy
import os
import warnings

import numpy as np
import torch

from make_golden import REF, _load, _stub_fairseq
from make_golden_tpt import MAX_REF_ERR, dataset_tokens

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "tpt")
SEED, INPUT_SEED, N_TOKENS = 7, 11, 60
GEOMETRIES = [(8, 42), (29, 8), (21, 24)]                      # (n_joints, nout): run.py:100-101, :92-93, :96-97
SHAPES = [(3, 9, 17, 1, 1), (2, 17, 33, 4, 4)]                 # (B, S, T, n_enc, n_dec)
LONG = ((29, 8), (2, 40, 130, 2, 2))                           # beyond 128 frames: the long-attention path
LIMIT = 1 << 20


def recipe_model(cls, seed, n_tokens, n_joints, nout, n_enc, n_dec, **kw):
    """make_golden_tpt.recipe_model with the geometry as a parameter."""
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        model = cls(n_tokens, n_joints, 2, 4, 128, nout, n_enc, n_dec, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, p in model.named_parameters():
            p += 0.05 * torch.randn(p.shape, generator=g)
    return model.eval()


def case_name(n_joints, nout, B, S, T, n_enc, n_dec):
    return f"geom_j{n_joints}_o{nout}_b{B}_s{S}_t{T}_e{n_enc}_d{n_dec}"


def save(path, rec):
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path))
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} B")


def forward_case(cls, n_joints, nout, B, S, T, n_enc, n_dec):
    model = recipe_model(cls, SEED, N_TOKENS, n_joints, nout, n_enc, n_dec)
    for input_seed in range(INPUT_SEED, INPUT_SEED + 50):  # the first draw that meets the condition; 11 for all of them
        gen = torch.Generator().manual_seed(input_seed)
        tokens = torch.randint(0, N_TOKENS, (B, S), generator=gen)
        pose = torch.rand((B, T, n_joints, 2), generator=gen) - 0.5
        with torch.no_grad():
            y32 = model(tokens, pose).contiguous()
            y64 = copy.deepcopy(model).double()(tokens, pose.double()).contiguous()
        err = float((y32.double() - y64).abs().max())
        print(f"({n_joints}, {nout}) at {(B, S, T, n_enc, n_dec)}, input seed {input_seed}: the reference's fp32 error {err:.2e}")
        if err <= MAX_REF_ERR:
            break
    else:
        raise SystemExit("no input draw meets the condition")
    sd = model.state_dict()
    save(os.path.join(OUT, case_name(n_joints, nout, B, S, T, n_enc, n_dec) + ".npz"),
         {"tokens": tokens.numpy(), "pose": pose.numpy(), "y32": y32.numpy(), "y64": y64.numpy(),
          "meta": np.array([B, S, T, N_TOKENS, n_enc, n_dec, SEED, n_joints, nout, input_seed], dtype=np.int64),
          "keys": np.array(list(sd)),
          "shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()]),
          "sums": np.array([v.double().sum().item() for v in sd.values()]),
          "abs_sums": np.array([v.double().abs().sum().item() for v in sd.values()])})


def _train_run(utils, model, tokens, x, target, lengths, dtype):
    m = copy.deepcopy(model).to(dtype).train()
    xx = torch.as_tensor(x).to(dtype).requires_grad_(True)
    prediction = utils.mask_output(m(torch.as_tensor(tokens), xx), lengths)
    loss = utils.maskedPoseL1()(prediction, torch.as_tensor(target).to(dtype), lengths)
    loss.backward()
    return loss.item(), {k: v.grad.numpy() for k, v in m.named_parameters()}, xx.grad.numpy()


def train_case(utils, cls, n_joints, nout, B, S, T, lengths, seed):
    model = recipe_model(cls, seed, 50, n_joints, nout, 1, 1, dropout=0.0).train()
    gen = torch.Generator().manual_seed(seed + 2)
    tokens = dataset_tokens(B, S, 50, gen).numpy()
    x = torch.randn((B, T, n_joints, 2), generator=gen).numpy()
    target = torch.randn((B, T, nout // 2, 2), generator=gen).numpy()
    loss64, g64, dx64 = _train_run(utils, model, tokens, x, target, lengths, torch.float64)
    loss32, g32, dx32 = _train_run(utils, model, tokens, x, target, lengths, torch.float32)
    rec = dict(tokens=tokens, x=x, target=target, lengths=np.array(lengths, np.int64),
               meta=np.array([B, S, T, 50, 1, 1, seed, n_joints, nout], np.int64),
               sums=np.array([p.double().sum().item() for _, p in model.named_parameters()]),
               loss64=np.array(loss64), loss32=np.array(loss32), dx64=dx64,
               err32_dx=np.array(np.abs(dx32.astype(np.float64) - dx64).max()))
    for k, a in g64.items():
        rec["err32_" + k] = np.array(np.abs(g32[k].astype(np.float64) - a).max())
        if k.startswith(("token_embedding", "hidden2pose", "pose2hidden")):
            rec["g64_" + k] = a
    save(os.path.join(OUT, f"geom_train_j{n_joints}_o{nout}_b{B}_s{S}_t{T}.npz"), rec)


def metric_case(utils, J, B, T, lengths, seed):
    gen = torch.Generator().manual_seed(seed)
    pred = torch.rand((B, T, J, 2), generator=gen) - 0.5
    tgt = torch.rand((B, T, J, 2), generator=gen) - 0.5
    scores = torch.rand((B, T, J), generator=gen)
    valid = [i for i, n in enumerate(lengths) if n > 0]
    vl = [lengths[i] for i in valid]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the mean of the empty sequence
        loss = utils.maskedPoseL1()(pred, tgt, lengths)
        wloss = utils.poderatedPoseL1()(pred, tgt, lengths, scores)
        per_seq = torch.stack([torch.nn.functional.l1_loss(pred[i, :n], tgt[i, :n]) for i, n in enumerate(lengths)])
        wper_seq = torch.stack([torch.nn.functional.l1_loss(pred[i, :n] * scores[i, :n].unsqueeze(2),
                                                            tgt[i, :n] * scores[i, :n].unsqueeze(2))
                                for i, n in enumerate(lengths)])
    loss_valid = utils.maskedPoseL1()(pred[valid], tgt[valid], vl)
    wloss_valid = utils.poderatedPoseL1()(pred[valid], tgt[valid], vl, scores[valid])
    pix = utils.L12Pixels(J, 1280)(loss_valid)
    save(os.path.join(HERE, f"metric_j{J}_b{B}_t{T}.npz"),
         dict(pred=pred.numpy(), target=tgt.numpy(), scores=scores.numpy(), lengths=np.array(lengths, dtype=np.int64),
              valid=np.array(valid, dtype=np.int64), loss=loss.numpy(), per_seq=per_seq.numpy(), wloss=wloss.numpy(),
              wper_seq=wper_seq.numpy(), loss_valid=loss_valid.numpy(), wloss_valid=wloss_valid.numpy(),
              pixels_valid=pix.numpy(), meta=np.array([B, T, J, seed], dtype=np.int64)))


def main():
    _stub_fairseq()
    hpm = _load(os.path.join(REF, "models", "HandPoseModels.py"), "ref_hpm")
    utils = _load(os.path.join(REF, "steps", "utils.py"), "ref_steps_utils")
    cls = hpm.TextPoseTransformer
    os.makedirs(OUT, exist_ok=True)
    for n_joints, nout in GEOMETRIES:
        for shape in SHAPES:
            forward_case(cls, n_joints, nout, *shape)
    forward_case(cls, *LONG[0], *LONG[1])
    train_case(utils, cls, 29, 8, 3, 9, 17, [17, 5, 30], 502)
    metric_case(utils, 4, 5, 60, [60, 0, 33, 59, 17], 41)
    metric_case(utils, 12, 5, 60, [60, 0, 33, 59, 17], 43)


if __name__ == "__main__":
    main()
