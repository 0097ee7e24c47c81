#!/usr/bin/env python3
"""GPU box: one training step of TextPoseTransformer (kernel_tpt_train.h, kernel_tenc_train.h, and
kernel_train_attn_long.h beyond 128 frames, or kernel_train_attn_mfma.h there with kernels=mfma; the Linear layers on
kernel_train_linear_mfma.h with linear=mfma), one JSON line.
Context only: the training kernels are plain per-operation fp32 kernels and carry no speed bar.
  * one full step of the reference loop body (steps/traintest.py:105-121), 4 + 4 layers, n_tokens = 1000,
    dropout 0.1: forward (masks drawn by torch), mask_output, maskedPoseL1, backward, torch.optim.Adam (lr 2e-4),
    steady state, HIP events, the median (and the minimum) of `reps` repetitions of ten steps;
  * the same step with torch-ROCm's own nn.Transformer (the reference's model restated with torch modules) on
    the same GPU.
The two shapes of the record (DESIGN.md sections 13 and 16):
    python tools/bench_train_tpt.py                  B x S x T = 128 x 40 x 100, 12 joints (the datasets' 100 frames)
    python tools/bench_train_tpt.py 128 40 200 8     the trainer's default batch: --max-frames 200, geometry (8, 42)
    python tools/bench_train_tpt.py 128 40 200 8 5 mfma   the same with model.set_train_kernels("mfma")
    python tools/bench_train_tpt.py 128 40 200 8 5 mfma mfma   and with model.set_train_linear("mfma") (section 19)
    python tools/bench_train_tpt.py 128 40 200 8 5 mfma mfma native   and with model.set_dropout_source("native") (section 20)
    python tools/bench_train_tpt.py 128 40 200 8 5 mfma mfma native native   and with hps.Adam as the optimizer (section 21)
    python tools/bench_train_tpt.py [B=128] [S=40] [T=100] [n_joints=12] [reps=5] [kernels=valu|mfma] [linear=valu|mfma]
                                    [dropout_source=torch|native] [optimizer=torch|native]
The optimizer argument concerns the library's step only; torch-ROCm's own model always steps with torch.optim.Adam."""
import json
import os
import sys
import warnings

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hand_pose_sl_amd as hps  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
S = int(sys.argv[2]) if len(sys.argv) > 2 else 40
T = int(sys.argv[3]) if len(sys.argv) > 3 else 100
J = int(sys.argv[4]) if len(sys.argv) > 4 else 12
REPS = int(sys.argv[5]) if len(sys.argv) > 5 else 5
KERNELS = sys.argv[6] if len(sys.argv) > 6 else "valu"
LINEAR = sys.argv[7] if len(sys.argv) > 7 else None    # absent: the model's default, and no key in the record
DROPOUT_SOURCE = sys.argv[8] if len(sys.argv) > 8 else None    # absent: the model's default, and no key in the record
OPTIMIZER = sys.argv[9] if len(sys.argv) > 9 else None    # absent: torch.optim.Adam, and no key in the record
if OPTIMIZER not in (None, "torch", "native"):
    sys.exit(f"optimizer must be torch or native, got {OPTIMIZER!r}")
N_TOKENS, L, P, LR = 1000, 4, 0.1, 2e-4
dev = torch.device("cuda:0")


SPREAD = []  # the slowest repetition of each events_ms call, in call order


def events_ms(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    ms.sort()
    SPREAD.append(ms[-1])
    return ms[len(ms) // 2], ms[0]


class TorchTpt(nn.Module):
    """The reference's TextPoseTransformer.forward (HandPoseModels.py:201-222) with torch's own modules."""

    def __init__(self):
        super().__init__()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            self.tr = nn.Transformer(128, 4, L, L, 128, dropout=P)
        self.emb = nn.Embedding(N_TOKENS, 128)
        self.h2p = nn.Linear(128, 42)
        self.p2h = nn.Linear(2 * J, 128)

    def forward(self, tok, pose):
        b, t = pose.shape[0], pose.shape[1]
        tgt = self.p2h(pose.view(b, t, 2 * J).permute(1, 0, 2))
        return self.h2p(self.tr(self.emb(tok).permute(1, 0, 2), tgt)).permute(1, 0, 2).reshape(b, t, 21, 2)


torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore", UserWarning)
    m = hps.TextPoseTransformer(N_TOKENS, J, 2, 4, 128, 42, L, L, dropout=P).to(dev).train()
m.set_train_kernels(KERNELS)
if LINEAR is not None:
    m.set_train_linear(LINEAR)
if DROPOUT_SOURCE is not None:
    m.set_dropout_source(DROPOUT_SOURCE, seed=0)
g = torch.Generator(device=dev).manual_seed(1)
lengths = [T - (i * 37) % (T // 2 + 1) for i in range(B)]
toks = torch.randint(0, N_TOKENS, (B, S), device=dev, generator=g)
xs = torch.rand((B, T, J, 2), device=dev, generator=g) - 0.5
ts = (torch.rand((B, T, 21, 2), device=dev, generator=g) - 0.5) * 0.2
crit = hps.maskedPoseL1()


def make_step(forward, params, optimizer=None):
    opt = (hps.Adam if optimizer == "native" else torch.optim.Adam)(params, lr=LR)

    def step():
        prediction = forward(toks, xs)
        for i, n in enumerate(lengths):
            prediction[i, n:, :] = 0
        loss = crit(prediction, ts, lengths)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


out = {"B": B, "S": S, "T": T, "n_joints": J, "n_enc": L, "n_dec": L, "n_tokens": N_TOKENS, "dropout": P, "reps": REPS,
       "kernels": KERNELS}
if LINEAR is not None:
    out["linear"] = LINEAR
if DROPOUT_SOURCE is not None:
    out["dropout_source"] = DROPOUT_SOURCE
if OPTIMIZER is not None:
    out["optimizer"] = OPTIMIZER
out["reference_step_ms"], out["reference_step_ms_min"] = events_ms(make_step(m, list(m.parameters()), OPTIMIZER), 10)
out["reference_step_ms_max"] = SPREAD[0]
tm = TorchTpt().to(dev).train()
out["torch_rocm_nn_transformer_step_ms_context_only"], out["torch_rocm_nn_transformer_step_ms_min"] = events_ms(
    make_step(tm, list(tm.parameters())), 10)
print(json.dumps(out))
