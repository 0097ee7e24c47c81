#!/usr/bin/env python3
"""GPU box: one training step of TransformerEnc (kernel_tenc_train.h), one JSON line.  Context only: the
training kernels are plain per-operation fp32 kernels and carry no speed bar.
  * one full step of the reference loop body (steps/traintest.py:94-121) at B x T = 128 x 100, 4 layers,
    dropout 0.1: forward (masks drawn by torch), mask_output, maskedPoseL1, backward, torch.optim.Adam
    (lr 2e-4), steady state, HIP events;
  * the same step with torch-ROCm's own nn.TransformerEncoder (the reference's model restated with torch
    modules) on the same GPU;
  * the same step of the tests' torch port (tests/tenc_train_ref.py) on the host CPU.
    python tools/bench_train_tenc.py [B=128] [T=100] [dropout_source=torch|native] [optimizer=torch|native]
                                     [train_kernels=valu|mfma] [train_linear=valu|mfma]
The third argument selects model.set_dropout_source, the fourth the optimizer of the library's
step, torch.optim.Adam or hps.Adam (section 21), the fifth and sixth model.set_train_kernels and
model.set_train_linear (section 25); each is recorded only when given.  With the fifth or sixth given, the record also
holds `reference_step_ms_repetitions`: five further repetitions of 20 steps each, for a median and a range."""
import json
import os
import sys
import time
import warnings

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hand_pose_sl_amd as hps  # noqa: E402
from tenc_train_ref import leaf_state, param_keys, port_forward  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
DROPOUT_SOURCE = sys.argv[3] if len(sys.argv) > 3 else None    # absent: the model's default, and no key in the record
OPTIMIZER = sys.argv[4] if len(sys.argv) > 4 else None    # absent: torch.optim.Adam, and no key in the record
TRAIN_KERNELS = sys.argv[5] if len(sys.argv) > 5 else None    # absent: the model's default, and no key in the record
TRAIN_LINEAR = sys.argv[6] if len(sys.argv) > 6 else None
if OPTIMIZER not in (None, "torch", "native"):
    sys.exit(f"optimizer must be torch or native, got {OPTIMIZER!r}")
L, P, LR = 4, 0.1, 2e-4
dev = torch.device("cuda:0")


def events_ms(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / iters
        best = ms if best is None else min(best, ms)
    return best


class TorchEnc(nn.Module):
    """The reference's TransformerEnc.forward (HandPoseModels.py:154-178) with torch's own modules."""

    def __init__(self):
        super().__init__()
        self.drop = nn.Dropout(P)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            self.enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(128, 4, 128, P), L)
        self.h2p = nn.Linear(128, 42)
        self.p2h = nn.Linear(24, 128)

    def forward(self, src, pe):
        b, t = src.shape[0], src.shape[1]
        h = self.drop(src.view(b, t, 24).permute(1, 0, 2) + pe[:t])
        return self.h2p(self.enc(self.p2h(h))).permute(1, 0, 2).reshape(b, t, 21, 2)


torch.manual_seed(0)
m = hps.TransformerEnc(24, 4, 128, 42, L, dropout=P).to(dev).train()
if DROPOUT_SOURCE is not None:
    m.set_dropout_source(DROPOUT_SOURCE, seed=0)
if TRAIN_KERNELS is not None:
    m.set_train_kernels(TRAIN_KERNELS)
if TRAIN_LINEAR is not None:
    m.set_train_linear(TRAIN_LINEAR)
g = torch.Generator(device=dev).manual_seed(1)
lengths = [T - (i * 37) % (T // 2 + 1) for i in range(B)]
xs = torch.rand((B, T, 12, 2), device=dev, generator=g) - 0.5
ts = (torch.rand((B, T, 21, 2), device=dev, generator=g) - 0.5) * 0.2
crit = hps.maskedPoseL1()


def make_step(forward, params, optimizer=None):
    opt = (hps.Adam if optimizer == "native" else torch.optim.Adam)(params, lr=LR)

    def step():
        prediction = forward(xs)
        for i, n in enumerate(lengths):
            prediction[i, n:, :] = 0
        loss = crit(prediction, ts, lengths)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


out = {"B": B, "T": T, "nlayers": L, "dropout": P}
if DROPOUT_SOURCE is not None:
    out["dropout_source"] = DROPOUT_SOURCE
if OPTIMIZER is not None:
    out["optimizer"] = OPTIMIZER
if TRAIN_KERNELS is not None:
    out["train_kernels"] = TRAIN_KERNELS
if TRAIN_LINEAR is not None:
    out["train_linear"] = TRAIN_LINEAR
reference_step = make_step(m, list(m.parameters()), OPTIMIZER)
out["reference_step_ms"] = events_ms(reference_step, 20)
if TRAIN_KERNELS is not None or TRAIN_LINEAR is not None:
    out["reference_step_ms_repetitions"] = [events_ms(reference_step, 20, warm=0) for _ in range(5)]
tm = TorchEnc().to(dev).train()
pe = m.pos_encoder.pe
out["torch_rocm_nn_transformer_step_ms_context_only"] = events_ms(make_step(lambda x: tm(x, pe), list(tm.parameters())), 20)

# context only: the tests' torch port, same step on the host CPU (masks drawn on the host)
state = leaf_state({k: v.cpu() for k, v in m.state_dict().items()}, torch.float32)
copt = torch.optim.Adam([state[k] for k in param_keys(L)], lr=LR)
xc, tc = xs.cpu(), ts.cpu()


def cstep():
    masks = {"pos": (torch.rand((B, T, 24)) >= P).to(torch.uint8)}
    for l in range(L):
        masks[(l, "attn")] = (torch.rand((B, 4, T, T)) >= P).to(torch.uint8)
        for n in ("drop1", "ff", "drop2"):
            masks[(l, n)] = (torch.rand((B, T, 128)) >= P).to(torch.uint8)
    p = port_forward(xc, state, masks, P, torch.float32)
    for i, n in enumerate(lengths):
        p[i, n:, :] = 0
    loss = sum(torch.nn.functional.l1_loss(p[i, :n], tc[i, :n]) for i, n in enumerate(lengths)) / B
    copt.zero_grad()
    loss.backward()
    copt.step()


for _ in range(2):
    cstep()
t0 = time.perf_counter()
for _ in range(5):
    cstep()
out["cpu_torch_port_step_ms_context_only"] = (time.perf_counter() - t0) / 5 * 1e3
out["cpu_threads"] = torch.get_num_threads()
print(json.dumps(out))
