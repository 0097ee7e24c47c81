#!/usr/bin/env python3
"""GPU box: ConvModel training throughput (kernel_train.h), one JSON line.
  * backward (b2h_backward, recompute included) at C = 30 on a large batch, with and without dx, and its
    fraction of the fp32 FLOP bound of the issue's cost model: 10*(66C + 2C^2) + 10*(2C^2 + 42C) +
    10*(24C + 2C^2) FLOP per frame (+ 10*(2*24*C) for dx) against 157.3 TFLOP/s;
  * one full step of the reference loop body (steps/traintest.py:94-121) at 128 x 200: forward,
    mask_output, maskedPoseL1, backward, torch.optim.Adam (lr 2e-4), steady state, HIP events;
  * the same step of the oracle's torch port on the host CPU -- context only, not a baseline.
    python tools/bench_train.py [B=65536] [T=200] [optimizer=torch|native]
The third argument selects the optimizer of the reference step, torch.optim.Adam or hps.Adam,
and is recorded only when given."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hand_pose_sl_amd as hps  # noqa: E402

PEAK = 157.3e12
C = 30
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
T = int(sys.argv[2]) if len(sys.argv) > 2 else 200
OPTIMIZER = sys.argv[3] if len(sys.argv) > 3 else None    # absent: torch.optim.Adam, and no key in the record
if OPTIMIZER not in (None, "torch", "native"):
    sys.exit(f"optimizer must be torch or native, got {OPTIMIZER!r}")
dev = torch.device("cuda:0")


def events_ms(fn, iters, warm=3):
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


def flop_per_frame(dx):
    f = 10 * (66 * C + 2 * C * C) + 10 * (2 * C * C + 42 * C) + 10 * (24 * C + 2 * C * C)
    return f + (10 * 2 * 24 * C if dx else 0)


torch.manual_seed(0)
m = hps.ConvModel(C, "ReLU", False).to(dev).train()
lib, _ = m._ensure_created()
import ctypes  # noqa: E402
vp = ctypes.c_void_p
g = torch.Generator(device=dev).manual_seed(1)
x = torch.rand((B, T, 12, 2), device=dev, generator=g) - 0.5
dy = torch.randn((B, T, 21, 2), device=dev, generator=g)
y = torch.empty((B, T, 21, 2), device=dev)
dx = torch.empty_like(x)
params = list(m._params())
grads = [torch.empty_like(p) for p in params]
pa = (vp * 8)(*[p.data_ptr() for p in params])
ga = (vp * 8)(*[q.data_ptr() for q in grads])
nbytes = lib.b2h_backward_workspace_bytes(m._handle, B, T)
ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def st():
    return vp(torch.cuda.current_stream(dev).cuda_stream)


def fwd():
    assert lib.b2h_train_forward(m._handle, pa, vp(x.data_ptr()), vp(y.data_ptr()), B, T, st()) == 0


def bwd(with_dx):
    def f():
        assert lib.b2h_backward(m._handle, pa, vp(x.data_ptr()), vp(dy.data_ptr()), vp(dx.data_ptr()) if with_dx else None,
                                ga, B, T, vp(ws.data_ptr()), nbytes, st()) == 0
    return f


out = {"C": C, "B": B, "T": T, "workspace_MiB": nbytes / 2**20, "peak_fp32_TFLOPs": PEAK / 1e12}
ms = events_ms(fwd, 5)
out["train_forward"] = {"ms": ms, "G_frames_per_s": B * T / ms / 1e6,
                        "frac_of_flop_bound": B * T * 10 * (66 * C + 2 * C * C) / (ms * 1e-3) / PEAK}
for with_dx in (False, True):
    ms = events_ms(bwd(with_dx), 5)
    out["backward_dx" if with_dx else "backward"] = {
        "ms": ms, "G_frames_per_s": B * T / ms / 1e6,
        "flop_bound_G_frames_per_s": PEAK / flop_per_frame(with_dx) / 1e9,
        "frac_of_flop_bound": B * T * flop_per_frame(with_dx) / (ms * 1e-3) / PEAK}
del x, dy, y, dx, ws
torch.cuda.empty_cache()

# one reference step at 128 x 200 (run.py:43-44: batch 128, lr 2e-4)
SB, ST = 128, 200
lengths = [ST - (i * 37) % 120 for i in range(SB)]
xs = torch.rand((SB, ST, 12, 2), device=dev, generator=g) - 0.5
ts = (torch.rand((SB, ST, 21, 2), device=dev, generator=g) - 0.5) * 0.2
opt = (hps.Adam if OPTIMIZER == "native" else torch.optim.Adam)(m.parameters(), lr=2e-4)
crit = hps.maskedPoseL1()


def step():
    prediction = m(xs)
    for i, n in enumerate(lengths):
        prediction[i, n:, :] = 0
    loss = crit(prediction, ts, lengths)
    opt.zero_grad()
    loss.backward()
    opt.step()


if OPTIMIZER is not None:
    out["optimizer"] = OPTIMIZER
out["reference_step_128x200_ms"] = events_ms(step, 20, warm=5)

# context only: the oracle's torch port, same step on the host CPU
from oracle.torch_port import torch_forward  # noqa: E402
state = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
copt = torch.optim.Adam(list(state.values()), lr=2e-4)
xc, tc = xs.cpu(), ts.cpu()


def cstep():
    p = torch_forward(xc, state)
    for i, n in enumerate(lengths):
        p[i, n:, :] = 0
    loss = sum(torch.nn.functional.l1_loss(p[i, :n], tc[i, :n]) for i, n in enumerate(lengths)) / SB
    copt.zero_grad()
    loss.backward()
    copt.step()


for _ in range(2):
    cstep()
t0 = time.perf_counter()
for _ in range(5):
    cstep()
out["cpu_torch_port_step_128x200_ms_context_only"] = (time.perf_counter() - t0) / 5 * 1e3
out["cpu_threads"] = torch.get_num_threads()
print(json.dumps(out))
