#!/usr/bin/env python3
"""GPU box: N training steps of TransformerEnc at bench_train_tenc.py's shape (B x T = 128 x 100, 4 layers, dropout
0.1, torch.optim.Adam) and nothing else, for a `rocprofv3 --kernel-trace --stats` run per route:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \\
        python tools/train_tenc_steps.py [steps=15] [train_kernels=valu|mfma] [train_linear=valu|mfma] [B=128] [T=100]
Every step is traced, the first ones with their one-time costs included; the kernels' average times are per launch."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hand_pose_sl_amd as hps  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
KERNELS = sys.argv[2] if len(sys.argv) > 2 else "valu"
LINEAR = sys.argv[3] if len(sys.argv) > 3 else "valu"
B = int(sys.argv[4]) if len(sys.argv) > 4 else 128
T = int(sys.argv[5]) if len(sys.argv) > 5 else 100
dev = torch.device("cuda:0")
torch.manual_seed(0)
m = hps.TransformerEnc(24, 4, 128, 42, 4, dropout=0.1).to(dev).train().set_train_kernels(KERNELS).set_train_linear(LINEAR)
g = torch.Generator(device=dev).manual_seed(1)
lengths = [T - (i * 37) % (T // 2 + 1) for i in range(B)]
xs = torch.rand((B, T, 12, 2), device=dev, generator=g) - 0.5
ts = (torch.rand((B, T, 21, 2), device=dev, generator=g) - 0.5) * 0.2
crit = hps.maskedPoseL1()
opt = torch.optim.Adam(m.parameters(), lr=2e-4)
for _ in range(STEPS):
    prediction = m(xs)
    for i, n in enumerate(lengths):
        prediction[i, n:, :] = 0
    loss = crit(prediction, ts, lengths)
    opt.zero_grad()
    loss.backward()
    opt.step()
torch.cuda.synchronize()
print(f"{STEPS} steps, train_kernels={KERNELS}, train_linear={LINEAR}, B={B}, T={T}, loss {loss.item():.6f}")
