#!/usr/bin/env python3
"""GPU box: what `mask_padding=True` costs or saves on a captured training step.
    python tools/bench_padding_masks.py [--shape 128 40 200] [--utterances 1024] [--rounds 7] [--epochs 2] [--trace]
A seeded store of `--utterances` utterances whose lengths are uniform over [20, T] frames and [3, S] tokens (the
distribution is printed), a TextPoseTransformer (8 joints, 4 + 4 layers, dropout 0.1 from the native source) with all
three MFMA switches on, and two GraphTrainers over the same store, one with mask_padding and one without.  After a
warm-up epoch each (eager step, capture), `--rounds` rounds alternate between the two; a round times `--epochs` epochs
with a host clock around them (an epoch ends in the device-to-host copy of its losses) and divides by the steps.
Prints one JSON line: the store's distribution and per variant the median / min / max ms per step.
`--trace` runs one warm-up and one epoch of each variant and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the attention kernels' times."""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hand_pose_sl_amd as hps

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=(128, 40, 200), metavar=("B", "S", "T"))
ap.add_argument("--utterances", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--epochs", type=int, default=2)
ap.add_argument("--trace", action="store_true")
a = ap.parse_args()
B, S, T = a.shape
dev = torch.device("cuda:0")
gen = np.random.default_rng(7)
frames = gen.integers(20, T + 1, a.utterances)
ntok = gen.integers(3, S + 1, a.utterances)
tg = torch.Generator().manual_seed(8)
rows = torch.rand((int(frames.sum()), 3, 50), generator=tg) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)
tokens = torch.randint(1, 1000, (a.utterances, S), generator=tg)
for i, n in enumerate(ntok):
    tokens[i, n:] = 0
offsets = torch.tensor([0] + np.cumsum(frames).tolist(), dtype=torch.int64)
ds = hps.DeviceDataset(rows.reshape(-1, 150).contiguous(), offsets, 8, tokens)
steps = a.utterances // B


def trainer(mask):
    torch.manual_seed(0)
    m = hps.TextPoseTransformer(1000, 8, 2, 4, 128, 42, 4, 4, dropout=0.1).to(dev).set_dropout_source("native", 3)
    m.set_train_kernels("mfma").set_train_linear("mfma").set_train_whole("mfma")
    loader = hps.DeviceLoader(ds, B, T, selection="first", drop_last=True)
    return hps.GraphTrainer(m, loader, hps.Adam(m.parameters(), lr=1e-4), loss="L1", mask_padding=mask)


variants = {"mask_padding=False": trainer(False), "mask_padding=True": trainer(True)}
for t in variants.values():
    t.epoch()                                   # the eager step and the capture
torch.cuda.synchronize(dev)
if a.trace:
    for t in variants.values():
        t.epoch()
    torch.cuda.synchronize(dev)
    sys.exit(0)
ms = {k: [] for k in variants}
for _ in range(a.rounds):
    for k, t in variants.items():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(a.epochs):
            t.epoch()
        torch.cuda.synchronize(dev)
        ms[k].append((time.perf_counter() - t0) * 1e3 / (a.epochs * steps))
print(json.dumps({"shape": [B, S, T], "utterances": a.utterances, "steps_per_epoch": steps,
                  "frames": {"min": int(frames.min()), "mean": round(float(frames.mean()), 1), "max": int(frames.max())},
                  "tokens": {"min": int(ntok.min()), "mean": round(float(ntok.mean()), 1), "max": int(ntok.max())},
                  "ms_per_step": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                  for k, v in ms.items()}}))
