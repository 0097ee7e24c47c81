#!/usr/bin/env python3
"""TextPoseTransformer forward (4 + 4 layers, 1000 tokens) at (B, S, T) = (4096, 40, 100) and (64, 40, 100) through
`model(tokens, pose)`, and at (4096, 40, 200) and (64, 40, 200) -- the reference CLIs' default 200 frames -- through
`model.forward_fused` with no flags (the long-attention kernels): one JSON line with, per shape,
  hip_ms        milliseconds per forward by HIP events around `iters` back-to-back calls, after warm-up
  kernels       the per-kernel split of a `rocprofv3 --kernel-trace --stats` run of its own (a child process that
                only runs the HIP forward), as a fraction of the GPU time and microseconds per forward
  eager_ms      for context: torch-ROCm's eager nn.Transformer holding the same weights on the same GPU
  cpu16_ms      for context: the same modules on the CPU with 16 threads
The timed runs are in this process, one after the other, with no other GPU work; the profiled child runs after them.

`--precision fp32` (default) times the exact-fp32 path, `f16x3` the f16 hi + lo split path (`set_precision`), `both`
the two one after the other on the same weights and inputs: the fp32 figures stay where they are and the f16x3 ones
go under "f16x3" per shape, with its speed-up over fp32 and max|y_f16x3 - y_fp32|.  `--reps R` repeats every
timing R times: `hip_ms` is then the median and `hip_ms_reps` lists all of them.

    python tools/bench_tpt.py [--iters N] [--precision fp32|f16x3|both] [--reps R] > profiles/tpt_long/bench_tpt_long.json
"""
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hand_pose_sl_amd as hps  # noqa: E402

SHAPES = [(4096, 40, 100), (64, 40, 100), (4096, 40, 200), (64, 40, 200)]
OFF = dict(dif_encoding=False, normalize=False, denormalize=False, mask_tail=False)


def hip(model, tok, pose):
    """The HIP forward: `model(tokens, pose)` up to its 128 frames, beyond them `forward_fused` with no flags."""
    return model(tok, pose) if pose.shape[1] <= 128 else model.forward_fused(tok, pose, **OFF)


def make(dev):
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return hps.TextPoseTransformer(1000, 12, 2, 4, 128, 42, 4, 4).eval().to(dev)


def inputs(B, S, T, dev):
    g = torch.Generator().manual_seed(1)
    return torch.randint(0, 1000, (B, S), generator=g).to(dev), (torch.rand((B, T, 12, 2), generator=g) - 0.5).to(dev)


def eager(model, tok, pose):
    """The reference's forward (HandPoseModels.py:201-222) through the mirror's own torch modules."""
    B, T = pose.shape[0], pose.shape[1]
    src = model.token_embedding(tok).permute(1, 0, 2)
    tgt = model.pose2hidden_projection(pose.view(B, T, -1)).permute(1, 0, 2)
    return model.hidden2pose_projection(model.transformer(src, tgt)).permute(1, 0, 2).reshape(B, T, 21, 2)


def event_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def child(B, S, T, iters, precision="fp32"):
    dev = torch.device("cuda:0")
    model = make(dev).set_precision(precision)
    tok, pose = inputs(B, S, T, dev)
    with torch.no_grad():
        for _ in range(iters):
            hip(model, tok, pose)
    torch.cuda.synchronize()


def kernel_split(B, S, T, iters, precision="fp32"):
    tmp = tempfile.mkdtemp(prefix="bench_tpt_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "tpt", "--",
                            sys.executable, os.path.abspath(__file__), "--child", str(B), str(S), str(T), str(iters), precision],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": r.stderr[-500:]}
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            return {"error": "no kernel_stats.csv in rocprofv3's output"}
        rows = list(csv.DictReader(open(stats[0])))
        ours = [x for x in rows if "b2h" in x["Name"]]
        total = sum(float(x["TotalDurationNs"]) for x in ours)
        return {x["Name"].replace("void b2h::", ""): {"calls_per_forward": int(x["Calls"]) / iters,
                                                      "us_per_forward": round(float(x["TotalDurationNs"]) / iters / 1e3, 1),
                                                      "fraction": round(float(x["TotalDurationNs"]) / total, 4)}
                for x in sorted(ours, key=lambda x: -float(x["TotalDurationNs"]))}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        return child(*[int(v) for v in sys.argv[i + 1:i + 5]], *sys.argv[i + 5:i + 6])

    def option(name, default):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default

    iters, reps, precision = int(option("--iters", 20)), int(option("--reps", 1)), option("--precision", "fp32")
    if precision not in ("fp32", "f16x3", "both"):
        raise SystemExit("--precision is one of fp32, f16x3, both")
    first, second = ("fp32", "f16x3") if precision == "both" else (precision, None)
    dev = torch.device("cuda:0")
    model = make(dev)
    out = {"tool": "tools/bench_tpt.py", "model": "TextPoseTransformer(1000, 12, 2, 4, 128, 42, 4, 4)",
           "device": torch.cuda.get_device_name(0), "iters": iters, "precision": first, "shapes": []}

    def timed(rec):
        ms = [round(event_ms(lambda: hip(model, tok, pose), 5, iters), 4) for _ in range(reps)]
        rec["hip_ms"] = statistics.median(ms)
        if reps > 1:
            rec["hip_ms_reps"] = ms

    for B, S, T in SHAPES:
        tok, pose = inputs(B, S, T, dev)
        rec = {"B": B, "S": S, "T": T}
        with torch.no_grad():
            model.set_precision(first)
            timed(rec)
            rec["eager_ms"] = round(event_ms(lambda: eager(model, tok, pose), 3, max(3, iters // 4)), 4)
            rec["max_abs_hip_vs_eager"] = float((hip(model, tok, pose) - eager(model, tok, pose)).abs().max())
            rec["hip_frames_per_s"] = round(B * T / rec["hip_ms"] * 1e3)
            rec["speedup_vs_eager"] = round(rec["eager_ms"] / rec["hip_ms"], 2)
            if second:
                y = hip(model, tok, pose)
                model.set_precision(second)
                sub = rec[second] = {}
                timed(sub)
                sub["max_abs_vs_" + first] = float((hip(model, tok, pose) - y).abs().max())
                sub["hip_frames_per_s"] = round(B * T / sub["hip_ms"] * 1e3)
                sub["speedup_vs_" + first] = round(rec["hip_ms"] / sub["hip_ms"], 3)
        out["shapes"].append(rec)
    # context: the same modules on the CPU, 16 threads (a fresh copy: the model above stays on the GPU)
    torch.set_num_threads(16)
    cpu = make(torch.device("cpu"))
    for rec in out["shapes"]:
        tok, pose = inputs(rec["B"], rec["S"], rec["T"], torch.device("cpu"))
        with torch.no_grad():
            eager(cpu, tok[:8], pose[:8])
            t0 = time.perf_counter()
            eager(cpu, tok, pose)
            rec["cpu16_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    del model
    torch.cuda.synchronize()
    for rec in out["shapes"]:
        rec["kernels"] = kernel_split(rec["B"], rec["S"], rec["T"], 6, first)
        if second:
            rec[second]["kernels"] = kernel_split(rec["B"], rec["S"], rec["T"], 6, second)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
