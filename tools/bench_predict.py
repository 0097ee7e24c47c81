#!/usr/bin/env python3
"""GPU box: what running a trained TextPoseTransformer over a whole device-resident store costs (hps.predict_dataset:
window plan -> b2h_build_batch -> the forward -> b2h_scatter_rows per slice of the plan), and the per-joint error of the
result against the store (hps.joint_pixel_error), one JSON line.  Context only: there is no speed bar.
  * predict: wall time of predict_dataset over the store, ending in a synchronise, the median, minimum and maximum of
    `reps` repetitions after one warm-up, per precision (fp32, f16x3); frames per second = store rows / that time;
  * build, write_back: `iters` back-to-back launches of one full batch between two HIP events, ms per launch (launch
    gaps included: kernels this short are launch-bound); forward: the same for the model's forward of that batch;
  * joint_error: wall ms of joint_pixel_error(prediction, store) with its copy of the results to the host.
The store is tools/bench_loader.py's: seeded, `utterances` HDF5-style utterances (8 body joints) of T / 2 .. 3 T frames;
the model the trainer's default geometry (4 + 4 layers, (8, 42)).
    python tools/bench_predict.py [B=128] [S=40] [T=200] [reps=5] [utterances=1024] [out.json] [once]
                                  [--overlap K [--blend linear|centre]]
`once`: one predict_dataset per precision and one joint_pixel_error, nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats` for the per-kernel times.
`--overlap K` adds, per precision, an "overlap" record: predict_dataset with windows that overlap by K frames
(b2h_window_plan_overlap, b2h_scatter_rows_blend) against overlap 0, `reps` runs of each ALTERNATING in this one process
after a warm-up of both, median and range; both plan lengths and their ratio, which is what the time ratio should be
(the model's work grows with the number of windows); and write_back_blend_ms, one b2h_scatter_rows_blend launch of a full
batch timed as write_back_ms is.  With `once` the one predict_dataset per precision runs with the overlap."""
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hand_pose_sl_amd as hps  # noqa: E402

OVERLAP, BLEND = 0, "linear"
for flag in ("--overlap", "--blend"):          # the two options, wherever they stand; what is left is positional
    if flag in sys.argv:
        at = sys.argv.index(flag)
        if at + 1 >= len(sys.argv):
            sys.exit(f"{flag} needs a value")
        value = sys.argv[at + 1]
        del sys.argv[at:at + 2]
        if flag == "--overlap":
            OVERLAP = int(value)
        else:
            BLEND = value
B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
S = int(sys.argv[2]) if len(sys.argv) > 2 else 40
T = int(sys.argv[3]) if len(sys.argv) > 3 else 200
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
U = int(sys.argv[5]) if len(sys.argv) > 5 else 1024
OUT = sys.argv[6] if len(sys.argv) > 6 and sys.argv[6] != "-" else None
ONCE = len(sys.argv) > 7 and sys.argv[7] == "once"
N_TOKENS, L, N_BODY, ITERS = 1000, 4, 8, 50
if not torch.cuda.is_available():
    sys.exit("bench_predict.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")


def stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


gen = torch.Generator().manual_seed(0)
lengths = torch.randint(T // 2, 3 * T + 1, (U,), generator=gen)
offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths, 0)])
J = N_BODY + 42
rows = (torch.rand((int(offsets[-1]), 3, J), generator=gen) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)).reshape(-1, 3 * J)
ds = hps.DeviceDataset(rows, offsets, N_BODY, torch.randint(0, N_TOKENS, (U, S), generator=gen), device=dev)
loader = hps.DeviceLoader(ds, B, T, selection="first")
plan = [t.to(dev) for t in hps.window_plan(ds, T)]
out = {"B": B, "S": S, "T": T, "n_body": N_BODY, "reps": REPS, "utterances": U, "store_rows": int(offsets[-1]),
       "store_MB": rows.numel() * 4 / 1e6, "windows": plan[0].numel(), "batches": -(-plan[0].numel() // B),
       "model": {"n_enc": L, "n_dec": L, "n_tokens": N_TOKENS, "geometry": [N_BODY, 42]}}
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore", UserWarning)
    model = hps.TextPoseTransformer(N_TOKENS, N_BODY, 2, 4, 128, 42, L, L).to(dev).eval()


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def launch_ms(fn):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / ITERS)
    return stats(ms)


for precision in ("fp32", "f16x3"):
    model.set_precision(precision)
    res = {}
    if ONCE:
        pred = hps.predict_dataset(model, loader, overlap=OVERLAP, blend=BLEND)
    else:
        wall_ms(lambda: hps.predict_dataset(model, loader))          # warm-up: allocators, workspaces
        ms = stats([wall_ms(lambda: hps.predict_dataset(model, loader)) for _ in range(REPS)])
        res["predict_ms"] = ms
        res["frames_per_s_at_median"] = int(offsets[-1]) / ms["median"] * 1e3
        u, s, k = (t[:B] for t in plan)
        batch = loader.build(u, s)
        rows_out = ds.rows.clone()
        with torch.no_grad():
            y = model.forward_long(batch["text_tokens"], batch["input_kp"])
            res["build_ms"] = launch_ms(lambda: loader.build(u, s, out=batch))
            res["forward_ms"] = launch_ms(lambda: model.forward_long(batch["text_tokens"], batch["input_kp"]))
            res["write_back_ms"] = launch_ms(lambda: loader.write_back(y, u, s, k, rows_out))
        res["build_plus_write_back_over_forward"] = (res["build_ms"]["median"] + res["write_back_ms"]["median"]) / res["forward_ms"]["median"]
        if OVERLAP:
            wide = [t.to(dev) for t in hps.window_plan(ds, T, overlap=OVERLAP)]
            runs = {0: lambda: hps.predict_dataset(model, loader), OVERLAP: lambda: hps.predict_dataset(
                model, loader, overlap=OVERLAP, blend=BLEND)}
            ms = {k: [] for k in runs}
            wall_ms(runs[OVERLAP])                                       # warm-up: this plan's last batch has another size
            for _ in range(REPS):
                for k, fn in runs.items():
                    ms[k].append(wall_ms(fn))
            with torch.no_grad():
                blend_ms = launch_ms(lambda: loader.write_back_blend(y, wide, B, rows_out, y[-1], BLEND))
            res["overlap"] = {"overlap": OVERLAP, "blend": BLEND, "windows": wide[0].numel(), "windows_without": plan[0].numel(),
                              "windows_ratio": wide[0].numel() / plan[0].numel(), "predict_ms": stats(ms[OVERLAP]),
                              "predict_ms_without": stats(ms[0]),
                              "time_ratio_at_median": stats(ms[OVERLAP])["median"] / stats(ms[0])["median"],
                              "write_back_blend_ms": blend_ms}
        pred = hps.predict_dataset(model, loader, overlap=OVERLAP, blend=BLEND)
    out[precision] = res
err = hps.joint_pixel_error(pred, ds)
if not ONCE:
    out["joint_error_ms"] = stats([wall_ms(lambda: hps.joint_pixel_error(pred, ds)) for _ in range(REPS)])
out["mean_pixel_error_of_the_untrained_model"] = err.mean
line = json.dumps(out)
print(line)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")
