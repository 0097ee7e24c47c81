#!/usr/bin/env python3
"""GPU box: what feeding a TextPoseTransformer training step costs, from the device-resident store (DeviceLoader,
b2h_build_batch, kernel_build_batch.h) and from the host as the reference feeds it, one JSON line.
Context only: there is no speed bar; a "faster" is claimed only where the ranges of the alternating runs separate.
  * build: `iters` back-to-back b2h_build_batch launches into the same tensors between two HIP events, per launch (the
    launch gaps are in it: a kernel this short is launch-bound), the median, minimum and maximum of `reps` repetitions;
    the bytes it reads and writes, counted from the shapes;
  * host path: wall time per batch of tests/batch_ref.py -- the restatement of the reference's __getitem__ and
    transforms, held to the reference's own batches bit for bit by the tests -- run per item in this process, stacked
    and copied to the device, ending in a synchronise: what the reference's DataLoader without workers (run.py:135-136)
    and the `.to(device)` of its loop (traintest.py:89-90,106) do.  It leaves out JSON parsing and tokenising, which the
    reference also does per item: a lower bound of the reference's host work;
  * epoch: hps.train_epoch over `steps` batches of the trainer's default model (4 + 4 layers, geometry (8, 42),
    dropout 0.1, Adam lr 2e-4; MFMA attention and Linears, native dropout masks, native Adam), fed by the DeviceLoader
    and by the host path, in alternating runs; wall time of the epoch (it ends in a host synchronisation) per step.
The store is seeded: `utterances` HDF5-style utterances (8 body joints) of T / 2 .. 3 T frames, random crops.
    python tools/bench_loader.py                 B x S x T = 128 x 40 x 200, the trainer's default batch
    python tools/bench_loader.py 128 40 100      the datasets' 100 frames
    python tools/bench_loader.py [B=128] [S=40] [T=200] [reps=5] [steps=8] [out.json] [arm=feed]

The captured arm (`arm` = captured:tpt, captured:tenc or captured:conv) measures something else
with the same store: hps.train_epoch against hps.GraphTrainer.epoch() over the same loader, model and optimizer, in
alternating runs of `steps` steps after a warm-up of each (the trainer's eager first step and its capture are in the
warm-up), wall time per step; tpt is the model above, tenc TransformerEnc(24, 4, 128, 42, 4) with MFMA attention and
Linears and native masks, conv ConvModel(30), the last two on a 12-joint store.  It also times the plan of an epoch over
32 768 utterances: one b2h_epoch_plan launch (back-to-back between HIP events, and one `plan_epoch()` call to the
synchronise) against the torch-drawn plan of the same loader.  `arm` = eager:<model> runs only the eager epochs, for a
kernel trace of the eager step.  An eighth argument, `train_whole` = valu (default) or mfma, sets
TextPoseTransformer.set_train_whole in the captured and eager arms; `arm` = whole:tpt runs eager epochs under valu and
under mfma in alternating runs.

`--augment` (anywhere among the arguments; the arm and train_whole arguments are then not read) measures the augmented
build of DESIGN.md section 32 against the plain one over the same store, alternating: b2h_build_batch_aug (Augment(scale
0.2, rotate_deg 15, mirror 0.5, jitter 3)) and b2h_build_batch as `iters` back-to-back launches between HIP events, per
launch, and hps.GraphTrainer.epoch() of the model above over a loader with and one without `augment=`, wall time per
step.  It first checks that Augment() -- all four 0 -- builds the plain batch bit for bit at this shape.  Kernel times
come from running it under `rocprofv3 --kernel-trace --stats`, in a run of its own."""
import json
import os
import random
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_ref  # noqa: E402
import hand_pose_sl_amd as hps  # noqa: E402

AUGMENT = "--augment" in sys.argv
sys.argv = [a for a in sys.argv if a != "--augment"]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
S = int(sys.argv[2]) if len(sys.argv) > 2 else 40
T = int(sys.argv[3]) if len(sys.argv) > 3 else 200
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
STEPS = int(sys.argv[5]) if len(sys.argv) > 5 else 8
OUT = sys.argv[6] if len(sys.argv) > 6 and sys.argv[6] != "-" else None
ARM, _, MODEL = (sys.argv[7] if len(sys.argv) > 7 else "feed").partition(":")
WHOLE = sys.argv[8] if len(sys.argv) > 8 else "valu"
if ARM not in ("feed", "captured", "eager", "whole") or (ARM != "feed" and MODEL not in ("tpt", "tenc", "conv")):
    sys.exit("arm must be feed, captured:tpt|tenc|conv, eager:tpt|tenc|conv or whole:tpt")
if WHOLE not in ("valu", "mfma") or (ARM == "whole" and MODEL != "tpt"):
    sys.exit("train_whole must be valu or mfma; the whole arm is whole:tpt")
N_TOKENS, L, P, LR, BUILD_ITERS = 1000, 4, 0.1, 2e-4, 200
N_BODY = 12 if MODEL in ("tenc", "conv") else 8
if not torch.cuda.is_available():
    sys.exit("bench_loader.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")


def stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


# ---- the store ---------------------------------------------------------------------------------------------------------
gen = torch.Generator().manual_seed(0)
U = B * STEPS
lengths = torch.randint(T // 2, 3 * T + 1, (U,), generator=gen)
offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths, 0)])
J = N_BODY + 42
rows = (torch.rand((int(offsets[-1]), 3, J), generator=gen) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)).reshape(-1, 3 * J)
tokens = torch.randint(0, N_TOKENS, (U, S), generator=gen)
ds = hps.DeviceDataset(rows, offsets, N_BODY, tokens, device=dev)
loader = hps.DeviceLoader(ds, B, T, selection="randomcrop")
out = {"B": B, "S": S, "T": T, "n_body": N_BODY, "reps": REPS, "steps": STEPS, "utterances": U, "store_rows": int(offsets[-1]),
       "store_MB": rows.numel() * 4 / 1e6, "model": {"n_enc": L, "n_dec": L, "n_tokens": N_TOKENS, "dropout": P}}


def finish():
    line = json.dumps(out)
    print(line)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(line + "\n")


# ---- the captured arm: train_epoch against GraphTrainer.epoch(), alternating --------------------------------------------
def captured_arm():
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        if MODEL == "tpt":
            m = hps.TextPoseTransformer(N_TOKENS, N_BODY, 2, 4, 128, 42, L, L, dropout=P)
        elif MODEL == "tenc":
            m = hps.TransformerEnc(24, 4, 128, 42, L, dropout=P)
        else:
            m = hps.ConvModel(30, "ReLU", False)
    m = m.to(dev).train()
    if MODEL != "conv":
        m.set_train_kernels("mfma").set_train_linear("mfma").set_dropout_source("native", seed=0)
    if MODEL == "tpt":
        m.set_train_whole(WHOLE)
    opt = hps.Adam(m.parameters(), lr=LR)
    crit = hps.maskedPoseL1()
    trainer = hps.GraphTrainer(m, loader, opt, crit)
    out["arm"], out["model"] = ARM, {"tpt": out["model"], "tenc": {"nlayers": L, "dropout": P}, "conv": {"conv_channels": 30}}[MODEL]
    out["model"]["name"] = MODEL
    if MODEL == "tpt":
        out["model"]["train_whole"] = WHOLE

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                                  # either epoch ends in its one host synchronisation
        return (time.perf_counter() - t0) * 1e3 / STEPS

    eager = lambda: hps.train_epoch(m, loader, crit, opt)
    timed(eager)                                              # warm-up: allocators, the optimizer state
    if ARM == "eager":
        out["epoch_step_ms"] = {"what": f"wall ms per step of hps.train_epoch over {STEPS} batches",
                                "eager": stats([timed(eager) for _ in range(REPS)])}
        return finish()
    if ARM == "whole":                                        # the third switch: valu against mfma, eager epochs
        runs = {"valu": [], "mfma": []}
        timed(lambda: (m.set_train_whole("mfma"), eager()))   # warm-up of the second route
        for _ in range(REPS):
            for route in ("valu", "mfma"):
                m.set_train_whole(route)
                runs[route].append(timed(eager))
        out["model"]["train_whole"] = "valu and mfma"
        out["epoch_step_ms"] = {"what": f"wall ms per step of hps.train_epoch over {STEPS} batches, train_whole valu and mfma in "
                                        "alternating runs, same model, optimizer and loader",
                                "valu": stats(runs["valu"]), "mfma": stats(runs["mfma"]), "valu_runs": runs["valu"],
                                "mfma_runs": runs["mfma"],
                                "ranges_separate": max(runs["mfma"]) < min(runs["valu"]) or max(runs["valu"]) < min(runs["mfma"])}
        return finish()
    timed(trainer.epoch), timed(trainer.epoch)                # warm-up: the eager first step, the capture
    runs = {"eager": [], "captured": []}
    for _ in range(REPS):
        runs["eager"].append(timed(eager))
        runs["captured"].append(timed(trainer.epoch))
    out["epoch_step_ms"] = {"what": f"wall ms per step over epochs of {STEPS} steps, hps.train_epoch and hps.GraphTrainer.epoch() "
                                    "in alternating runs, same model, optimizer and loader",
                            "eager": stats(runs["eager"]), "captured": stats(runs["captured"]), "eager_runs": runs["eager"],
                            "captured_runs": runs["captured"], "captures": trainer.captures, "replays": trainer.replays,
                            "ranges_separate": max(runs["captured"]) < min(runs["eager"]) or max(runs["eager"]) < min(runs["captured"])}
    # the plan of an epoch over 32 768 utterances of 1 .. 3 frames at T = 1: native launch against the torch-drawn plan
    n = 32768
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(1, 4, (n,), generator=g)
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    big = hps.DeviceDataset(torch.zeros((int(offs[-1]), 3 * J)), offs, N_BODY, device=dev)
    plans = {}
    for source in ("native", "torch"):
        ld = hps.DeviceLoader(big, 128, 1, selection="randomcrop", shuffle=True, plan_source=source)
        ld.plan_epoch()
        plans[source + "_plan_epoch_wall_ms"] = stats([timed(lambda: (ld.plan_epoch(), torch.cuda.synchronize())) * STEPS for _ in range(max(REPS, 5))])
        if source == "native":
            ms = []
            for _ in range(REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(BUILD_ITERS):
                    ld.plan_epoch(epoch=0)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / BUILD_ITERS)
            plans["native_launch_ms"] = stats(ms)
    plans["what"] = (f"the plan of {n} utterances, shuffled with random crops: wall ms of one plan_epoch() call up to a "
                     f"synchronise, and {BUILD_ITERS} back-to-back b2h_epoch_plan calls (each with its two torch.empty) "
                     "between HIP events, ms per call")
    out["plan"] = plans
    finish()


# ---- the augmented build against the plain one, alternating --------------------------------------------------------------
def augment_arm():
    aug = hps.Augment(scale=0.2, rotate_deg=15, mirror=0.5, jitter=3)
    loaders = {"plain": loader, "augmented": hps.DeviceLoader(ds, B, T, selection="randomcrop", augment=aug)}
    out["arm"], out["augment"] = "augment", {"scale": aug.scale, "rotate_deg": aug.rotate_deg, "mirror": aug.mirror, "jitter": aug.jitter}
    utt = torch.arange(B, dtype=torch.int64, device=dev)
    start = torch.tensor([(int(lengths[u]) * 7) % (max(0, int(lengths[u]) - T) + 1) for u in range(B)], device=dev)
    want = loader.build(utt, start)
    zero = hps.DeviceLoader(ds, B, T, selection="randomcrop", augment=hps.Augment()).build(utt, start, entry0=B)
    out["zero_parameters_agree_bit_for_bit"] = all(batch_ref.same_bits(zero[k], want[k]) for k in want)
    assert out["zero_parameters_agree_bit_for_bit"]
    bufs = {k: ld.build(utt, start) for k, ld in loaders.items()}
    out["augmented_input_differs"] = not torch.equal(bufs["plain"]["input_kp"], bufs["augmented"]["input_kp"])

    def launches(name):
        ld, buf = loaders[name], bufs[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(BUILD_ITERS):
            ld.build(utt, start, out=buf)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / BUILD_ITERS

    for name in loaders:
        launches(name)                                        # warm-up of both
    runs = {"plain": [], "augmented": []}
    for _ in range(REPS):
        for name in runs:
            runs[name].append(launches(name))
    out["build"] = {"what": f"{BUILD_ITERS} back-to-back launches between HIP events, ms per launch (launch gaps included), "
                            "b2h_build_batch and b2h_build_batch_aug in alternating runs",
                    "plain": stats(runs["plain"]), "augmented": stats(runs["augmented"]), "plain_runs": runs["plain"],
                    "augmented_runs": runs["augmented"],
                    "ranges_separate": max(runs["plain"]) < min(runs["augmented"]) or max(runs["augmented"]) < min(runs["plain"])}

    trainers = {}
    for name, ld in loaders.items():
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            m = hps.TextPoseTransformer(N_TOKENS, N_BODY, 2, 4, 128, 42, L, L, dropout=P).to(dev).train()
        m.set_train_kernels("mfma").set_train_linear("mfma").set_dropout_source("native", seed=0)
        trainers[name] = hps.GraphTrainer(m, ld, hps.Adam(m.parameters(), lr=LR), hps.maskedPoseL1())

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                                  # the epoch ends in its one host synchronisation
        return (time.perf_counter() - t0) * 1e3 / STEPS

    for tr in trainers.values():
        timed(tr.epoch), timed(tr.epoch)                      # warm-up: the eager first step, the capture
    runs = {"plain": [], "augmented": []}
    for _ in range(REPS):
        for name in runs:
            runs[name].append(timed(trainers[name].epoch))
    out["epoch_step_ms"] = {"what": f"wall ms per step over hps.GraphTrainer.epoch() of {STEPS} steps, a loader without and one "
                                    "with augment= in alternating runs, twin models and optimizers",
                            "plain": stats(runs["plain"]), "augmented": stats(runs["augmented"]), "plain_runs": runs["plain"],
                            "augmented_runs": runs["augmented"], "captures": {k: t.captures for k, t in trainers.items()},
                            "ranges_separate": max(runs["plain"]) < min(runs["augmented"]) or max(runs["augmented"]) < min(runs["plain"])}
    finish()


if AUGMENT:
    augment_arm()
    sys.exit(0)
if ARM != "feed":
    captured_arm()
    sys.exit(0)


# ---- the host path -----------------------------------------------------------------------------------------------------
def host_batches():
    """The reference's loader over the same store: items in order, a random crop each (select_jsons draws
    random.randint), stacked per batch; the loop that consumes them copies them to the device."""
    for i in range(0, U, B):
        utt = range(i, min(i + B, U))
        start = [random.randint(0, max(0, int(lengths[u]) - T)) for u in utt]
        yield batch_ref.batch(rows, offsets, N_BODY, tokens, utt, start, T)


# the two paths build the same batch from the same utterances and starts (the tests hold this at small shapes)
utt0 = torch.arange(B, dtype=torch.int64)
start0 = torch.tensor([(int(lengths[u]) * 7) % (max(0, int(lengths[u]) - T) + 1) for u in range(B)])
want = batch_ref.batch(rows, offsets, N_BODY, tokens, utt0.tolist(), start0.tolist(), T)
got = loader.build(utt0, start0)
out["paths_agree_bit_for_bit"] = all(batch_ref.same_bits(got[k], want[k]) for k in want)
assert out["paths_agree_bit_for_bit"]

# ---- 1. the build launch -------------------------------------------------------------------------------------------------
dutt, dstart = utt0.to(dev), start0.to(dev)
for _ in range(20):
    loader.build(dutt, dstart, out=got)
torch.cuda.synchronize()
ms = []
for _ in range(REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(BUILD_ITERS):
        loader.build(dutt, dstart, out=got)
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1) / BUILD_ITERS)
n_frames = torch.clamp(lengths[:B], max=T)
read = int(n_frames.sum()) * (2 * N_BODY + 3 * 21) * 4 + B * S * 8 + 3 * B * 8     # the joints used of the live frames
written = B * T * (2 * N_BODY + 3 * 21) * 4 + B * S * 8 + B * 8
out["build"] = {"what": f"{BUILD_ITERS} back-to-back launches between HIP events, ms per launch", "ms": stats(ms),
                "bytes_read_needed": read, "bytes_written": written,
                "GB_per_s_at_median": (read + written) / 1e6 / stats(ms)["median"]}

# ---- 2. the host path, per batch -----------------------------------------------------------------------------------------
def host_pass_ms():
    t0, n = time.perf_counter(), 0
    for b in host_batches():
        moved = {k: v.to(dev) for k, v in b.items()}
        torch.cuda.synchronize()
        n += 1
    del moved
    return (time.perf_counter() - t0) * 1e3 / n


random.seed(0)
host_pass_ms()                                                # the first pass warms the allocators
out["host_path"] = {"what": "wall ms per batch: the restatement per item, stacked, copied to the device, synchronised",
                    "ms": stats([host_pass_ms() for _ in range(REPS)])}

# ---- 3. an epoch fed each way, alternating -------------------------------------------------------------------------------
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore", UserWarning)
    m = hps.TextPoseTransformer(N_TOKENS, N_BODY, 2, 4, 128, 42, L, L, dropout=P).to(dev).train()
m.set_train_kernels("mfma").set_train_linear("mfma").set_dropout_source("native", seed=0)
opt = hps.Adam(m.parameters(), lr=LR)
crit = hps.maskedPoseL1()


def epoch_ms(feed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hps.train_epoch(m, feed, crit, opt)                       # ends in its one host synchronisation
    return (time.perf_counter() - t0) * 1e3 / STEPS


epoch_ms(loader), epoch_ms(host_batches())                    # warm-up of both
fed = {"device": [], "host": []}
for _ in range(REPS):
    fed["device"].append(epoch_ms(loader))
    fed["host"].append(epoch_ms(host_batches()))
out["epoch_step_ms"] = {"what": f"wall ms per step of hps.train_epoch over {STEPS} batches, alternating runs",
                        "device_loader": stats(fed["device"]), "host_path": stats(fed["host"]),
                        "device_loader_runs": fed["device"], "host_path_runs": fed["host"],
                        "ranges_separate": max(fed["device"]) < min(fed["host"]) or max(fed["host"]) < min(fed["device"])}
finish()
