#!/usr/bin/env python3
"""GPU box: what gradient clipping, the non-finite guard and warmup cost a TextPoseTransformer training step
(profiles/adam_step_control/), one JSON line.  The step is bench_train_tpt.py's (4 + 4 layers,
n_tokens = 1000, dropout 0.1 drawn natively, the mfma train kernels and Linears, maskedPoseL1, lr 2e-4) with three
routes between backward and the update:
    a   hand_pose_sl_amd.Adam                                       nothing: the step as it was
    b   torch.nn.utils.clip_grad_norm_(parameters, 1.0), then a     torch's clipping in front of the native update
    c   hand_pose_sl_amd.Adam(max_grad_norm=1.0, skip_nonfinite=True, warmup_steps=1000)
Each route has a model of its own from the same seed.  `rounds` rounds, each timing `steps` steps of a, b and c in turn
between HIP events after a warm-up of each; per route the median, minimum and maximum over the rounds, every round listed,
and whether the ranges separate.

    python tools/bench_step_control.py [B=128] [S=40] [T=200] [n_joints=8] [rounds=7] [steps=20]
    python tools/bench_step_control.py B S T n_joints profile:b|profile:c [steps=100]

`profile:b` makes one backward and then only `steps` calls of clip_grad_norm_; `profile:c` makes one backward and then
`steps` steps of route c's optimizer and `steps` of route a's on the same gradients: nothing else, to run under
`rocprofv3 --kernel-trace --stats`, once per route.  The kernels whose call count is a multiple of `steps` are the
clip work (b), and b2h_grad_sumsq_k, b2h_step_control_k, b2h_adam_guarded_k beside b2h_adam_step_k (c)."""
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hand_pose_sl_amd as hps  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
S = int(sys.argv[2]) if len(sys.argv) > 2 else 40
T = int(sys.argv[3]) if len(sys.argv) > 3 else 200
J = int(sys.argv[4]) if len(sys.argv) > 4 else 8
PROFILE = sys.argv[5].split(":", 1)[1] if len(sys.argv) > 5 and sys.argv[5].startswith("profile:") else None
ROUNDS = 1 if PROFILE else (int(sys.argv[5]) if len(sys.argv) > 5 else 7)
STEPS = int(sys.argv[6]) if len(sys.argv) > 6 else (100 if PROFILE else 20)
if PROFILE not in (None, "b", "c"):
    sys.exit(f"profile:b or profile:c, got {sys.argv[5]!r}")
N_TOKENS, L, P, LR = 1000, 4, 0.1, 2e-4
CONTROL = dict(max_grad_norm=1.0, skip_nonfinite=True, warmup_steps=1000)
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
lengths = [T - (i * 37) % (T // 2 + 1) for i in range(B)]
toks = torch.randint(0, N_TOKENS, (B, S), device=dev, generator=g)
xs = torch.rand((B, T, J, 2), device=dev, generator=g) - 0.5
ts = (torch.rand((B, T, 21, 2), device=dev, generator=g) - 0.5) * 0.2
crit = hps.maskedPoseL1()


def make(route):
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        m = hps.TextPoseTransformer(N_TOKENS, J, 2, 4, 128, 42, L, L, dropout=P).to(dev).train()
    m.set_train_kernels("mfma").set_train_linear("mfma").set_dropout_source("native", seed=0)
    params = list(m.parameters())
    opt = hps.Adam(params, lr=LR, **(CONTROL if route == "c" else {}))

    def backward():
        prediction = m(toks, xs)
        for i, n in enumerate(lengths):
            prediction[i, n:, :] = 0
        loss = crit(prediction, ts, lengths)
        opt.zero_grad()
        loss.backward()

    def step():
        backward()
        if route == "b":
            torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
    return step, backward, opt, params


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / STEPS


if PROFILE == "b":
    _, backward, _, params = make("b")
    backward()
    for _ in range(STEPS):
        torch.nn.utils.clip_grad_norm_(params, 1.0)
    torch.cuda.synchronize()
    print(json.dumps({"profile": "b", "steps": STEPS, "tensors": len(params)}))
    sys.exit(0)
if PROFILE == "c":
    _, backward, opt, params = make("c")
    plain = hps.Adam(params, lr=LR)
    backward()
    for _ in range(STEPS):
        opt.step()
    for _ in range(STEPS):
        plain.step()
    torch.cuda.synchronize()
    print(json.dumps({"profile": "c", "steps": STEPS, "tensors": len(params), "skipped": opt.skipped_steps(),
                      "grad_norm": opt.grad_norm.item()}))
    sys.exit(0)

routes = {r: make(r) for r in "abc"}
for step, _, _, _ in routes.values():
    for _ in range(5):
        step()
torch.cuda.synchronize()
runs = {r: [] for r in routes}
for _ in range(ROUNDS):
    for r, (step, _, _, _) in routes.items():
        runs[r].append(round(timed(step), 4))
out = {"B": B, "S": S, "T": T, "n_joints": J, "n_enc": L, "n_dec": L, "dropout": P, "kernels": "mfma", "linear": "mfma",
       "dropout_source": "native", "rounds": ROUNDS, "steps_per_round": STEPS, "control": CONTROL,
       "routes": {"a": "hps.Adam", "b": "clip_grad_norm_ + hps.Adam", "c": "hps.Adam with max_grad_norm, skip_nonfinite, warmup"}}
for r, ms in runs.items():
    s = sorted(ms)
    out[r] = {"step_ms_median": s[len(s) // 2], "step_ms_min": s[0], "step_ms_max": s[-1], "step_ms_runs": ms}
for x, y in (("a", "c"), ("b", "c"), ("a", "b")):
    out[f"ranges_separate_{x}_{y}"] = out[x]["step_ms_max"] < out[y]["step_ms_min"] or out[y]["step_ms_max"] < out[x]["step_ms_min"]
c_opt = routes["c"][2]
out["c_skipped_steps"], out["c_current_lr"], out["c_grad_norm"] = c_opt.skipped_steps(), c_opt.current_lr(), c_opt.grad_norm.item()
print(json.dumps(out))
