#!/usr/bin/env python3
"""GPU box: the TextPoseTransformer forward (4 + 4 layers, 1000 tokens) in the four geometries the reference's CLIs
build, at (B, S, T) = (4096, 40, 200) and (64, 40, 200) in both arithmetics, through `forward_long` (rows already
built): median ms per forward by HIP events over 5 bursts, one after the other in one process.  One JSON line.
    python tools/bench_tpt_geom.py > profiles/tpt_geom/bench_tpt_geom.json"""
import json, os, statistics, sys, warnings
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hand_pose_sl_amd as hps

dev = torch.device("cuda:0")
out = {}
for n_joints, nout in ((12, 42), (8, 42), (29, 8), (21, 24)):
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        m = hps.TextPoseTransformer(1000, n_joints, 2, 4, 128, nout, 4, 4).eval().to(dev)
    for B, S, T in ((4096, 40, 200), (64, 40, 200)):
        g = torch.Generator().manual_seed(1)
        tok = torch.randint(0, 1000, (B, S), generator=g).to(dev)
        pose = (torch.rand((B, T, n_joints, 2), generator=g) - 0.5).to(dev)
        iters = 10 if B >= 1024 else 50
        for prec in ("fp32", "f16x3"):
            m.set_precision(prec)
            with torch.no_grad():
                for _ in range(3):
                    m.forward_long(tok, pose)
                ts = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        m.forward_long(tok, pose)
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) / iters)
            out[f"j{n_joints}_o{nout} ({B}, {S}, {T}) {prec}"] = round(statistics.median(ts), 4)
print(json.dumps(out))
