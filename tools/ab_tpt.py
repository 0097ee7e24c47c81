#!/usr/bin/env python3
"""GPU box: same-process, interleaved A/B of two or more builds of libb2h.so on the TextPoseTransformer forward (the
default geometry, 4 + 4 layers, 1000 tokens), after tools/ab_tenc.py.
    python tools/ab_tpt.py <libA.so> <libB.so> [...] [precision=fp32] [B=4096] [S=40] [T=200] [shapes=BxSxT,...] [rounds=7]
shapes= runs a list of shapes in one process (one model per library); rounds=0 only compares.
Each library gets its own ctypes handle and its own model (same seed, same weights); the handle is swapped in before
each timed burst.  Naming the same file twice (or a copy of it) gives the spread of a build against itself, which is
what a difference between two builds has to exceed.  Prints median / min ms per forward and whether the outputs equal
the first library's bit for bit.  An older library that lacks entry points of today's binding is typed as far as it
goes."""
import ctypes, os, statistics, sys, warnings
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hand_pose_sl_amd as hps
from hand_pose_sl_amd import _lib

paths = [a for a in sys.argv[1:] if a.endswith(".so")]
rest = [a for a in sys.argv[1:] if not a.endswith(".so") and "=" not in a]
kw = dict(a.split("=", 1) for a in sys.argv[1:] if not a.endswith(".so") and "=" in a)
prec = rest[0] if len(rest) > 0 else "fp32"
SHAPES = [tuple(int(rest[i]) if len(rest) > i else d for i, d in ((1, 4096), (2, 40), (3, 200)))]
if "shapes" in kw:
    SHAPES = [tuple(int(v) for v in sh.split("x")) for sh in kw["shapes"].split(",")]
ROUNDS = int(kw.get("rounds", 7))
dev = torch.device("cuda:0")
OFF = dict(dif_encoding=False, normalize=False, denormalize=False, mask_tail=False)


def typed(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def run(m, tok, pose):
    return m(tok, pose) if pose.shape[1] <= 128 else m.forward_fused(tok, pose, **OFF)


libs = [typed(p) for p in paths]
models = []
for lib in libs:
    _lib._lib = lib
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        models.append(hps.TextPoseTransformer(1000, 12, 2, 4, 128, 42, 4, 4).eval().to(dev).set_precision(prec))


@torch.no_grad()
def ab(B, S, T):
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, 1000, (B, S), generator=g).to(dev)
    pose = (torch.rand((B, T, 12, 2), generator=g) - 0.5).to(dev)
    iters = 10 if B >= 1024 else 50
    outs = []
    for lib, m in zip(libs, models):
        _lib._lib = lib
        for _ in range(3):
            y = run(m, tok, pose)
        torch.cuda.synchronize()
        outs.append(y.clone())
    print(f"{prec} ({B}, {S}, {T}) outputs identical to the first:", [bool(torch.equal(outs[0], o)) for o in outs[1:]],
          " max |diff|:", [float((outs[0] - o).abs().max()) for o in outs[1:]])
    times = [[] for _ in libs]
    for rnd in range(ROUNDS):
        for i, (lib, m) in enumerate(zip(libs, models)):
            _lib._lib = lib
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run(m, tok, pose)
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / iters)
    for p, t in zip(paths, times if ROUNDS else []):
        print(f"{p}: median {statistics.median(t):.4f} ms  min {min(t):.4f} ms  max {max(t):.4f} ms")


for shape in SHAPES:
    ab(*shape)
