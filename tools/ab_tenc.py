#!/usr/bin/env python3
"""GPU box: same-process, interleaved A/B of two or more builds of libb2h.so on the TransformerEnc path.
    python tools/ab_tenc.py <libA.so> <libB.so> [...] [precision=f16x3] [B=32768] [T=100] [max_len=100] [layers=4] [rounds=7]
T may be a comma-separated list (one model per library, every length in turn); max_len swaps in a positional table of
that many rows (the class builds the reference's 100; the handle takes up to 128); rounds=0 only compares.
Each library gets its own ctypes handle and its own model (same seed, same weights); the Python binding looks
the library up per call, so the handle is swapped in before each timed burst.  Prints median / min ms per
forward and whether the outputs equal the first library's bit for bit."""
import ctypes, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hand_pose_sl_amd as hps
from hand_pose_sl_amd import _lib

paths = [a for a in sys.argv[1:] if a.endswith(".so")]
rest = [a for a in sys.argv[1:] if not a.endswith(".so") and "=" not in a]
kw = dict(a.split("=", 1) for a in sys.argv[1:] if not a.endswith(".so") and "=" in a)
prec = rest[0] if len(rest) > 0 else "f16x3"
B = int(rest[1]) if len(rest) > 1 else 32768
Ts = [int(t) for t in rest[2].split(",")] if len(rest) > 2 else [100]
MAX_LEN, LAYERS, ROUNDS = int(kw.get("max_len", 100)), int(kw.get("layers", 4)), int(kw.get("rounds", 7))
dev = torch.device("cuda:0")


def typed(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SYMBOLS.items():
        if hasattr(lib, name):  # an older build lacks the entry points added since
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


libs = [typed(p) for p in paths]
models = []
for lib in libs:
    _lib._lib = lib
    torch.manual_seed(0)
    m = hps.TransformerEnc(24, 4, 128, 42, LAYERS, precision=prec)
    if MAX_LEN != 100:
        m.pos_encoder = hps.PositionalEncoding(24, 0.5, max_len=MAX_LEN)
    models.append(m.to(dev).eval())


@torch.no_grad()
def run(T):
    g = torch.Generator().manual_seed(T)
    x = (torch.rand((B, T, 12, 2), generator=g) - 0.5).to(dev)
    outs = []
    for lib, m in zip(libs, models):
        _lib._lib = lib
        for _ in range(3):
            y = m(x)
        torch.cuda.synchronize()
        outs.append(y.clone())
    print(f"{prec} ({B}, {T}) outputs identical to the first:", [bool(torch.equal(outs[0], o)) for o in outs[1:]],
          " max |diff|:", [float((outs[0] - o).abs().max()) for o in outs[1:]])
    times = [[] for _ in libs]
    for rnd in range(ROUNDS):
        for i, (lib, m) in enumerate(zip(libs, models)):
            _lib._lib = lib
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                m(x)
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / 10)
    for p, t in zip(paths, times if ROUNDS else []):
        print(f"{p}: median {statistics.median(t):.3f} ms  min {min(t):.3f} ms  max {max(t):.3f} ms  "
              f"({B * T / statistics.median(t) / 1e3:.1f} M frames/s)")


for T in Ts:
    run(T)
