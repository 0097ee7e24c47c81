#!/usr/bin/env python3
"""GPU box: same-process, interleaved A/B of two or more builds of libb2h.so on one training step (train-forward +
backward) of TransformerEnc or TextPoseTransformer through the C ABI, after tools/ab_lib.py and tools/ab_tpt.py.
    python tools/ab_train.py <libA.so> <libB.so> [...] --model tpt --shape 128 40 200 --layers 4 --p 0.1 \
        [--attn valu|mfma] [--linear valu|mfma] [--whole valu|mfma] [--geometry 8 42] [--rounds 7] [--iters 10] [--host-calls 0] \
        [--refused-calls 0] [--max-len 100]
Each library is loaded under its own ctypes handle (only the symbols it has are typed) and gets its own model handle;
all of them run on the same inputs, parameters, masks and the same output, saved and scratch buffers.  Naming the same
file twice (or a copy of it) gives the spread of a build against itself, which a difference between two builds has to
exceed.  Prints one JSON line: per library whether y, dx and every gradient equal the first library's bit for bit, the
ms per step over interleaved rounds (HIP events around `--iters` back-to-back steps), and with `--host-calls N` the
host's microseconds per step over N steps enqueued without a synchronisation in between (at small shapes the queue
paces these, not the host).  `--refused-calls N` times the host checks alone: N train-forward + backward pairs that
are refused by the last check before the launches (y laid over the saved buffer, dx over the scratch: "two outputs
overlap", found after every other comparison) and launch nothing.  `--rounds 0` runs each library once and only
compares (a run to trace)."""
import argparse, ctypes, json, os, statistics, sys, time, warnings
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hand_pose_sl_amd as hps
from hand_pose_sl_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--model", choices=("tenc", "tpt"), default="tpt")
ap.add_argument("--shape", type=int, nargs="+", default=None, help="B T (tenc) or B S T (tpt)")
ap.add_argument("--layers", type=int, default=4, help="encoder layers; a tpt model gets as many decoder layers")
ap.add_argument("--p", type=float, default=0.1)
ap.add_argument("--attn", choices=sorted(_lib.TRAIN_KERNELS), default="valu")
ap.add_argument("--linear", choices=sorted(_lib.TRAIN_KERNELS), default="valu")
ap.add_argument("--whole", choices=sorted(_lib.TRAIN_KERNELS), default="valu", help="tpt only: b2h_tpt_set_train_whole")
ap.add_argument("--geometry", type=int, nargs=2, default=(8, 42), metavar=("N_JOINTS", "NOUT"), help="tpt only")
ap.add_argument("--max-len", type=int, default=100, help="tenc only: rows of the positional table (T <= max_len)")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--host-calls", type=int, default=0)
ap.add_argument("--refused-calls", type=int, default=0)
a = ap.parse_args()
tpt = a.model == "tpt"
dims = tuple(a.shape or ((128, 40, 200) if tpt else (128, 100)))
assert len(dims) == (3 if tpt else 2), "--shape takes B S T for tpt, B T for tenc"
B, T = dims[0], dims[-1]
dev = torch.device("cuda:0")
vp = ctypes.c_void_p


def ptr(t):
    return vp(t.data_ptr())


def ptrs(ts):
    return (vp * len(ts))(*[t.data_ptr() for t in ts])


# one seeded model on the host supplies the parameters and the mask order; the handles come from each library
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore", UserWarning)
    if tpt:
        model = hps.TextPoseTransformer(1000, a.geometry[0], 2, 4, 128, a.geometry[1], a.layers, a.layers, dropout=a.p)
        create, ninp, nout = "b2h_tpt_create", model.ninp, model.nout
    else:
        model = hps.TransformerEnc(24, 4, 128, 42, a.layers, dropout=a.p)
        if a.max_len != 100:  # the class builds the reference's table of 100 rows; the handle takes any length
            model.pos_encoder = type(model.pos_encoder)(24, a.p, max_len=a.max_len)
        create, ninp, nout = "b2h_tenc_create", 24, 42
tensors = [t.detach().to(dev).contiguous() for t in model._tensors()]
g = torch.Generator().manual_seed(1)
x = (torch.rand((B, T, ninp), generator=g) - 0.5).to(dev)
dy = (torch.rand((B, T, nout), generator=g) - 0.5).to(dev)
tok = torch.randint(0, 1000, (B, dims[1]), generator=g).to(dev) if tpt else None
masks = [(torch.rand(shape, generator=g) >= a.p).to(torch.uint8).to(dev) for _, shape in model._mask_order(*dims)] if a.p > 0 else []
grads = [torch.empty_like(t) for t in (tensors if tpt else tensors[1:])]
y, dx = torch.empty((B, T, nout), device=dev), torch.empty((B, T, ninp), device=dev)

libs = []
for path in a.libs:
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    h = vp()
    assert getattr(lib, create)(*model._create_args(), ctypes.byref(h)) == 0, lib.b2h_last_error()
    if tpt:
        assert lib.b2h_tpt_set_train_kernel(h, _lib.TRAIN_KERNELS[a.attn]) == 0, lib.b2h_last_error()
        assert lib.b2h_tpt_set_train_linear(h, _lib.TRAIN_KERNELS[a.linear]) == 0, lib.b2h_last_error()
        if a.whole != "valu":   # (a library older than the switch keeps its only route)
            assert lib.b2h_tpt_set_train_whole(h, _lib.TRAIN_KERNELS[a.whole]) == 0, lib.b2h_last_error()
    libs.append((lib, h))
nbytes = getattr(libs[0][0], f"b2h_{a.model}_train_bytes")
nsaved, nscratch = nbytes(libs[0][1], *dims, 0), nbytes(libs[0][1], *dims, 1)
saved = torch.empty(nsaved, dtype=torch.uint8, device=dev)
scratch = torch.empty(nscratch, dtype=torch.uint8, device=dev)
head = (ptrs(tensors), ptr(tok)) if tpt else (ptrs(tensors),)
pm, pg = (ptrs(masks) if masks else None), ptrs(grads)


def step(lib, h):
    rc = getattr(lib, f"b2h_{a.model}_train_forward")(h, *head, ptr(x), pm, a.p, ptr(y), ptr(saved), nsaved, *dims, None)
    rc = rc or getattr(lib, f"b2h_{a.model}_backward")(h, *head, pm, a.p, ptr(dy), ptr(saved), nsaved, ptr(dx), pg,
                                                       ptr(scratch), nscratch, *dims, None)
    assert rc == 0, lib.b2h_last_error()


outputs = [y, dx] + grads
same, ref = [], None
for lib, h in libs:
    for t in outputs:
        t.fill_(float("nan"))
    step(lib, h)
    torch.cuda.synchronize()
    if ref is None:
        ref = [t.clone() for t in outputs]
    # bit patterns, so that a NaN compares equal to the same NaN
    same.append(all(torch.equal(r.view(torch.int32), t.view(torch.int32)) for r, t in zip(ref, outputs)))

ms = [[] for _ in libs]
for _ in range(a.rounds):
    for i, (lib, h) in enumerate(libs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            step(lib, h)
        e1.record()
        torch.cuda.synchronize()
        ms[i].append(e0.elapsed_time(e1) / a.iters)
host_us = [[] for _ in libs]
for _ in range(a.rounds if a.host_calls else 0):
    for i, (lib, h) in enumerate(libs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.host_calls):
            step(lib, h)
        host_us[i].append((time.perf_counter() - t0) / a.host_calls * 1e6)
        torch.cuda.synchronize()


def refused(lib, h):
    rc = getattr(lib, f"b2h_{a.model}_train_forward")(h, *head, ptr(x), pm, a.p, ptr(saved), ptr(saved), nsaved, *dims, None)
    rb = getattr(lib, f"b2h_{a.model}_backward")(h, *head, pm, a.p, ptr(dy), ptr(saved), nsaved, ptr(scratch), pg,
                                                 ptr(scratch), nscratch, *dims, None)
    return rc, rb


refused_us = [[] for _ in libs]
for _ in range(a.rounds if a.refused_calls else 0):
    for i, (lib, h) in enumerate(libs):
        assert refused(lib, h) == (_lib.ERR_INVALID, _lib.ERR_INVALID) and lib.b2h_last_error() == b"two outputs overlap"
        t0 = time.perf_counter()
        for _ in range(a.refused_calls):
            refused(lib, h)
        refused_us[i].append((time.perf_counter() - t0) / a.refused_calls * 1e6)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} if v else None


print(json.dumps({"model": a.model, "shape": dims, "layers": a.layers, "p": a.p, "attn": a.attn if tpt else None,
                  "linear": a.linear if tpt else None, "geometry": list(a.geometry) if tpt else None, "iters": a.iters,
                  "rounds": a.rounds, "host_calls": a.host_calls, "refused_calls": a.refused_calls,
                  "libs": [{"path": p, "identical_to_first": s, "ms_per_step": spread(m), "host_us_per_step": spread(u),
                            "refused_us_per_pair": spread(r)}
                           for p, s, m, u, r in zip(a.libs, same, ms, host_us, refused_us)]}))
