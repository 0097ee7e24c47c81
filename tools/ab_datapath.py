#!/usr/bin/env python3
"""GPU box: two (or more) builds of libb2h.so in ONE process on the data-path entry points, the same inputs to each
(profiles/datapath_refactor/): are the outputs equal bit for bit, and what does a call cost the host that the last
host check refuses.  One JSON line per case.
    python tools/ab_datapath.py <libA.so> <libB.so> [...] [--refused-calls N [--rounds R]]
Bits: b2h_adam_step / _guarded over 81 tensors (sizes (37 i) % 53, two raised to 257 and 1025, aligned and 4 bytes off
the 16-byte grid); b2h_step_prepare's partials and words; b2h_dropout_masks over 70 masks; b2h_build_batch, _planned and
_aug at B = 3, T = 7 (both n_body, every predict, every flag combination, an unknown and an empty utterance, a step past
the plan, every augmentation stage on and off); b2h_scatter_rows (skip given and not) and _blend at T = 7, overlap 3,
both blends, pred_before given and not.  Every output buffer is compared whole: words that must stay unwritten too.
--refused-calls: per table-driven entry point one call whose LAST operand is host memory, so every host check runs and
nothing is launched; microseconds per call, median [min, max] over interleaved rounds."""
import ctypes
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hand_pose_sl_amd import _lib

vp, i64 = ctypes.c_void_p, ctypes.c_int64
dev = torch.device("cuda:0")
rng = np.random.default_rng(7)


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SYMBOLS.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def ok(lib, rc):
    assert rc == 0, (rc, lib.b2h_last_error())


def ptr(t):
    return None if t is None else vp(t.data_ptr())


def on(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same(outs):
    """outs: per library a list of tensors; every library's against the first's, as raw bytes."""
    torch.cuda.synchronize()
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for o in outs[1:] for x, y in zip(outs[0], o))


def report(case, outs, **more):
    print(json.dumps(dict(case=case, identical=bool(same(outs)), bytes=int(sum(x.numel() * x.element_size() for x in outs[0])),
                          **more)), flush=True)


def placed(sizes, shift):
    """Start (in floats) of every tensor in one buffer, 16-byte aligned or `shift` floats past it, and the total."""
    starts, total = [], 0
    for n in sizes:
        starts.append(total + shift)
        total = (total + shift + n + 3) // 4 * 4 + 4
    return starts, total + 4


# ---- Adam, step control, dropout masks ---------------------------------------------------------------------------------
def tensor_lists(libs):
    sizes = [(37 * i) % 53 for i in range(81)]
    sizes[20], sizes[80] = 257, 1025
    n = len(sizes)
    numel = (i64 * n)(*sizes)
    for shift in (0, 1):
        starts, total = placed(sizes, shift)
        host = [rng.standard_normal(total).astype(np.float32) for _ in range(4)]
        host[3] = np.abs(host[3])
        for guarded, scale, apply in ((False, None, None), (True, None, None), (True, 0.37, 1), (True, 1.0, 1), (True, 0.37, 0)):
            outs = []
            for lib in libs:
                bufs = [on(h) for h in host]
                tabs = [(vp * n)(*[b.data_ptr() + 4 * s for s in starts]) for b in bufs]
                sw = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=dev)
                aw = None if apply is None else torch.tensor([apply], dtype=torch.int64, device=dev)
                head = (*tabs, numel, n, 2e-4, None, 0.9, 0.999, 1e-8, 1e-2, 3, None)
                ok(lib, lib.b2h_adam_step_guarded(*head, ptr(sw), ptr(aw), None) if guarded else lib.b2h_adam_step(*head, None))
                outs.append(bufs)
            report("adam_step_guarded" if guarded else "adam_step", outs, tensors=n, shift_bytes=4 * shift, scale=scale, apply=apply)
    sizes = sizes + [4096, 4097, 2 ** 20 + 5] + [(37 * i) % 53 for i in range(90)]     # 174 tensors: three launches
    n = len(sizes)
    numel = (i64 * n)(*sizes)
    for shift, max_norm in ((0, 1.0), (1, 0.05)):
        starts, total = placed(sizes, shift)
        host = rng.standard_normal(total).astype(np.float32)
        need = libs[0].b2h_step_prepare_bytes(numel, n)
        outs = []
        for lib in libs:
            assert lib.b2h_step_prepare_bytes(numel, n) == need
            g = on(host)
            words = torch.full((16,), -1, dtype=torch.int64, device=dev)      # norm, scale, apply, skipped, lr: 16 bytes apart
            ws = torch.full((need // 8 + 2,), float("nan"), dtype=torch.float64, device=dev)
            w = lambda k: vp(words.data_ptr() + 16 * k)
            ok(lib, lib.b2h_step_prepare((vp * n)(*[g.data_ptr() + 4 * s for s in starts]), numel, n, max_norm, 1, 1e-3, None, 2, 4,
                                         3, None, w(0), w(1), w(2), w(3), w(4), ptr(ws), need, None))
            outs.append([g, words, ws])
        report("step_prepare", outs, tensors=n, shift_bytes=4 * shift, partials=need // 8)
    base = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 392, 4099, 2 ** 20 + 5]                # tests/test_dropout_masks_gpu.py SIZES
    sizes = [base[i % len(base)] for i in range(70)]
    outs = []
    for lib in libs:
        masks = [torch.full((s + 32,), 7, dtype=torch.uint8, device=dev) for s in sizes]
        assert all(m.data_ptr() % 16 == 0 for m in masks)
        sw = torch.tensor([5], dtype=torch.int64, device=dev)
        ok(lib, lib.b2h_dropout_masks((vp * 70)(*[m.data_ptr() for m in masks]), (i64 * 70)(*sizes), 70, 3, 0.1, 0x1234567890AB, 2,
                                      ptr(sw), None))
        outs.append(masks)
    report("dropout_masks", outs, masks=70)


# ---- the store: build and write-back -------------------------------------------------------------------------------------
def store(n_body):
    lengths = [9, 0, 7, 16, 3, 11]                                        # an empty utterance, one of exactly T, longer ones
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = rng.standard_normal((int(offsets[-1]), 3 * (n_body + 42))).astype(np.float32) * 100
    tokens = rng.integers(0, 50, (len(lengths), 5)).astype(np.int64)
    return offsets, rows, tokens


def builds(libs):
    B, T, S = 3, 7, 5
    count = 0
    identical = True
    for n_body, predict in ((8, 0), (12, 0), (12, 1), (12, 2)):
        offsets, rows, tokens = store(n_body)
        U, N = len(offsets) - 1, rows.shape[0]
        ni, nt = {0: (n_body, 21), 1: (29, 4), 2: (21, 12)}[predict]
        d_rows, d_off, d_tok = on(rows), on(offsets), on(tokens)
        plan_utt = on(np.array([3, 1, 0, U + 3, 5, 2, 3, 4], np.int64))       # unknown: U + 3; empty: 1
        plan_start = on(np.array([4, 0, 1, 0, 2, 0, 100, -3], np.int64))
        key = on(np.array([0x9E3779B97F4A7C15, 11], np.uint64).view(np.int64))
        augs = [_lib.AugmentStruct(s, r, m, j) for s, r, m, j in itertools.product((0.0, 0.2), (0.0, 0.3), (0.0, 0.5), (0.0, 0.02))]
        for flags in range(8):
            variants = [("build_batch", None, None)] + [("planned", step, None) for step in (0, 2, 3, -1)]
            variants += [("aug", None, a) for a in augs] + [("aug_planned", 1, a) for a in augs[1::5]]
            for kind, step, aug in variants:
                outs = []
                for lib in libs:
                    o = [torch.full(s, 7, dtype=dt, device=dev) for s, dt in (((B, T, ni, 2), torch.float32), ((B, T, nt, 2), torch.float32),
                                                                             ((B, T, nt), torch.float32), ((B, S), torch.int64), ((B,), torch.int64))]
                    sw = None if step is None else torch.tensor([step], dtype=torch.int64, device=dev)
                    tail = (B, T, predict, flags, 1280.0, *[ptr(x) for x in o], None)
                    head = (ptr(d_rows), N, ptr(d_off), U, n_body, ptr(d_tok), S)
                    if kind == "build_batch":
                        rc = lib.b2h_build_batch(*head, ptr(plan_utt), ptr(plan_start), *tail)
                    elif kind == "planned":
                        rc = lib.b2h_build_batch_planned(*head, ptr(plan_utt), ptr(plan_start), 8, ptr(sw), *tail)
                    else:
                        rc = lib.b2h_build_batch_aug(*head, ptr(plan_utt), ptr(plan_start), 8, ptr(sw), 2, ctypes.byref(aug), ptr(key), *tail)
                    ok(lib, rc)
                    outs.append(o)
                count += 1
                if not same(outs):
                    identical = False
                    print(json.dumps(dict(case="build", differs=[kind, n_body, predict, flags, step])), flush=True)
    print(json.dumps(dict(case="build_batch, _planned, _aug", identical=identical, calls_per_library=count, B=B, T=T)), flush=True)


def write_backs(libs):
    T, overlap, count, identical = 7, 3, 0, True
    for n_body, predict in ((8, 0), (12, 1), (12, 2)):
        offsets, rows, _ = store(n_body)
        U, N = len(offsets) - 1, rows.shape[0]
        nt = {0: 21, 1: 4, 2: 12}[predict]
        cap = 64
        as_p = lambda a: a.ctypes.data_as(ctypes.POINTER(i64))
        d_rows, d_off = on(rows), on(offsets)
        # the plain write-back takes a plan without overlap (b2h_window_plan: one writer per row), the blend one with
        for kind_of_plan in ("plain", "blend"):
            plan = [np.zeros(cap, np.int64) for _ in range(3)]
            if kind_of_plan == "plain":
                n_plan = libs[0].b2h_window_plan(as_p(offsets), U, T, 0, as_p(plan[0]), as_p(plan[1]), as_p(plan[2]), cap)
            else:
                n_plan = libs[0].b2h_window_plan_overlap(as_p(offsets), U, T, overlap, as_p(plan[0]), as_p(plan[1]), as_p(plan[2]), cap)
            assert 0 < n_plan <= cap
            d_plan = [on(p[:n_plan]) for p in plan]
            preds = rng.standard_normal((n_plan, T, nt, 2)).astype(np.float32)
            for flags, B in itertools.product(range(4), (3, 2)):
                for entry0 in range(0, n_plan - B + 1, B):
                    pred = on(preds[entry0:entry0 + B])
                    before = on(preds[entry0 - 1]) if entry0 > 0 else None
                    if kind_of_plan == "plain":
                        calls = [("plain", None, None), ("plain without skip", None, None)]
                    else:
                        calls = [("blend", blend, b) for blend in (0, 1) for b in (before, None)]
                    for kind, blend, pb in calls:
                        outs = []
                        for lib in libs:
                            out = on(rows) + 0.5
                            head = (ptr(d_rows), N, ptr(d_off), U, n_body)
                            if kind_of_plan == "plain":
                                sl = [on(p[entry0:entry0 + B]) for p in plan]
                                # without skip the last window of an utterance rewrites rows of the one before: one batch
                                # must then not hold both, so that call takes one entry
                                Bk = B if kind == "plain" else 1
                                rc = lib.b2h_scatter_rows(*head, ptr(sl[0]), ptr(sl[1]), ptr(sl[2]) if kind == "plain" else None, Bk, T,
                                                          predict, flags, 1280.0, ptr(pred), 0.75, ptr(out), None)
                            else:
                                rc = lib.b2h_scatter_rows_blend(*head, *[ptr(p) for p in d_plan], n_plan, entry0, B, T, predict, flags,
                                                                1280.0, ptr(pred), ptr(pb), blend, 0.75, ptr(out), None)
                            ok(lib, rc)
                            outs.append([out])
                        count += 1
                        if not same(outs):
                            identical = False
                            print(json.dumps(dict(case="write_back", differs=[kind, n_body, predict, flags, B, entry0, blend, pb is not None])),
                                  flush=True)
    print(json.dumps(dict(case="scatter_rows, _blend", identical=identical, calls_per_library=count, T=T, overlap=overlap)), flush=True)


# ---- host time of a refused call -----------------------------------------------------------------------------------------
def refused(libs, paths, calls, rounds):
    B, T, S, n_body = 3, 7, 5, 12
    offsets, rows, tokens = store(n_body)
    U, N = len(offsets) - 1, rows.shape[0]
    d_rows, d_off, d_tok, d_out = on(rows), on(offsets), on(tokens), on(rows)
    utt, start = on(np.array([3, 0, 2], np.int64)), on(np.zeros(3, np.int64))
    o = [torch.zeros(s, dtype=dt, device=dev) for s, dt in (((B, T, n_body, 2), torch.float32), ((B, T, 21, 2), torch.float32),
                                                          ((B, T, 21), torch.float32), ((B, S), torch.int64))]
    pred = torch.zeros((B, T, 21, 2), device=dev)
    cells = [torch.zeros(U * 21, device=dev), torch.zeros(U * 21, dtype=torch.int32, device=dev), torch.zeros(21, dtype=torch.float64, device=dev)]
    plan = torch.zeros(U, dtype=torch.int64, device=dev)
    host = np.zeros(1 << 16, np.int64)                                    # the last operand of every call: host memory
    hp = vp(host.ctypes.data)
    entries = {
        "b2h_build_batch": lambda lib: lib.b2h_build_batch(ptr(d_rows), N, ptr(d_off), U, n_body, ptr(d_tok), S, ptr(utt), ptr(start), B, T, 0,
                                                           3, 1280.0, *[ptr(x) for x in o], hp, None),
        "b2h_scatter_rows": lambda lib: lib.b2h_scatter_rows(ptr(d_rows), N, ptr(d_off), U, n_body, ptr(utt), ptr(start), None, B, T, 0, 3,
                                                             1280.0, ptr(pred), 1.0, hp, None),
        "b2h_epoch_plan": lambda lib: lib.b2h_epoch_plan(ptr(d_off), U, T, 1, 1, 3, 1, ptr(plan), hp, None),
        "b2h_joint_error": lambda lib: lib.b2h_joint_error(ptr(d_rows), ptr(d_out), N, ptr(d_off), U, n_body, ptr(cells[0]), ptr(cells[1]),
                                                           ptr(cells[2]), hp, None),
    }
    for name, call in entries.items():
        for lib in libs:
            assert call(lib) == _lib.ERR_INVALID and b"device" in lib.b2h_last_error(), (name, lib.b2h_last_error())
        us = [[] for _ in libs]
        for _ in range(rounds):
            for k, lib in enumerate(libs):
                t0 = time.perf_counter()
                for _ in range(calls):
                    call(lib)
                us[k].append((time.perf_counter() - t0) / calls * 1e6)
        print(json.dumps(dict(case="refused " + name, calls=calls, rounds=rounds, message=libs[0].b2h_last_error().decode(),
                              us_per_call={p: [round(statistics.median(u), 3), round(min(u), 3), round(max(u), 3)]
                                           for p, u in zip(paths, us)})), flush=True)


def main():
    paths = [a for a in sys.argv[1:] if a.endswith(".so")]
    libs = [load(p) for p in paths]
    arg = lambda flag, default: int(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default
    print(json.dumps(dict(libraries=paths, device=torch.cuda.get_device_name(0))), flush=True)
    if "--refused-calls" in sys.argv:
        refused(libs, paths, arg("--refused-calls", 20000), arg("--rounds", 5))
        return
    tensor_lists(libs)
    builds(libs)
    write_backs(libs)


if __name__ == "__main__":
    main()
