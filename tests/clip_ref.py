"""numpy restatements of b2h_step_prepare and b2h_adam_step_guarded (include/b2h.h, kernel_step_control.h,
kernel_adam.h), and the float64 truths their tests share.  A helper module, not a conftest.py: the tests import it by
name.

    partials(grads)           the fp64 partial sums of squares in the kernel's own order: the flat index over 16-byte
                              chunks, blocks of 1024 chunks, thread j of 256 on chunks j, j + 256, j + 512, j + 768, the
                              wave butterfly, the four waves in order; a block shared by two 80-tensor launches is the
                              earlier launch's sum plus the later one's.  fma(x, x, acc) in double is x * x + acc rounded
                              once, and x * x is exact for a float x, so numpy's multiply and add restate it bit for bit.
    total(partials)           the control kernel's sum: thread j adds partial[j], partial[j + 256], ... then the same tree
    control(...)              the words of b2h_step_prepare from that total, line by line in float64
    truth_norm(grads)         sqrt of the exactly rounded sum (math.fsum) of the float64 squares
    truth_scale / truth_lr    torch's clamped clip_coef and the schedules in float64
    clipped(...)              adam_ref.restate32 / adam_ref.truth on the gradient times the coefficient
"""
import math

import numpy as np

import adam_ref

f32, f64 = np.float32, np.float64
CHUNK, BLOCK, THREADS, LAUNCH = 4, 1024, 256, 80
NONE, LINEAR, INV_SQRT = 0, 1, 2


def _tree(per_thread):
    """(..., 256) float64 -> (...): butterfly inside each wave of 64, then ((w0 + w1) + w2) + w3."""
    v = per_thread.reshape(per_thread.shape[:-1] + (4, 64)).copy()
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ off]
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def partials(grads):
    grads = [np.asarray(g, f32).reshape(-1) for g in grads]
    chunks = [(g.size + CHUNK - 1) // CHUNK for g in grads]
    n_blocks = (sum(chunks) + BLOCK - 1) // BLOCK
    out = np.zeros(n_blocks, f64)
    stored = np.zeros(n_blocks, bool)
    at = 0
    for base in range(0, len(grads), LAUNCH):
        sq = np.zeros((n_blocks * BLOCK, CHUNK), f64)     # a chunk of another launch adds nothing: acc + 0.0 is acc
        lo = at
        for g, c in zip(grads[base:base + LAUNCH], chunks[base:base + LAUNCH]):
            x = np.zeros(c * CHUNK, f64)
            x[:g.size] = g.astype(f64)
            sq[at:at + c] = (x * x).reshape(c, CHUNK)
            at += c
        if at == lo:
            continue
        sq = sq.reshape(n_blocks, BLOCK // THREADS, THREADS, CHUNK)
        acc = np.zeros((n_blocks, THREADS), f64)
        for k in range(BLOCK // THREADS):
            for e in range(CHUNK):
                acc = acc + sq[:, k, :, e]
        s = _tree(acc)
        for b in range(lo // BLOCK, (at - 1) // BLOCK + 1):
            out[b] = out[b] + s[b] if stored[b] else s[b]
            stored[b] = True
    return out


def total(part):
    part = np.asarray(part, f64)
    acc = np.zeros(THREADS, f64)
    for j0 in range(0, part.size, THREADS):
        row = part[j0:j0 + THREADS]
        acc[:row.size] = acc[:row.size] + row
    return float(_tree(acc))


def factor(schedule, W, t):
    if schedule == LINEAR:
        return 1.0 if t >= W else t / W
    if schedule == INV_SQRT:
        return t / W if t <= W else math.sqrt(W / t)
    return 1.0


def control(tot, max_norm, guard, base_lr, schedule, W, t):
    """(norm, scale, apply, lr): float32, float32, int, float32 as b2h_step_control_k stores them."""
    with np.errstate(invalid="ignore", over="ignore"):
        norm = math.sqrt(tot) if tot >= 0 else float("nan")
        apply = int(math.isfinite(tot)) if guard else 1
        scale = f32(1.0)
        if max_norm > 0:
            c = float(f32(max_norm)) / (norm + 1e-6)
            scale = f32(1.0 if c >= 1.0 else c)
        if not apply:
            scale = f32(0.0)
        return f32(norm), scale, apply, f32(float(f32(base_lr)) * factor(schedule, W, t))


def truth_norm(grads):
    return math.sqrt(math.fsum(math.fsum((np.asarray(g, f64).reshape(-1) ** 2).tolist()) for g in grads))


def truth_scale(norm, max_norm):
    c = float(f32(max_norm)) / (norm + 1e-6)
    return min(c, 1.0)


def truth_lr(base_lr, schedule, W, t):
    return float(f32(base_lr)) * factor(schedule, W, t)


def within_one_ulp(got, want64):
    """|got - float32(want64)| is at most the float32 spacing there."""
    want = f32(want64)
    return bool(abs(float(got) - float(want)) <= float(np.spacing(np.abs(want))))


def clipped(fn, p, g, m, v, t, lr, wd, coef):
    """fn = adam_ref.restate32: the guarded kernel's listing, the product g * coef rounded to float32 first;
    fn = adam_ref.truth: the same update with nothing rounded."""
    if fn is adam_ref.restate32:
        g = np.asarray(g, f32) * f32(coef)
    else:
        g = np.asarray(g, f64) * float(coef)
    return fn(p, g, m, v, t, lr, wd=wd)
