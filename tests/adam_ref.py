"""numpy restatements of b2h_adam_step (include/b2h.h, kernel_adam.h), the inputs of its accuracy tests and the
measure they share.  A helper module, not a conftest.py: the tests import it by name.

    truth(...)      torch.optim.Adam's update (amsgrad = False, maximize = False, L2 weight decay) in float64, the
                    hyper-parameters the Python doubles torch gets
    restate32(...)  the kernel's listing line by line in float32: every line one rounding, the fused multiply-adds
                    through a float64 product and sum (exact product, then two roundings instead of one: they differ
                    from a true FMA in about one element in 2^29)
    ulp_error(...)  max |got - truth| in units of the float32 spacing at the truth's value

The bar of the issue: the error of the native update against the truth is at most 2 x the largest error of
torch.optim.Adam(foreach=False) in fp32 over all the cases below + 1 ulp, per quantity (p, m, v).  The cases keep torch's
own error bounded: p stays away from zero (|p| >= 0.5, the update is at most a few lr), exp_avg has the sign of the
gradient it meets and, under weight decay, the gradient the sign of p, so no line cancels to much less than its operands
and the maximum over millions of elements is not the luck of one cancellation (with free signs torch's own exp_avg was
off by 38 882 ulp in one element of 17 million on the CPU)."""
import numpy as np

f32, f64 = np.float32, np.float64
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 2 ** 20 + 5]
STEPS = [1, 2, 1000, 10 ** 6]
SCALES = [-6, -3, 0, 3]                                   # gradients N(0, 1) * 10^k
SETTINGS = [(0.0, 2e-4), (1e-2, 2e-4), (0.0, 1e-3), (1e-2, 1e-3)]      # (weight_decay, lr)
B1, B2, EPS = 0.9, 0.999, 1e-8


def cases():
    """(t, k, weight_decay, lr): every step with every gradient scale; the four settings go round so that each meets
    every step and every scale once."""
    return [(t, k, *SETTINGS[(i + j) % 4]) for i, t in enumerate(STEPS) for j, k in enumerate(SCALES)]


def pow_sq(b, t):
    """b^t by squaring, as ad_pow of kernel_adam.h."""
    r, t = 1.0, int(t)
    while t > 0:
        if t & 1:
            r *= b
        b *= b
        t >>= 1
    return r


def inputs(n, t, k, wd, seed):
    """p, g, m, v (float32, n elements) for an update at step t: g = N(0, 1) * 10^k with exact zeros in a tenth of the
    elements; m = v = 0 at t = 1, else a state consistent with t - 1 steps of such gradients, v > 0."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** k
    g = (rng.standard_normal(n) * scale).astype(f32)
    g[rng.random(n) < 0.1] = 0
    p = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * (0.5 + np.abs(rng.standard_normal(n)))).astype(f32)
    if wd != 0:
        g = np.copysign(g, p)                             # g + wd * p must not cancel either
    if t == 1:
        return p, g, np.zeros(n, f32), np.zeros(n, f32)
    gg = g.astype(f64) + wd * p.astype(f64)
    sign = np.where(gg == 0, np.where(rng.random(n) < 0.5, -1.0, 1.0), np.sign(gg))
    m = (sign * np.abs(rng.standard_normal(n)) * scale * (1 - B1 ** (t - 1))).astype(f32)
    v = (scale * scale * (1 - B2 ** (t - 1)) * rng.uniform(0.5, 1.5, n)).astype(f32)
    return p, g, m, v


def truth(p, g, m, v, t, lr, b1=B1, b2=B2, eps=EPS, wd=0.0):
    p, g, m, v = (np.asarray(a, f64) for a in (p, g, m, v))
    if wd != 0:
        g = g + wd * p
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    step_size, bc2s = lr / (1 - b1 ** t), (1 - b2 ** t) ** 0.5
    den = np.sqrt(v) / bc2s + eps
    return p - step_size * (m / den), m, v


def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def restate32(p, g, m, v, t, lr, b1=B1, b2=B2, eps=EPS, wd=0.0):
    p, g, m, v = (np.asarray(a, f32) for a in (p, g, m, v))
    w1, b2f, w2, epsf, wdf = f32(1 - b1), f32(b2), f32(1 - b2), f32(eps), f32(wd)
    bc2s = f32((1 - pow_sq(b2, t)) ** 0.5)
    step_size = f32(float(f32(lr)) / (1 - pow_sq(b1, t)))
    if wd != 0:
        g = _fma(wdf, p, g)
    d = g - m
    m = _fma(d, w1, m)
    a = v * b2f
    b = w2 * g
    v = _fma(b, g, a)
    den = np.sqrt(v) / bc2s + epsf
    u = m / den
    return _fma(-step_size, u, p), m, v


def ulp_error(got, want):
    """max |got - want| / (the spacing of float32 at |want|); 0 for empty arrays."""
    want = np.asarray(want, f64)
    if want.size == 0:
        return 0.0
    got = np.asarray(got, f64)
    assert np.isfinite(got).all()
    return float((np.abs(got - want) / np.spacing(np.abs(want).astype(f32)).astype(f64)).max())


def bar(ref_max):
    return 2.0 * ref_max + 1.0


def torch_adam_step(p, g, m, v, t, lr, wd, device="cpu", steps=1, grad_scale=None):
    """torch.optim.Adam(foreach=False) in fp32 on `device` from the state (m, v, t - 1 steps done): `steps` updates, the
    j-th with the gradient g * grad_scale(j) when given.  Returns p, m, v as numpy."""
    import torch
    q = torch.from_numpy(np.array(p, f32)).to(device).requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    if t > 1:
        opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(np.array(m, f32)).to(device),
                        "exp_avg_sq": torch.from_numpy(np.array(v, f32)).to(device)}
    g = torch.from_numpy(np.array(g, f32)).to(device)
    for j in range(steps):
        q.grad = g if grad_scale is None else g * float(grad_scale(j))
        opt.step()
    st = opt.state[q]
    return q.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()
