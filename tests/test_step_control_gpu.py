"""Gradient clipping, the non-finite guard and warmup of the native Adam on the MI355X: b2h_step_prepare's words against
the float64 truths of clip_ref.py within 1 ulp (and its partials against the restated order, bit for bit), between
poisoned guard bands, aligned and off the 16-byte grid; b2h_adam_step_guarded against b2h_adam_step; the class against a
hand-made route, bit for bit; the guard in an eager loop, in a captured step and in GraphTrainer epochs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import adam_ref
import clip_ref
import hand_pose_sl_amd as hps
import poison
from hand_pose_sl_amd import _lib
from test_graph_trainer_gpu import _conv, _h5, _json, _tpt
from tpt_train_ref import recipe_state, tokens_with_padding, train_model

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
vp, i64 = ctypes.c_void_p, ctypes.c_int64
EDGES = [1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 2 ** 20 + 5]     # chunk, wave, block and multi-block edges
SIZES = EDGES + [EDGES[i % 10] for i in range(159)]                  # 170 tensors: three launches share one flat index
SCALES = [1e-30, 1e-6, 1.0, 1e3, 1e18]
GUARD = 32                                                           # floats of NaN on either side of every gradient
NAN_WORD = 0x7FC5A5A5
ALL_ON = dict(max_grad_norm=0.05, skip_nonfinite=True, warmup_steps=3, schedule="inv_sqrt")


def _stream(dev):
    return vp(torch.cuda.current_stream(dev).cuda_stream)


def _place(sizes, mode):
    """The first float of every tensor in one buffer, GUARD floats of NaN around each: "aligned" on the 16-byte grid,
    "offset" 4, 8 or 12 bytes past it (the layout of test_adam_gpu._place)."""
    starts, total = [], 0
    for i, n in enumerate(sizes):
        start = total + GUARD + (1 + i % 3 if mode == "offset" else 0)
        starts.append(start)
        total = (start + n + GUARD + 3) // 4 * 4
    return starts, max(total, 4)


@functools.lru_cache(maxsize=None)
def _grads(scale):
    """The gradients of one scale and their float64 truth (shared: leave unchanged)."""
    rng = np.random.default_rng(int(abs(np.log10(scale))) + 40)
    grads = [(rng.standard_normal(n) * scale).astype(f32) for n in SIZES]
    return grads, clip_ref.truth_norm(grads)


class Words:
    """The five words and the workspace of one b2h_step_prepare call, each between poisoned guard bands, the float
    words 4 bytes and the int64 words 8 bytes off the 16-byte grid (the weakest alignment the header promises)."""

    def __init__(self, dev, need, skipped=0):
        P = poison.POISON
        self.norm, self.scale, self.lr = (poison.Guarded(4, P, P, dev, shift) for shift in (4, 12, 4))
        self.apply, self.skipped = poison.Guarded(8, P, P, dev, 8), poison.Guarded(8, P, None, dev, 8)
        self.skipped.view(torch.int64, (1,)).fill_(skipped)
        self.ws = poison.Guarded(max(need, 8), P, P, dev)
        self.need = need

    def read(self):
        for name in ("norm", "scale", "lr", "apply", "skipped", "ws"):
            assert getattr(self, name).guards_intact(), name + ": guard band overwritten"
        one = lambda g, dt: g.view(dt, (1,)).cpu().numpy()[0]
        return dict(norm=one(self.norm, torch.float32), scale=one(self.scale, torch.float32), lr=one(self.lr, torch.float32),
                    apply=int(one(self.apply, torch.int64)), skipped=int(one(self.skipped, torch.int64)),
                    partial=self.ws.body.view(torch.float64)[:self.need // 8].cpu().numpy())


def _prepare(dev, grads, mode="aligned", max_norm=1.0, guard=1, base_lr=1e-3, schedule=clip_ref.NONE, W=1, step=1,
             step_word=None, lr_word=None, skipped=0):
    """One b2h_step_prepare on float32 arrays placed in one guarded buffer; checks that the gradients and every guard kept
    their bits and that the read-only words were only read; returns the words and the partials."""
    lib, sizes = _lib.load(), [g.size for g in grads]
    starts, total = _place(sizes, mode)
    host = np.full(total, NAN_WORD, np.uint32)
    for g, a in zip(grads, starts):
        host[a:a + g.size] = g.view(np.uint32)
    buf = torch.from_numpy(host.view(np.int32)).to(dev)
    assert buf.data_ptr() % 16 == 0
    n = len(sizes)
    numel = (i64 * n)(*sizes)
    need = lib.b2h_step_prepare_bytes(numel, n)
    assert need == 8 * ((sum((s + 3) // 4 for s in sizes) + 1023) // 1024)
    w = Words(dev, need, skipped)
    sw = None if step_word is None else torch.tensor([step_word], dtype=torch.int64, device=dev)
    lw = None if lr_word is None else torch.tensor([lr_word], dtype=torch.float32, device=dev)
    _lib.check(lib.b2h_step_prepare((vp * n)(*[buf.data_ptr() + 4 * a for a in starts]), numel, n, max_norm, guard, base_lr,
                                    None if lw is None else vp(lw.data_ptr()), schedule, W, step,
                                    None if sw is None else vp(sw.data_ptr()), w.norm.ptr, w.scale.ptr, w.apply.ptr, w.skipped.ptr,
                                    w.lr.ptr, w.ws.ptr, need, _stream(dev)))
    out = w.read()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), host), "a gradient or one of its guards was written"
    assert sw is None or int(sw.item()) == step_word
    assert lw is None or lw.cpu().numpy()[0] == f32(lr_word)
    return out


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_norm_and_scale_within_one_ulp_of_the_truth(cuda_device, scale):
    grads, truth = _grads(scale)
    part = clip_ref.partials(grads)
    for mode in ("aligned", "offset"):
        for max_norm in (1e-3, 1.0, 1e30):
            out = _prepare(cuda_device, grads, mode, max_norm=max_norm)
            want = clip_ref.truth_scale(truth, max_norm)
            print(f"\nscale {scale:g} {mode} max_norm {max_norm:g}: norm {out['norm']!r} truth {truth!r}; scale {out['scale']!r} truth {want!r}")
            assert clip_ref.within_one_ulp(out["norm"], truth), (mode, out["norm"], truth)
            assert clip_ref.within_one_ulp(out["scale"], want), (mode, max_norm, out["scale"], want)
            assert out["apply"] == 1 and out["skipped"] == 0
            # the partials are the restated order's, bit for bit: a function of the numel list and the values alone
            assert np.array_equal(out["partial"].view(np.uint64), part.view(np.uint64)), mode
            restated = clip_ref.control(clip_ref.total(part), max_norm, 1, 1e-3, clip_ref.NONE, 1, 1)
            assert (out["norm"], out["scale"], out["apply"], out["lr"]) == restated


def test_norm_does_not_overflow_where_fp32_does(cuda_device):
    """Gradients of 1e19 and 1e-30: their squares leave fp32 at either end (torch's fp32 norm gives inf and 0)."""
    for value, n in ((1e19, 5000), (-1e19, 7), (1e-30, 5000)):
        g = np.full(n, value, f32)
        assert not 0 < float((torch.from_numpy(g) ** 2).sum()) < np.inf          # what an fp32 sum of squares makes of it
        out = _prepare(cuda_device, [g], max_norm=1.0)
        truth = clip_ref.truth_norm([g])
        assert out["norm"] > 0 and np.isfinite(out["norm"]) and clip_ref.within_one_ulp(out["norm"], truth), (value, out["norm"], truth)
        assert out["apply"] == 1 and clip_ref.within_one_ulp(out["scale"], clip_ref.truth_scale(truth, 1.0))


@pytest.mark.parametrize("W", [1, 4, 1000])
def test_learning_rate_words_follow_the_schedules(cuda_device, W):
    """t = 1 .. W + 3, both schedules, two base rates, the base rate and the step by value and as device words; every
    call stores into a slot of its own, read back once.  Stage 1 does not run: grads is NULL."""
    lib, st = _lib.load(), _stream(cuda_device)
    cases = [(s, lr, t) for s in (clip_ref.LINEAR, clip_ref.INV_SQRT) for lr in (2e-4, 1e-3) for t in range(1, W + 4)]
    out = poison.Guarded(4 * 2 * len(cases), poison.POISON, poison.POISON, cuda_device, 4)
    base = {lr: torch.tensor([lr], dtype=torch.float32, device=cuda_device) for lr in (2e-4, 1e-3)}
    steps = torch.arange(0, W + 4, dtype=torch.int64, device=cuda_device)
    for i, (s, lr, t) in enumerate(cases):
        slot = out.ptr.value + 8 * i
        _lib.check(lib.b2h_step_prepare(None, None, 129, 0.0, 0, lr, None, s, W, t, None, None, None, None, None, vp(slot), None, 0, st))
        _lib.check(lib.b2h_step_prepare(None, None, 0, -1.0, 0, 7.0, vp(base[lr].data_ptr()), s, W, 1, vp(steps.data_ptr() + 8 * (t - 1)),
                                        None, None, None, None, vp(slot + 4), None, 0, st))
    got = out.view(torch.float32, (len(cases), 2)).cpu().numpy()
    assert out.guards_intact() and steps.tolist() == list(range(W + 4))
    for (s, lr, t), (by_value, by_word) in zip(cases, got):
        want = clip_ref.truth_lr(lr, s, W, t)
        assert by_value.view(np.uint32) == by_word.view(np.uint32), (s, lr, t)
        assert clip_ref.within_one_ulp(by_value, want), (s, lr, t, by_value, want)
        assert by_value == clip_ref.control(0.0, 0.0, 0, lr, s, W, t)[3]
        if s == clip_ref.LINEAR and t >= W:
            assert by_value.view(np.uint32) == f32(lr).view(np.uint32), (lr, t)      # the base rate's own bits
        if t < W:
            assert by_value < f32(lr)
    no_schedule = _prepare(cuda_device, [np.ones(3, f32)], base_lr=2e-4, schedule=clip_ref.NONE, W=0, step=0)
    assert no_schedule["lr"].view(np.uint32) == f32(2e-4).view(np.uint32)


# ---- 2. determinism and bounds ---------------------------------------------------------------------------------------------
def test_words_are_deterministic_and_nothing_else_is_written(cuda_device):
    grads, _ = _grads(1.0)
    runs = [_prepare(cuda_device, grads, mode, max_norm=0.5, schedule=clip_ref.LINEAR, W=10, step=1, step_word=2, lr_word=2e-4,
                     skipped=5) for mode in ("aligned", "aligned", "offset")]
    for r in runs[1:]:
        assert np.array_equal(r["partial"].view(np.uint64), runs[0]["partial"].view(np.uint64))
        for k in ("norm", "scale", "lr"):
            assert r[k].view(np.uint32) == runs[0][k].view(np.uint32), k
        assert (r["apply"], r["skipped"]) == (runs[0]["apply"], runs[0]["skipped"])
    assert runs[0]["skipped"] == 5 and runs[0]["apply"] == 1 and 0 < runs[0]["scale"] < 1
    assert runs[0]["lr"] == f32(clip_ref.truth_lr(2e-4, clip_ref.LINEAR, 10, 3))
    # without clipping and guard stage 1 does not run: the workspace keeps its poison, the norm is 0, the scale 1
    off = _prepare(cuda_device, grads[:3], max_norm=0.0, guard=0)
    assert (off["norm"], off["scale"], off["apply"], off["skipped"]) == (0.0, 1.0, 1, 0)
    assert (off["partial"].view(np.uint32) == poison.POISON).all()
    # the result depends on the tensors' order and sizes only through the flat index: one tensor alone, and 81 tensors
    for sub in (grads[:1], grads[:81], grads[10:11]):
        out = _prepare(cuda_device, sub, "offset")
        assert np.array_equal(out["partial"].view(np.uint64), clip_ref.partials(sub).view(np.uint64))


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_gradients_set_the_words(cuda_device, bad):
    grads = [g.copy() for g in _grads(1.0)[0][:12]]
    grads[9] = grads[9].copy()
    grads[9][-1] = bad                                  # 4097 elements: the last, partial chunk; "offset" takes it off the grid
    for mode in ("aligned", "offset"):
        on = _prepare(cuda_device, grads, mode, guard=1, skipped=2, schedule=clip_ref.LINEAR, W=4, step=2)
        assert (on["apply"], on["skipped"], on["scale"]) == (0, 3, 0.0) and not np.isfinite(on["norm"])
        assert on["lr"] == f32(clip_ref.truth_lr(1e-3, clip_ref.LINEAR, 4, 2))
        off = _prepare(cuda_device, grads, mode, guard=0, skipped=2)
        assert (off["apply"], off["skipped"]) == (1, 2)
        assert np.isnan(off["scale"]) if np.isnan(bad) else off["scale"] == 0.0     # torch's clip_coef for such a norm


# ---- 3. the guarded update ---------------------------------------------------------------------------------------------
def _adam(dev, tensors, lr, wd, t, mode, guarded, scale=None, apply=None):
    """b2h_adam_step or b2h_adam_step_guarded on [(p, g, m, v)] placed as test_adam_gpu._native places them; returns
    [(p, m, v)] and checks guards, gradients and the two words."""
    sizes = [x[0].size for x in tensors]
    hosts, starts = [], []
    for which in range(4):
        s, total = _place(sizes, mode)
        h = np.full(total, NAN_WORD, np.uint32)
        for x, a in zip(tensors, s):
            h[a:a + x[which].size] = np.ascontiguousarray(x[which], f32).view(np.uint32)
        hosts.append(h)
        starts.append(s)
    bufs = [torch.from_numpy(h.view(np.int32)).to(dev) for h in hosts]
    n = len(sizes)
    ptrs = [(vp * n)(*[b.data_ptr() + 4 * s[i] for i in range(n)]) for b, s in zip(bufs, starts)]
    sw = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=dev)
    aw = None if apply is None else torch.tensor([apply], dtype=torch.int64, device=dev)
    lib = _lib.load()
    head = (ptrs[0], ptrs[1], ptrs[2], ptrs[3], (i64 * n)(*sizes), n, lr, None, adam_ref.B1, adam_ref.B2, adam_ref.EPS, wd, t, None)
    if guarded:
        _lib.check(lib.b2h_adam_step_guarded(*head, None if sw is None else vp(sw.data_ptr()),
                                             None if aw is None else vp(aw.data_ptr()), _stream(dev)))
    else:
        _lib.check(lib.b2h_adam_step(*head, _stream(dev)))
    outs = [b.cpu().numpy().view(np.uint32) for b in bufs]
    assert sw is None or sw.cpu().numpy()[0].view(np.uint32) == f32(scale).view(np.uint32)
    assert aw is None or int(aw.item()) == apply
    assert np.array_equal(outs[1], hosts[1]), "a gradient or one of its guards was written"
    for which in (0, 2, 3):
        guard = np.ones(outs[which].shape, bool)
        for a, size in zip(starts[which], sizes):
            guard[a:a + size] = False
        assert (outs[which][guard] == NAN_WORD).all(), "a guard word was written"
    return [tuple(outs[w][starts[w][i]:starts[w][i] + sizes[i]].view(f32).copy() for w in (0, 2, 3)) for i in range(n)]


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for s, t in zip(a, b) for x, y in zip(s, t))


def _split(arrays, sizes):
    out, at = [], 0
    for n in sizes:
        out.append(tuple(a[at:at + n] for a in arrays))
        at += n
    return out


def test_guarded_update_against_the_plain_one(cuda_device):
    dev, sizes = cuda_device, adam_ref.SIZES[:17] + [0]
    for i, (t, k, wd, lr) in enumerate(adam_ref.cases()[::3]):
        p, g, m, v = adam_ref.inputs(sum(sizes), t, k, wd, 300 + i)
        tensors = _split((p, g, m, v), sizes)
        for mode in ("aligned", "offset"):
            plain = _adam(dev, tensors, lr, wd, t, mode, False)
            assert _same_bits(plain, _adam(dev, tensors, lr, wd, t, mode, True)), "both words NULL"
            assert _same_bits(plain, _adam(dev, tensors, lr, wd, t, mode, True, scale=1.0, apply=1))
            assert _same_bits(plain, _adam(dev, tensors, lr, wd, t, mode, True, apply=7)), "any non-zero word applies"
            for s in (0.37, 1e-3, 0.0):
                gs = (torch.from_numpy(g).to(dev) * torch.tensor(s, dtype=torch.float32, device=dev)).cpu().numpy()   # torch's fp32 product
                fed = _adam(dev, _split((p, gs, m, v), sizes), lr, wd, t, mode, False)
                assert _same_bits(fed, _adam(dev, tensors, lr, wd, t, mode, True, scale=s, apply=1)), (t, k, mode, s)
            before = [(x[0], x[2], x[3]) for x in tensors]
            assert _same_bits(before, _adam(dev, tensors, lr, wd, t, mode, True, scale=0.37, apply=0)), "apply 0 wrote"
            assert _same_bits(before, _adam(dev, tensors, lr, wd, t, mode, True, apply=0))


def test_guarded_update_over_two_launches_against_the_plain_one(cuda_device):
    """81 tensors: one more than a launch holds, so the guarded kernel's second launch and its chunk locator are met.
    Sizes (37 i) % 53 (0 at i = 0 and 53), two raised past a wave's 64 chunks; the last tensor is the second launch."""
    dev, sizes = cuda_device, [(37 * i) % 53 for i in range(81)]
    sizes[20], sizes[80] = 257, 1025
    assert len(sizes) == 81 and sizes.count(0) >= 1
    t, k, wd, lr = adam_ref.cases()[5]
    p, g, m, v = adam_ref.inputs(sum(sizes), t, k, wd, 340)
    tensors = _split((p, g, m, v), sizes)
    before = [(x[0], x[2], x[3]) for x in tensors]
    for mode in ("aligned", "offset"):
        plain = _adam(dev, tensors, lr, wd, t, mode, False)
        assert not _same_bits(plain, before), "the plain update changed nothing: the comparison below would be empty"
        assert _same_bits(plain, _adam(dev, tensors, lr, wd, t, mode, True, scale=1.0, apply=1)), mode
        assert _same_bits(before, _adam(dev, tensors, lr, wd, t, mode, True, scale=1.0, apply=0)), "apply 0 wrote"


def test_clipped_update_within_the_bar_of_torch_on_this_gpu(cuda_device):
    """clip_grad_norm_ + torch.optim.Adam(foreach=False) on this GPU against the float64 truth gives the bar (2 x its
    largest error + 1 ulp, adam_ref.bar); b2h_step_prepare + b2h_adam_step_guarded must be within it."""
    dev, n, lib = cuda_device, sum(adam_ref.SIZES), _lib.load()
    ref, rows, kinds = [0.0] * 3, [], set()
    for i, (t, k, wd, lr) in enumerate(adam_ref.cases()):
        p, g, m, v = adam_ref.inputs(n, t, k, wd, 100 + i)
        coef = clip_ref.truth_scale(clip_ref.truth_norm([g]), 1.0)
        kinds.add(coef < 1.0)
        want = clip_ref.clipped(adam_ref.truth, p, g, m, v, t, lr, wd, coef)
        # torch's route
        q = torch.from_numpy(p.copy()).to(dev).requires_grad_(True)
        opt = torch.optim.Adam([q], lr=lr, betas=(adam_ref.B1, adam_ref.B2), eps=adam_ref.EPS, weight_decay=wd, foreach=False)
        if t > 1:
            opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()).to(dev),
                            "exp_avg_sq": torch.from_numpy(v.copy()).to(dev)}
        q.grad = torch.from_numpy(g.copy()).to(dev)
        torch.nn.utils.clip_grad_norm_([q], 1.0, foreach=False)
        opt.step()
        theirs = (q.detach().cpu().numpy(), opt.state[q]["exp_avg"].cpu().numpy(), opt.state[q]["exp_avg_sq"].cpu().numpy())
        # the native route: the words stay on the device
        dp, dg, dm, dv = (torch.from_numpy(a.copy()).to(dev) for a in (p, g, m, v))
        sizes = (i64 * 1)(n)
        ws = torch.empty(lib.b2h_step_prepare_bytes(sizes, 1) // 8, dtype=torch.float64, device=dev)
        scale, apply = torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        one = lambda x: (vp * 1)(x.data_ptr())
        _lib.check(lib.b2h_step_prepare(one(dg), sizes, 1, 1.0, 1, lr, None, clip_ref.NONE, 1, t, None, None, vp(scale.data_ptr()),
                                        vp(apply.data_ptr()), None, None, vp(ws.data_ptr()), 8 * ws.numel(), _stream(dev)))
        _lib.check(lib.b2h_adam_step_guarded(one(dp), one(dg), one(dm), one(dv), sizes, 1, lr, None, adam_ref.B1, adam_ref.B2,
                                             adam_ref.EPS, wd, t, None, vp(scale.data_ptr()), vp(apply.data_ptr()), _stream(dev)))
        ours = tuple(x.cpu().numpy() for x in (dp, dm, dv))
        assert int(apply.item()) == 1 and clip_ref.within_one_ulp(scale.cpu().numpy()[0], coef)
        rows.append(((t, k, wd, lr), [adam_ref.ulp_error(a, b) for a, b in zip(ours, want)]))
        ref = [max(a, b) for a, b in zip(ref, [adam_ref.ulp_error(a, b) for a, b in zip(theirs, want)])]
    print("\nclip_grad_norm_ + torch.optim.Adam(foreach=False) on the GPU, max ulp error of (p, m, v):", ["%.2f" % e for e in ref])
    print("b2h_step_prepare + b2h_adam_step_guarded, max ulp error of (p, m, v):", ["%.2f" % max(r[1][q] for r in rows) for q in range(3)])
    assert kinds == {True, False} and all(np.isfinite(ref))
    for case, errs in rows:
        for name, e, r in zip("pmv", errs, ref):
            assert e <= adam_ref.bar(r), f"{case} {name}: {e:.2f} ulp > 2 * {r:.2f} + 1"


# ---- 4. the class against a hand-made route ------------------------------------------------------------------------------
def _small_tpt(dev, seed=31):
    torch.manual_seed(seed)
    return hps.TextPoseTransformer(1000, 8, 2, 4, 128, 42, 1, 1, dropout=0.0).to(dev).train()


def _batch(dev, seed=5, B=2, S=7, T=15):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randint(1, 1000, (B, S), generator=gen).to(dev), (torch.rand((B, T, 8, 2), generator=gen) - 0.5).to(dev),
            (torch.rand((B, T, 21, 2), generator=gen) - 0.5).to(dev), torch.tensor([T, T - 4], dtype=torch.int64, device=dev))


def _backward(m, opt, batch, weight=None):
    tok, x, target, lengths = batch
    opt.zero_grad(set_to_none=True)
    loss = hps.masked_pose_l1(m(tok, x), target, lengths)
    (loss if weight is None else loss * weight).backward()


def _assert_same_training_state(m, opt, twin, twin_opt):
    for (k, a), b in zip(m.named_parameters(), twin.parameters()):
        assert torch.equal(a, b), k
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[a][key], twin_opt.state[b][key]), (k, key)


def test_class_equals_a_hand_made_route_bit_for_bit(cuda_device):
    dev, lib, lr = cuda_device, _lib.load(), 1e-3
    m, twin = _small_tpt(dev), _small_tpt(dev)
    opt = hps.Adam(m.parameters(), lr=lr, max_grad_norm=0.05, warmup_steps=2)
    twin_opt = hps.Adam(twin.parameters(), lr=lr)
    scales, rates = [], []
    for step in range(1, 4):
        batch = _batch(dev, seed=step)
        _backward(m, opt, batch)
        kept = [q.grad.clone() for q in m.parameters()]
        opt.step()
        assert all(torch.equal(q.grad, g) for q, g in zip(m.parameters(), kept)), "p.grad is left unscaled"
        # the twin: b2h_step_prepare by hand, torch scales .grad, the rate by hand, a plain hps.Adam
        _backward(twin, twin_opt, batch)
        params = [q for q in twin.parameters() if q.grad is not None]
        n = len(params)
        sizes = (i64 * n)(*[q.numel() for q in params])
        ws = torch.empty(max(lib.b2h_step_prepare_bytes(sizes, n) // 8, 1), dtype=torch.float64, device=dev)
        norm, scale, rate = (torch.zeros(1, device=dev) for _ in range(3))
        _lib.check(lib.b2h_step_prepare((vp * n)(*[q.grad.data_ptr() for q in params]), sizes, n, 0.05, 0, lr, None, clip_ref.LINEAR,
                                        2, step, None, vp(norm.data_ptr()), vp(scale.data_ptr()), None, None, vp(rate.data_ptr()),
                                        vp(ws.data_ptr()), 8 * ws.numel(), _stream(dev)))
        for q in params:
            q.grad.mul_(scale)
        twin_opt.param_groups[0]["lr"] = float(rate.item())
        twin_opt.step()
        scales.append(float(scale.item()))
        rates.append(float(rate.item()))
        assert torch.equal(opt.grad_norm, norm) and opt.current_lr() == rates[-1]
        want = torch.sqrt(sum((g.double() ** 2).sum() for g in kept)).item()
        assert clip_ref.within_one_ulp(norm.item(), want)
        _assert_same_training_state(m, opt, twin, twin_opt)
    assert min(scales) < 1.0, scales                                    # at least one step clipped
    assert rates == [float(f32(clip_ref.truth_lr(lr, clip_ref.LINEAR, 2, t))) for t in (1, 2, 3)] and rates[0] < rates[1] == rates[2]
    assert opt.steps_done() == 3 and opt.skipped_steps() == 0 and opt._lr_word.item() == f32(lr)      # the base rate stays


# ---- 5. the guard, eager ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_guard_skips_a_non_finite_step_and_the_next_one_is_untouched(cuda_device, bad):
    dev = cuda_device
    m, twin = _small_tpt(dev), _small_tpt(dev)
    opt, twin_opt = (hps.Adam(x.parameters(), lr=1e-3, skip_nonfinite=True) for x in (m, twin))
    first, second = _batch(dev, 1), _batch(dev, 2)
    for x, o in ((m, opt), (twin, twin_opt)):
        _backward(x, o, first)
        o.step()
    before = [(q.detach().clone(), opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone()) for q in m.parameters()]
    _backward(m, opt, second)
    # a gradient tensor off the 16-byte grid whose last chunk is partial: a view into a larger buffer
    q = max(m.parameters(), key=lambda t: t.numel() if t.numel() % 4 else 0)
    assert q.numel() % 4
    store = torch.zeros(q.numel() + 8, device=dev)
    view = store[1:1 + q.numel()].view_as(q)
    assert view.data_ptr() % 16 == 4
    view.copy_(q.grad)
    view.view(-1)[-1] = bad
    q.grad = view
    opt.step()
    assert opt.steps_done() == 1 and opt.skipped_steps() == 1 and not np.isfinite(opt.grad_norm.item())
    for p, (p0, m0, v0) in zip(m.parameters(), before):
        assert torch.equal(p, p0) and torch.equal(opt.state[p]["exp_avg"], m0) and torch.equal(opt.state[p]["exp_avg_sq"], v0)
    for x, o in ((m, opt), (twin, twin_opt)):                          # the next finite step: as if the bad one never came
        _backward(x, o, second)
        o.step()
    assert opt.steps_done() == twin_opt.steps_done() == 2 and opt.skipped_steps() == 1 and twin_opt.skipped_steps() == 0
    _assert_same_training_state(m, opt, twin, twin_opt)
    assert float(opt.state_dict()["state"][0]["step"]) == 2.0


def test_without_the_guard_a_nan_gradient_reaches_every_weight_as_with_torch(cuda_device):
    dev = cuda_device
    m = _small_tpt(dev)
    opt = hps.Adam(m.parameters(), lr=1e-3, max_grad_norm=1.0)
    _backward(m, opt, _batch(dev, 1))
    next(m.parameters()).grad.view(-1)[0] = float("nan")
    theirs = [q.detach().clone().requires_grad_(True) for q in m.parameters()]
    for t, q in zip(theirs, m.parameters()):
        t.grad = q.grad.clone()
    torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    torch.optim.Adam(theirs, lr=1e-3).step()
    opt.step()
    assert opt.steps_done() == 1 and opt.skipped_steps() == 0 and np.isnan(opt.grad_norm.item())
    for q, t in zip(m.parameters(), theirs):
        assert bool(torch.isnan(q).all()) and bool(torch.isnan(t).all())


# ---- 6. a captured step --------------------------------------------------------------------------------------------------
def test_captured_step_skips_on_the_device_and_warms_up_across_replays(cuda_device):
    dev, lr, W = cuda_device, 1e-3, 4
    state = recipe_state(90, 50, 1, 1)
    gen = torch.Generator().manual_seed(91)
    batch = (tokens_with_padding(2, 7, 50, gen).to(dev), torch.randn((2, 15, 12, 2), generator=gen).to(dev),
             torch.randn((2, 15, 21, 2), generator=gen).to(dev), torch.tensor([15, 11], dtype=torch.int64, device=dev))
    w = torch.ones(1, device=dev)

    def make():
        m = train_model(state, 0.0, dev)
        return m, hps.Adam(m.parameters(), lr=lr, weight_decay=1e-2, max_grad_norm=0.5, skip_nonfinite=True, warmup_steps=W)

    m, opt = make()
    s = torch.cuda.Stream(dev)                               # warm-up on a side stream, as torch's docs do: step 1
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        _backward(m, opt, batch, w)
        opt.step()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    assert opt.steps_done() == 1 and opt.current_lr() == float(f32(clip_ref.truth_lr(lr, clip_ref.LINEAR, W, 1)))
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):                            # one stream: no parallel branches
        _backward(m, opt, batch, w)
        opt.step()
    assert opt.steps_done() == 1                             # capturing ran nothing
    rates, norms = [], []
    for value in (1.0, float("inf"), 1.0):
        w.fill_(value)
        graph.replay()
        rates.append(opt.current_lr())
        norms.append(opt.grad_norm.item())
    assert opt.steps_done() == 3 and opt.skipped_steps() == 1
    # the rate of the update about to be made: t = 2, then 3 twice (the skipped replay did not advance the step word)
    assert rates == [float(f32(clip_ref.truth_lr(lr, clip_ref.LINEAR, W, t))) for t in (2, 3, 3)] and rates[0] < rates[1]
    assert np.isfinite(norms[0]) and not np.isfinite(norms[1]) and np.isfinite(norms[2])
    twin, twin_opt = make()
    w.fill_(1.0)
    for _ in range(3):                                       # the warm-up and the two finite replays
        _backward(twin, twin_opt, batch, w)
        twin_opt.step()
    assert twin_opt.steps_done() == 3 and twin_opt.skipped_steps() == 0
    _assert_same_training_state(m, opt, twin, twin_opt)
    fresh, _ = make()
    assert any(not torch.equal(a, b) for a, b in zip(m.parameters(), fresh.parameters()))


# ---- 7. GraphTrainer -------------------------------------------------------------------------------------------------------
def _epochs(dev, make_model, make_loader, options, epochs=2, between=None):
    eager_model, eager_loader = make_model(dev), make_loader()
    eager_opt = hps.Adam(eager_model.parameters(), lr=1e-3, **options)
    torch.manual_seed(77)
    eager = []
    for e in range(epochs):
        if e and between:
            between(eager_opt)
        eager.append(hps.train_epoch(eager_model, eager_loader, None, eager_opt, loss="L1"))
    model, loader = make_model(dev), make_loader()
    opt = hps.Adam(model.parameters(), lr=1e-3, **options)
    trainer = hps.GraphTrainer(model, loader, opt, loss="L1")
    torch.manual_seed(77)
    got = []
    for e in range(epochs):
        if e and between:
            between(opt)
        got.append(trainer.epoch())
    assert got == eager and all(np.isfinite(v) for v in got), (got, eager)
    _assert_same_training_state(model, opt, eager_model, eager_opt)
    assert opt.steps_done() == eager_opt.steps_done() and opt.skipped_steps() == eager_opt.skipped_steps() == 0
    assert opt.current_lr() == eager_opt.current_lr() and torch.equal(opt.grad_norm, eager_opt.grad_norm)
    return trainer, opt


def test_trainer_with_every_option_on_equals_train_epoch(cuda_device):
    trainer, opt = _epochs(cuda_device, _tpt, lambda: hps.DeviceLoader(_h5(), 2, 7, selection="first"), ALL_ON)
    assert trainer.captures == 1 and trainer.replays == 3 and opt.steps_done() == 6
    assert opt.current_lr() == float(f32(clip_ref.truth_lr(1e-3, clip_ref.INV_SQRT, 3, 6)))      # t = 6, W = 3


def test_trainer_recaptures_when_max_grad_norm_changes(cuda_device):
    def change(opt):
        opt.max_grad_norm = 0.01
    trainer, _ = _epochs(cuda_device, _tpt, lambda: hps.DeviceLoader(_h5(), 2, 7, selection="first"), ALL_ON, epochs=3,
                         between=change)
    assert trainer.captures == 2


def test_trainer_convmodel_with_every_option_on(cuda_device):
    trainer, _ = _epochs(cuda_device, _conv, lambda: hps.DeviceLoader(_json(), 2, 7, selection="randomcrop", pad="frame0",
                                                                      shuffle=True), ALL_ON)
    assert trainer.captures == 1
