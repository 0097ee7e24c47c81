"""Gradient clipping, the non-finite guard and warmup of the native Adam (b2h_step_prepare, b2h_adam_step_guarded,
kernel_step_control.h, kernel_adam.h) without a GPU: the entry points declared, typed and exported; every refusal, which
launches nothing, and the empty calls; the three new kernels compile for gfx950 without scratch or spills and
b2h_adam_step_k is still one kernel; the numpy restatements (clip_ref.py) against torch.nn.utils.clip_grad_norm_ followed
by torch.optim.Adam(foreach=False) on the CPU over ten steps at adam_ref's bar; the class's refusals and its state_dict."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_ref
import clip_ref
import hand_pose_sl_amd as hps
from hand_pose_sl_amd import _lib
from kernel_remarks import ROOT, kernel_remarks

f32, f64 = np.float32, np.float64
vp, i64, cf = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float


def test_entry_points_declared_typed_and_exported():
    header = " ".join(open(os.path.join(ROOT, "include", "b2h.h")).read().split())
    for decl in ("size_t b2h_step_prepare_bytes(const int64_t* numel, int n_tensors);",
                 "int b2h_step_prepare(const float* const* grads, const int64_t* numel, int n_tensors, float max_norm, int guard, "
                 "float base_lr, const float* base_lr_dev, int schedule, int64_t warmup_steps, int64_t step, const int64_t* "
                 "step_dev, float* norm_out, float* scale_out, int64_t* apply_out, int64_t* skipped, float* lr_out, void* "
                 "workspace, size_t workspace_bytes, void* stream);",
                 "int b2h_adam_step_guarded(float* const* params, const float* const* grads, float* const* exp_avg, float* const* "
                 "exp_avg_sq, const int64_t* numel, int n_tensors, float lr, const float* lr_dev, float beta1, float beta2, float "
                 "eps, float weight_decay, int64_t step, const int64_t* step_dev, const float* grad_scale_dev, const int64_t* "
                 "apply_dev, void* stream);",
                 "enum { B2H_SCHED_NONE = 0, B2H_SCHED_LINEAR = 1, B2H_SCHED_INV_SQRT = 2 };"):
        assert decl in header, decl
    assert header.count("b2h_adam_step below is that optimizer") == 3
    i64p = ctypes.POINTER(i64)
    assert _lib.SYMBOLS["b2h_step_prepare_bytes"] == (ctypes.c_size_t, [i64p, ctypes.c_int])
    assert _lib.SYMBOLS["b2h_step_prepare"] == (ctypes.c_int, [ctypes.POINTER(vp), i64p, ctypes.c_int, cf, ctypes.c_int, cf, vp,
                                                               ctypes.c_int, i64, i64, vp, vp, vp, vp, vp, vp, vp,
                                                               ctypes.c_size_t, vp])
    adam = _lib.SYMBOLS["b2h_adam_step"]
    assert _lib.SYMBOLS["b2h_adam_step_guarded"] == (adam[0], adam[1][:-1] + [vp, vp, vp])
    assert _lib.SCHEDULES == {"none": 0, "linear": 1, "inv_sqrt": 2}
    lib = _lib.load()                                    # types every symbol: a missing export raises here
    # 8 bytes per block of 1024 chunks of the flat index; a tensor's last chunk may be partial
    sizes = lambda *n: (i64 * len(n))(*n)
    assert lib.b2h_step_prepare_bytes(sizes(1), 1) == 8 and lib.b2h_step_prepare_bytes(sizes(4096), 1) == 8
    assert lib.b2h_step_prepare_bytes(sizes(4097), 1) == 16 and lib.b2h_step_prepare_bytes(sizes(*[1] * 1025), 1025) == 16
    assert lib.b2h_step_prepare_bytes(sizes(0, 0), 2) == 0 and lib.b2h_step_prepare_bytes(None, 0) == 0
    assert lib.b2h_step_prepare_bytes(None, 3) == 0 and lib.b2h_step_prepare_bytes(sizes(-1), 1) == 0


# made-up addresses that nothing dereferences: a refused call launches nothing
G, WS, NORM, SCALE, APPLY, SKIPPED, LR, BASE, STEP = 0x20000, 0x90000, 0x50000, 0x50010, 0x50020, 0x50030, 0x50040, 0x60000, 0x60010


def _prepare(lib, g=(G,), sizes=(16,), n=None, max_norm=1.0, guard=1, base_lr=1e-3, base_lr_dev=None, schedule=1, warmup=4,
             step=1, step_dev=None, norm=NORM, scale=SCALE, apply=APPLY, skipped=SKIPPED, lr=LR, ws=WS, ws_bytes=1 << 20):
    grads = None if g is None else (vp * len(g))(*g)
    numel = None if sizes is None else (i64 * len(sizes))(*sizes)
    n = len(sizes) if n is None else n
    return lib.b2h_step_prepare(grads, numel, n, max_norm, guard, base_lr, base_lr_dev, schedule, warmup, step, step_dev, norm,
                                scale, apply, skipped, lr, ws, ws_bytes, None)


def _guarded(lib, p=(0x10000,), g=(G,), m=(0x30000,), v=(0x40000,), sizes=(16,), n=None, lr=1e-3, lr_dev=None, b1=0.9, b2=0.999,
             eps=1e-8, wd=0.0, step=1, step_dev=None, scale_dev=SCALE, apply_dev=APPLY):
    arr = [None if a is None else (vp * len(a))(*a) for a in (p, g, m, v)]
    numel = None if sizes is None else (i64 * len(sizes))(*sizes)
    n = len(sizes) if n is None else n
    return lib.b2h_adam_step_guarded(*arr, numel, n, lr, lr_dev, b1, b2, eps, wd, step, step_dev, scale_dev, apply_dev, None)


def test_refusals_launch_nothing_and_empty_calls_return_ok():
    """No GPU here: a call that reached a launch would fail with another status (B2H_ERR_HIP), so ERR_INVALID with a
    message shows the refusal came first."""
    lib = _lib.load()
    nan = float("nan")
    refused = {
        "n_tensors < 0": lambda: _prepare(lib, n=-1),
        "NaN max_norm": lambda: _prepare(lib, max_norm=nan),
        "unknown schedule": lambda: _prepare(lib, schedule=3),
        "negative schedule": lambda: _prepare(lib, schedule=-1),
        "warmup 0 with a schedule": lambda: _prepare(lib, warmup=0),
        "warmup < 0 with a schedule": lambda: _prepare(lib, schedule=2, warmup=-5),
        "step 0 with a schedule, no step_dev": lambda: _prepare(lib, step=0),
        "step < 0 with step_dev": lambda: _prepare(lib, step=-1, step_dev=STEP),
        "base_lr < 0": lambda: _prepare(lib, base_lr=-1e-3),
        "base_lr NaN": lambda: _prepare(lib, base_lr=nan),
        "NULL grads": lambda: _prepare(lib, g=None),
        "NULL numel": lambda: _prepare(lib, sizes=None, n=1),
        "NULL gradient": lambda: _prepare(lib, g=(None,)),
        "numel < 0": lambda: _prepare(lib, sizes=(-1,)),
        "gradient misaligned by 2": lambda: _prepare(lib, g=(G + 2,)),
        "gradient misaligned by 1, 90th of 90": lambda: _prepare(lib, g=[G + 64 * i for i in range(89)] + [G + 64 * 89 + 1],
                                                                 sizes=[16] * 90),
        "NULL workspace": lambda: _prepare(lib, ws=None),
        "workspace misaligned by 8": lambda: _prepare(lib, ws=WS + 8),
        "workspace too small": lambda: _prepare(lib, sizes=(4097,), ws_bytes=8),
        "norm_out misaligned": lambda: _prepare(lib, norm=NORM + 2),
        "scale_out misaligned": lambda: _prepare(lib, scale=SCALE + 1),
        "lr_out misaligned": lambda: _prepare(lib, lr=LR + 2),
        "apply_out misaligned by 4": lambda: _prepare(lib, apply=APPLY + 4),
        "skipped misaligned by 4": lambda: _prepare(lib, skipped=SKIPPED + 4),
        "base_lr_dev misaligned": lambda: _prepare(lib, base_lr_dev=BASE + 2),
        "step_dev misaligned by 4": lambda: _prepare(lib, step_dev=STEP + 4),
        "norm_out is scale_out": lambda: _prepare(lib, scale=NORM),
        "lr_out inside apply_out": lambda: _prepare(lib, lr=APPLY + 4),
        "skipped is apply_out": lambda: _prepare(lib, skipped=APPLY),
        "norm_out inside the workspace": lambda: _prepare(lib, norm=WS + 4),
        "scale_out inside a gradient": lambda: _prepare(lib, scale=G + 60),
        "workspace over a gradient": lambda: _prepare(lib, ws=G + 48),
        "lr_out is base_lr_dev": lambda: _prepare(lib, base_lr_dev=BASE, lr=BASE),
        "apply_out is step_dev": lambda: _prepare(lib, step_dev=STEP, apply=STEP),
        "NULL grads, guard only": lambda: _prepare(lib, g=None, max_norm=0.0, guard=1),
        # the guarded update: b2h_adam_step's list, and the two words
        "guarded: NULL params": lambda: _guarded(lib, p=None),
        "guarded: n_tensors < 0": lambda: _guarded(lib, n=-1),
        "guarded: NULL gradient": lambda: _guarded(lib, g=(None,)),
        "guarded: misaligned by 2": lambda: _guarded(lib, m=(0x30002,)),
        "guarded: numel < 0": lambda: _guarded(lib, sizes=(-1,)),
        "guarded: beta2 = 1": lambda: _guarded(lib, b2=1.0),
        "guarded: eps NaN": lambda: _guarded(lib, eps=nan),
        "guarded: lr < 0": lambda: _guarded(lib, lr=-1e-3),
        "guarded: step 0 without step_dev": lambda: _guarded(lib, step=0),
        "guarded: p overlaps m": lambda: _guarded(lib, m=(0x10000 + 60,)),
        "guarded: grad_scale_dev misaligned": lambda: _guarded(lib, scale_dev=SCALE + 2),
        "guarded: apply_dev misaligned by 4": lambda: _guarded(lib, apply_dev=APPLY + 4),
        "guarded: grad_scale_dev inside params": lambda: _guarded(lib, scale_dev=0x10000 + 8),
        "guarded: apply_dev inside exp_avg_sq": lambda: _guarded(lib, apply_dev=0x40000 + 56),
    }
    for what, call in refused.items():
        assert call() == _lib.ERR_INVALID, what
        assert _lib.last_error(), what
        with pytest.raises(ValueError):
            _lib.check(call())
    # empty calls: nothing to reduce and no word to store launches nothing
    none = dict(norm=None, scale=None, apply=None, skipped=None, lr=None)
    assert _prepare(lib, g=None, sizes=None, n=0, ws=None, ws_bytes=0, **none) == _lib.OK
    assert _prepare(lib, sizes=(0,), ws=None, ws_bytes=0, **none) == _lib.OK                      # all sizes 0
    assert _prepare(lib, g=(None, 0x3), sizes=(0, 0), ws=None, ws_bytes=0, **none) == _lib.OK     # an empty tensor's pointer
    assert _prepare(lib, g=None, sizes=None, n=5, max_norm=0.0, guard=0, ws=None, ws_bytes=0, **none) == _lib.OK   # stage 1 off
    assert _prepare(lib, g=None, sizes=None, n=0, max_norm=-1.0, guard=0, schedule=0, warmup=0, step=0, ws=None, ws_bytes=0,
                    **none) == _lib.OK                                                            # no schedule: W, step unread
    assert lib.b2h_adam_step_guarded(None, None, None, None, None, 0, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 1, None, None, None,
                                     None) == _lib.OK
    assert _guarded(lib, sizes=(0,)) == _lib.OK
    assert _guarded(lib, p=(None,), g=(None,), m=(None,), v=(0x3,), sizes=(0,), scale_dev=None, apply_dev=None) == _lib.OK


def test_new_kernels_have_no_scratch_or_spills_and_adam_step_is_one_kernel():
    kernels, listing = kernel_remarks()
    assert len([n for n in kernels if "b2h_adam_step_k" in n]) == 1
    for key in ("b2h_grad_sumsq_k", "b2h_step_control_k", "b2h_adam_guarded_k"):
        new = {n: res for n, res in kernels.items() if key in n}
        assert len(new) == 1, (key, sorted(new))
        for name, res in new.items():
            print(name, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "LDS", res["LDS Size [bytes/block]"], "occupancy",
                  res["Occupancy [waves/SIMD]"])
            assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
    text = open(listing).read()

    def body(mangled):
        b = text[text.index(mangled + ":"):]
        return b[:b.index("s_endpgm")]
    sumsq = body("_ZN3b2h16b2h_grad_sumsq_kENS_6SsArgsE")
    assert re.search(r"\bglobal_load_dwordx4\b", sumsq) and "atomic" not in sumsq and "v_fma_f64" in sumsq
    assert "atomic" not in body("_ZN3b2h18b2h_step_control_kENS_6ScArgsE")
    # the guarded update: the loads, stores and IEEE divisions of b2h_adam_step_k, no more
    guarded = body("_ZN3b2h18b2h_adam_guarded_kENS_6AdArgsENS_7AdGuardE")
    assert len(re.findall(r"\bglobal_load_dwordx4\b", guarded)) == 4 and len(re.findall(r"\bglobal_store_dwordx4\b", guarded)) == 3
    assert "atomic" not in guarded and len(re.findall(r"\bv_div_fixup_f32\b", guarded)) == 10


# ---- the restatements against torch on the CPU -----------------------------------------------------------------------
N_CPU, MAX_NORM = 2 ** 16, 1.0


def _grad_scale(j):
    return f32(1 + j / 8)                                 # as test_adam_cpu: the same gradient, growing


def _torch_clipped_steps(p, g, m, v, t, lr, wd):
    """Ten steps of clip_grad_norm_ and torch.optim.Adam(foreach=False) in fp32; p, m, v and torch's ten coefficients."""
    q = torch.from_numpy(np.array(p, f32)).requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(adam_ref.B1, adam_ref.B2), eps=adam_ref.EPS, weight_decay=wd, foreach=False)
    if t > 1:
        opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(np.array(m, f32)),
                        "exp_avg_sq": torch.from_numpy(np.array(v, f32))}
    coefs = []
    for j in range(10):
        q.grad = torch.from_numpy(np.array(g, f32)) * float(_grad_scale(j))
        norm = torch.nn.utils.clip_grad_norm_([q], MAX_NORM, foreach=False)
        coefs.append(min(float(f32(MAX_NORM) / (norm.numpy() + f32(1e-6))), 1.0))
        opt.step()
    st = opt.state[q]
    return (q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()), coefs


def test_restatements_match_clip_grad_norm_and_adam_on_the_cpu_over_ten_steps():
    ref, rows, kinds = [0.0] * 3, [], set()
    for i, (t, k, wd, lr) in enumerate(adam_ref.cases()):
        p, g, m, v = adam_ref.inputs(N_CPU, t, k, wd, 700 + i)
        got_torch, torch_coefs = _torch_clipped_steps(p, g, m, v, t, lr, wd)
        want, got_32 = (p, m, v), (p, m, v)
        for j in range(10):
            gj = g * _grad_scale(j)
            coef = clip_ref.truth_scale(clip_ref.truth_norm([gj]), MAX_NORM)
            kinds.add(coef < 1.0)
            # torch's own coefficient: an fp32 norm of N terms errs by less than N * 2^-24 of itself (any summation order)
            assert abs(torch_coefs[j] - coef) <= coef * N_CPU * 2.0 ** -24, (t, k, j, torch_coefs[j], coef)
            _, scale, apply, _ = clip_ref.control(clip_ref.total(clip_ref.partials([gj])), MAX_NORM, 1, lr, clip_ref.NONE, 1, t + j)
            assert apply == 1 and clip_ref.within_one_ulp(scale, coef), (t, k, j, scale, coef)
            assert (coef < 1.0) == (scale < 1.0)
            want = clip_ref.clipped(adam_ref.truth, want[0], gj, want[1], want[2], t + j, lr, wd, coef)
            got_32 = clip_ref.clipped(adam_ref.restate32, got_32[0], gj, got_32[1], got_32[2], t + j, lr, wd, scale)
        e_torch = [adam_ref.ulp_error(a, b) for a, b in zip(got_torch, want)]
        rows.append(((t, k, wd, lr), [adam_ref.ulp_error(a, b) for a, b in zip(got_32, want)]))
        ref = [max(a, b) for a, b in zip(ref, e_torch)]
    print("\nclip_grad_norm_ + torch.optim.Adam(foreach=False) on the CPU, max ulp error of (p, m, v):", ["%.2f" % e for e in ref])
    print("fp32 restatement of the clipped update, max ulp error of (p, m, v):", ["%.2f" % max(r[1][q] for r in rows) for q in range(3)])
    assert kinds == {True, False}, "max_norm = 1 must clip some cases and leave others alone"
    assert all(np.isfinite(ref))
    for case, errs in rows:
        for name, e, r in zip("pmv", errs, ref):
            assert e <= adam_ref.bar(r), f"{case} {name}: restatement {e:.2f} ulp > 2 * {r:.2f} + 1"


def test_partial_order_of_the_restatement():
    """The restated tree against a plain float64 sum, and the pieces of its order that the GPU test relies on."""
    rng = np.random.default_rng(3)
    grads = [rng.standard_normal(n).astype(f32) for n in [1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097] * 17]   # 170: 3 launches
    part = clip_ref.partials(grads)
    chunks = sum((g.size + 3) // 4 for g in grads)
    assert part.size == (chunks + 1023) // 1024
    tot, truth = clip_ref.total(part), clip_ref.truth_norm(grads) ** 2
    assert abs(tot - truth) <= truth * 1e-12
    assert np.array_equal(clip_ref.partials(grads[:1]), [float(grads[0][0]) ** 2])
    # an empty tensor has no chunk of the flat index (a leading one would move the 80-tensor launch boundaries, and with
    # them the two halves of a block that two launches share)
    assert np.array_equal(clip_ref.partials(grads + [np.zeros(0, f32)]), part)
    assert clip_ref.control(float("inf"), 1.0, 1, 1e-3, 0, 1, 1)[1:3] == (0.0, 0) and clip_ref.control(float("inf"), 1.0, 0, 1e-3, 0, 1, 1)[1:3] == (0.0, 1)
    assert np.isnan(clip_ref.control(float("nan"), 1.0, 0, 1e-3, 0, 1, 1)[1])
    for W in (1, 4, 1000):
        for t in range(1, W + 4):
            assert clip_ref.factor(clip_ref.LINEAR, W, t) == min(t / W, 1.0)
            assert clip_ref.factor(clip_ref.INV_SQRT, W, t) == (t / W if t <= W else (W / t) ** 0.5)
    assert clip_ref.control(0.0, 0.0, 0, 2e-4, clip_ref.LINEAR, 4, 4)[3] == f32(2e-4)


# ---- the class ---------------------------------------------------------------------------------------------------------
def _params():
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7))]


ALL_ON = dict(max_grad_norm=1.0, skip_nonfinite=True, warmup_steps=1000, schedule="inv_sqrt")


def test_class_refuses_bad_options_and_names_the_remedy():
    for kw, remedy in ((dict(max_grad_norm=0.0), "None"), (dict(max_grad_norm=-1.0), "None"), (dict(max_grad_norm=float("nan")), "None"),
                       (dict(warmup_steps=-1), "0 for no warmup"), (dict(warmup_steps=2.5), "0 for no warmup"),
                       (dict(schedule="cosine"), "inv_sqrt"), (dict(warmup_steps=10, schedule=None), "linear")):
        with pytest.raises(ValueError, match=remedy):
            hps.Adam(_params(), **kw)
    opt = hps.Adam(_params(), lr=1e-3, **ALL_ON)
    assert (opt.max_grad_norm, opt.skip_nonfinite, opt.warmup_steps, opt.schedule) == (1.0, True, 1000, "inv_sqrt")
    assert opt.grad_norm is None and opt.skipped_steps() == 0 and opt.current_lr() == 1e-3 and opt.steps_done() == 0
    assert opt.step() is None                                                           # no gradients: nothing to do
    for q in opt.param_groups[0]["params"]:
        q.grad = torch.zeros_like(q)
    with pytest.raises(RuntimeError, match="torch.optim.Adam"):                         # no CPU path, no quiet fall-back
        opt.step()
    opt.max_grad_norm = 0                                                                # options are read at every step
    with pytest.raises(ValueError, match="None"):
        opt.step()
    plain = hps.Adam(_params())
    assert (plain.max_grad_norm, plain.skip_nonfinite, plain.warmup_steps, plain.schedule) == (None, False, 0, "linear")
    assert plain.grad_norm is None and plain.skipped_steps() == 0


def test_state_dict_keeps_torch_adams_structure_with_every_option_on():
    ours, theirs = hps.Adam(_params(), lr=2e-4, weight_decay=1e-2, **ALL_ON), torch.optim.Adam(_params(), lr=2e-4, weight_decay=1e-2)
    a, b = ours.state_dict(), theirs.state_dict()
    assert a["param_groups"] == b["param_groups"] and list(a["param_groups"][0]) == list(b["param_groups"][0])
    assert a["state"] == b["state"] == {} and list(a) == list(b)
    assert not set(ALL_ON) & (set(ours.defaults) | set(ours.param_groups[0]))
    for q in theirs.param_groups[0]["params"]:
        q.grad = torch.ones_like(q)
    for _ in range(3):
        theirs.step()
    b = theirs.state_dict()
    ours.load_state_dict(b)                                                             # --resume across the classes
    a = ours.state_dict()
    assert a["param_groups"] == b["param_groups"] and a["state"].keys() == b["state"].keys()
    for i in b["state"]:
        assert list(a["state"][i]) == list(b["state"][i]) == ["step", "exp_avg", "exp_avg_sq"]
        for key in b["state"][i]:
            assert torch.equal(a["state"][i][key], b["state"][i][key]), (i, key)
    assert ours.steps_done() == 3 and ours.max_grad_norm == 1.0 and ours.warmup_steps == 1000
    theirs.load_state_dict(a)
    theirs.step()
    assert float(theirs.state_dict()["state"][0]["step"]) == 4.0


def test_graph_trainer_keys_the_four_options():
    src = open(os.path.join(ROOT, "hand_pose_sl_amd", "graph_trainer.py")).read()
    key = src[src.index("def _graph_key"):src.index("def _reset")]
    for name in ("max_grad_norm", "skip_nonfinite", "warmup_steps", "schedule"):
        assert "optimizer." + name in key, name
