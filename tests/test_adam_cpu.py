"""The native Adam (b2h_adam_step, kernel_adam.h, hand_pose_sl_amd.Adam) without a GPU: the entry point declared, typed
and exported; every refusal, which launches nothing, and the no-op cases; the kernel compiles for gfx950 without scratch,
spills or LDS (its register counts are printed: pytest -s; DESIGN.md section 21 quotes them); the numpy restatements
(adam_ref.py) against torch.optim.Adam(foreach=False) on the CPU over 10 steps at the issue's bar; the class's refusals
and the structure of its state_dict; the C host that trains compiles and links libb2h alone."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import adam_ref
import hand_pose_sl_amd as hps
from conftest import ROOT
from hand_pose_sl_amd import _lib
from hand_pose_sl_amd import build as b2h_build
from kernel_remarks import kernel_remarks


def test_entry_point_declared_typed_and_exported():
    header = " ".join(open(os.path.join(ROOT, "include", "b2h.h")).read().split())
    decl = ("int b2h_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* "
            "exp_avg_sq, const int64_t* numel, int n_tensors, float lr, const float* lr_dev, float beta1, float beta2, "
            "float eps, float weight_decay, int64_t step, const int64_t* step_dev, void* stream);")
    assert decl in header
    assert header.count("an optimizer may update the tensors in place between launches.") == 1     # replaced nothing
    assert header.count("b2h_adam_step below is that optimizer") == 3
    vp, f = ctypes.c_void_p, ctypes.c_float
    assert _lib.SYMBOLS["b2h_adam_step"] == (ctypes.c_int, [ctypes.POINTER(vp)] * 4 + [
        ctypes.POINTER(ctypes.c_int64), ctypes.c_int, f, vp, f, f, f, f, ctypes.c_int64, vp, vp])
    _lib.load()                                          # types every symbol: a missing export raises here
    assert hps.Adam is __import__("hand_pose_sl_amd.optim", fromlist=["Adam"]).Adam and "Adam" in hps.__all__


def _call(lib, p=(0x10000,), g=(0x20000,), m=(0x30000,), v=(0x40000,), sizes=(16,), n=None, lr=1e-3, lr_dev=None, b1=0.9,
          b2=0.999, eps=1e-8, wd=0.0, step=1, step_dev=None):
    arr = [None if a is None else (ctypes.c_void_p * len(a))(*a) for a in (p, g, m, v)]
    numel = None if sizes is None else (ctypes.c_int64 * len(sizes))(*sizes)
    n = len(sizes) if n is None else n
    return lib.b2h_adam_step(*arr, numel, n, lr, lr_dev, b1, b2, eps, wd, step, step_dev, None)


def test_refusals_launch_nothing_and_no_ops_return_ok():
    """No GPU here: a call that reached a launch would fail with another status (B2H_ERR_HIP), so ERR_INVALID with a
    message shows the refusal came first; the pointers are made-up addresses that nothing dereferences."""
    lib = _lib.load()
    nan, word = float("nan"), 0x50000
    refused = {
        "NULL params": lambda: _call(lib, p=None),
        "NULL grads": lambda: _call(lib, g=None),
        "NULL exp_avg": lambda: _call(lib, m=None),
        "NULL exp_avg_sq": lambda: _call(lib, v=None),
        "NULL numel": lambda: _call(lib, sizes=None, n=1),
        "n_tensors < 0": lambda: _call(lib, n=-1),
        "NULL pointer of a tensor": lambda: _call(lib, p=(0x10000, None), g=(0x20000, 0x21000), m=(0x30000, 0x31000),
                                                  v=(0x40000, 0x41000), sizes=(16, 16)),
        "NULL gradient": lambda: _call(lib, g=(None,)),
        "misaligned by 2": lambda: _call(lib, m=(0x30002,)),
        "misaligned by 1, 90th of 90": lambda: _call(lib, p=[0x10000 + 64 * i for i in range(90)],
                                                     g=[0x20000 + 64 * i for i in range(90)],
                                                     m=[0x30000 + 64 * i for i in range(90)],
                                                     v=[0x40000 + 64 * i for i in range(89)] + [0x48001], sizes=[16] * 90),
        "numel < 0": lambda: _call(lib, sizes=(-1,)),
        "beta1 = 1": lambda: _call(lib, b1=1.0),
        "beta1 < 0": lambda: _call(lib, b1=-0.1),
        "beta2 = 1": lambda: _call(lib, b2=1.0),
        "beta2 NaN": lambda: _call(lib, b2=nan),
        "beta1 NaN": lambda: _call(lib, b1=nan),
        "eps < 0": lambda: _call(lib, eps=-1e-8),
        "eps NaN": lambda: _call(lib, eps=nan),
        "weight_decay < 0": lambda: _call(lib, wd=-1e-2),
        "weight_decay NaN": lambda: _call(lib, wd=nan),
        "lr < 0": lambda: _call(lib, lr=-1e-3),
        "lr NaN": lambda: _call(lib, lr=nan),
        "step 0 without step_dev": lambda: _call(lib, step=0),
        "step < 0 with step_dev": lambda: _call(lib, step=-1, step_dev=word),
        "p overlaps m": lambda: _call(lib, m=(0x10000 + 60,)),
        "p overlaps v": lambda: _call(lib, v=(0x10000 - 60,)),
        "m overlaps v": lambda: _call(lib, v=(0x30000 + 32,)),
        "p is g": lambda: _call(lib, g=(0x10000,)),
        "m overlaps g": lambda: _call(lib, g=(0x30000 + 4,)),
        "v overlaps g": lambda: _call(lib, g=(0x40000 - 4,)),
        "bad beta with nothing to update": lambda: _call(lib, sizes=(0,), b1=2.0),
    }
    for what, call in refused.items():
        assert call() == _lib.ERR_INVALID, what
        assert _lib.last_error(), what
        with pytest.raises(ValueError):
            _lib.check(call())
    assert lib.b2h_adam_step(None, None, None, None, None, 0, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 1, None, None) == _lib.OK
    assert _call(lib, sizes=(0,)) == _lib.OK                                              # all sizes 0
    assert _call(lib, p=(None,), g=(None,), m=(None,), v=(0x3,), sizes=(0,)) == _lib.OK   # an empty tensor's pointers
    assert _call(lib, sizes=(0,), lr=-1.0, lr_dev=word, step=0, step_dev=word) == _lib.OK # lr ignored beside lr_dev
    assert _call(lib, p=[0x10000] * 200, g=[0x10000] * 200, m=[0x10000] * 200, v=[0x10000] * 200, sizes=[0] * 200) == _lib.OK


def test_kernel_has_no_scratch_spills_or_lds():
    kernels, listing = kernel_remarks()
    new = {n: res for n, res in kernels.items() if "b2h_adam_step_k" in n}
    assert len(new) == 1, sorted(new)
    for name, res in new.items():
        print(name, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "occupancy", res["Occupancy [waves/SIMD]"])
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)
    text = open(listing).read()
    body = text[text.index("b2h_adam_step_kENS_6AdArgsE:"):]
    body = body[:body.index("s_endpgm")]
    # the whole chunks: four 16-byte loads (g, m, v, p) and three 16-byte stores (p, m, v); the dword path: four loads
    # and three stores; no atomics; IEEE division (v_div_fixup_f32), never a bare reciprocal
    assert len(re.findall(r"\bglobal_load_dwordx4\b", body)) == 4 and len(re.findall(r"\bglobal_store_dwordx4\b", body)) == 3
    assert len(re.findall(r"\bglobal_load_dword\b", body)) == 4 and len(re.findall(r"\bglobal_store_dword\b", body)) == 3
    assert "atomic" not in body and len(re.findall(r"\bv_div_fixup_f32\b", body)) == 10


# ---- the restatements against torch on the CPU -----------------------------------------------------------------------
# The arithmetic is elementwise, so the tensor sizes of the GPU test (which are about the kernel's indexing) play no
# part here: every case runs on one flat array.
N_CPU = 2 ** 16


def _grad_scale(j):
    return np.float32(1 + j / 8)                          # the same gradient, growing: exp_avg keeps its sign


def _ten_steps(fn, p, g, m, v, t, lr, wd):
    for j in range(10):
        p, m, v = fn(p, g * _grad_scale(j), m, v, t + j, lr, wd=wd)
    return p, m, v


def test_restatements_match_torch_on_the_cpu_over_ten_steps():
    ref, rows = [0.0] * 3, []
    for i, (t, k, wd, lr) in enumerate(adam_ref.cases()):
        p, g, m, v = adam_ref.inputs(N_CPU, t, k, wd, 500 + i)
        want = _ten_steps(adam_ref.truth, p, g, m, v, t, lr, wd)
        got_torch = adam_ref.torch_adam_step(p, g, m, v, t, lr, wd, steps=10, grad_scale=_grad_scale)
        got_32 = _ten_steps(adam_ref.restate32, p, g, m, v, t, lr, wd)
        e_torch = [adam_ref.ulp_error(a, b) for a, b in zip(got_torch, want)]
        rows.append(((t, k, wd, lr), [adam_ref.ulp_error(a, b) for a, b in zip(got_32, want)]))
        ref = [max(a, b) for a, b in zip(ref, e_torch)]
    print("\ntorch.optim.Adam(foreach=False) on the CPU, max ulp error of (p, m, v):", ["%.2f" % e for e in ref])
    print("fp32 restatement, max ulp error of (p, m, v):", ["%.2f" % max(r[1][q] for r in rows) for q in range(3)])
    assert all(np.isfinite(ref)) and max(ref) < 64        # the precondition: the reference's own error is bounded
    for case, errs in rows:
        for name, e, r in zip("pmv", errs, ref):
            assert e <= adam_ref.bar(r), f"{case} {name}: restatement {e:.2f} ulp > 2 * {r:.2f} + 1"


def test_hyper_parameters_of_the_restatement():
    assert adam_ref.pow_sq(0.999, 1) == 0.999 and adam_ref.pow_sq(0.9, 2) == 0.9 * 0.9 and adam_ref.pow_sq(0.5, 0) == 1.0
    for t in adam_ref.STEPS + [7, 12345]:                # by squaring against Python's pow: the same float
        for b in (0.9, 0.999):
            assert np.float32((1 - adam_ref.pow_sq(b, t)) ** 0.5) == np.float32((1 - b ** t) ** 0.5), (b, t)
            assert np.float32(2e-4 / (1 - adam_ref.pow_sq(b, t))) == np.float32(2e-4 / (1 - b ** t)), (b, t)


# ---- the class ---------------------------------------------------------------------------------------------------------
def _params():
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7))]


def test_class_refuses_what_it_does_not_do():
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError, match="torch.optim.Adam"):
            hps.Adam(_params(), **kw)
    a, b = _params()
    for bad in ([{"params": [a]}, {"params": [b], "lr": 1e-2}], [{"params": [a]}, {"params": [b], "betas": (0.8, 0.999)}],
                [{"params": [a], "weight_decay": 0.1}, {"params": [b]}], [{"params": [a]}, {"params": [b], "eps": 1e-6}]):
        with pytest.raises(ValueError, match="torch.optim.Adam"):
            hps.Adam(bad, lr=1e-3)
    hps.Adam([{"params": [a]}, {"params": [b]}], lr=1e-3)                               # equal groups are fine
    with pytest.raises(ValueError, match="torch.optim.Adam"):
        hps.Adam([torch.nn.Parameter(torch.randn(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="torch.optim.Adam"):
        hps.Adam([torch.nn.Parameter(torch.randn(4, 6).t())])                           # not contiguous
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=-1.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            hps.Adam(_params(), **kw)
    opt = hps.Adam(_params(), lr=1e-3)
    with pytest.raises(ValueError, match="torch.optim.Adam"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.randn(2))], "lr": 0.5})
    opt = hps.Adam(_params(), lr=1e-3)
    assert opt.step() is None                                                           # no gradients: nothing to do
    for q in opt.param_groups[0]["params"]:
        q.grad = torch.zeros_like(q)
    with pytest.raises(RuntimeError, match="torch.optim.Adam"):                         # no CPU path, no quiet fall-back
        opt.step()


def test_state_dict_has_torch_adams_structure():
    ours, theirs = hps.Adam(_params(), lr=2e-4, weight_decay=1e-2), torch.optim.Adam(_params(), lr=2e-4, weight_decay=1e-2)
    assert isinstance(ours, torch.optim.Optimizer)
    a, b = ours.state_dict(), theirs.state_dict()
    assert a["param_groups"] == b["param_groups"] and a["state"] == b["state"] == {}
    # a state as torch leaves it after 3 steps, loaded and given back
    for q in theirs.param_groups[0]["params"]:
        q.grad = torch.ones_like(q)
    for _ in range(3):
        theirs.step()
    b = theirs.state_dict()
    ours.load_state_dict(b)
    a = ours.state_dict()
    assert a["param_groups"] == b["param_groups"] and a["state"].keys() == b["state"].keys()
    for i in b["state"]:
        assert list(a["state"][i]) == list(b["state"][i]) == ["step", "exp_avg", "exp_avg_sq"]
        for key in b["state"][i]:
            x, y = a["state"][i][key], b["state"][i][key]
            assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device and torch.equal(x, y), (i, key)
    assert ours.steps_done() == 3
    theirs.load_state_dict(a)                                                           # and back into torch's
    theirs.step()
    assert float(theirs.state_dict()["state"][0]["step"]) == 4.0
    # one step count for all: a state with two is refused
    b["state"][1]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="torch.optim.Adam"):
        hps.Adam(_params(), lr=2e-4, weight_decay=1e-2).load_state_dict(b)


# ---- the C host that trains ------------------------------------------------------------------------------------------
def test_training_host_compiles_and_links_libb2h_alone():
    import c_train_host
    exe = c_train_host.compile_host()
    assert os.access(exe, os.X_OK)
    needed = subprocess.check_output(["readelf", "-d", exe]).decode()
    assert "libb2h.so" in needed and "torch" not in needed and "python" not in needed.lower()
    assert os.path.getmtime(exe) >= os.path.getmtime(b2h_build.build())
