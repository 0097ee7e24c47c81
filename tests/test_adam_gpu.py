"""The native Adam on the MI355X: b2h_adam_step (kernel_adam.h) against the float64 truth of adam_ref.py at the issue's
bar -- at most 2 x the largest error of torch.optim.Adam(foreach=False) on the same GPU over the same cases + 1 ulp --
between NaN guard bands, aligned and with every pointer off the 16-byte grid; grouping into launches and grid passes; the
step and the learning rate as device words; `hand_pose_sl_amd.Adam` as a drop-in on the three models with state_dicts
crossing to torch.optim.Adam and back; the reference's loop with it; a captured training step; the C host that trains."""
import ctypes
import functools
import subprocess
import warnings

import numpy as np
import pytest
import torch

import adam_ref
import hand_pose_sl_amd as hps
import tenc_train_ref
import test_tpt_train_long_gpu as long_gpu
from hand_pose_sl_amd import _lib
from tpt_train_ref import recipe_state, train_model
from train_ref import KEYS, assert_within_bar, load_train

pytestmark = pytest.mark.gpu
GUARD = 32                                # floats of NaN on either side of every tensor
NAN_WORD = 0x7FC5A5A5
GRID_THREADS = 256 * 1024                 # kAdThreads * kAdMaxBlocks of kernel_adam.h: one grid pass of 16-byte chunks
N_TOKENS = 50
f32 = np.float32


# ---- one b2h_adam_step call between guard bands -------------------------------------------------------------------
def _place(sizes, mode, which):
    """The first float of every tensor in one buffer: GUARD floats of NaN before and after each; "aligned" puts every
    start on the 16-byte grid, "offset" 4, 8 or 12 bytes past it, another one for each of p, g, m, v of a tensor."""
    starts, total = [], 0
    for i, n in enumerate(sizes):
        start = total + GUARD + (1 + (i + which) % 3 if mode == "offset" else 0)
        starts.append(start)
        total = (start + n + GUARD + 3) // 4 * 4
    return starts, max(total, 4)


def _native(dev, tensors, lr, wd, step, mode="aligned", step_word=None, lr_word=None):
    """`tensors`: [(p, g, m, v)] float32 arrays.  One call on all of them; checks that every guard word and all of g
    kept their bits and that the device words were only read; returns [(p, m, v)] as updated."""
    sizes = [t[0].size for t in tensors]
    hosts, starts = [], []
    for which in range(4):
        s, total = _place(sizes, mode, which)
        h = np.full(total, NAN_WORD, np.uint32)
        for t, a in zip(tensors, s):
            h[a:a + t[which].size] = np.ascontiguousarray(t[which], f32).view(np.uint32)
        hosts.append(h)
        starts.append(s)
    bufs = [torch.from_numpy(h.view(np.int32)).to(dev) for h in hosts]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    n = len(sizes)
    # an empty tensor's pointers are never looked at: NULL for every other one
    ptrs = [(ctypes.c_void_p * n)(*[None if sizes[i] == 0 and i % 2 else b.data_ptr() + 4 * s[i] for i in range(n)])
            for b, s in zip(bufs, starts)]
    sw = None if step_word is None else torch.tensor([step_word], dtype=torch.int64, device=dev)
    lw = None if lr_word is None else torch.tensor([lr_word], dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.load().b2h_adam_step(ptrs[0], ptrs[1], ptrs[2], ptrs[3], (ctypes.c_int64 * n)(*sizes), n, lr,
                                         None if lw is None else ctypes.c_void_p(lw.data_ptr()), adam_ref.B1, adam_ref.B2,
                                         adam_ref.EPS, wd, step, None if sw is None else ctypes.c_void_p(sw.data_ptr()),
                                         ctypes.c_void_p(st)))
    outs = [b.cpu().numpy().view(np.uint32) for b in bufs]
    assert sw is None or int(sw.item()) == step_word                  # read, never written
    assert lw is None or lw.cpu().numpy()[0] == f32(lr_word)
    assert np.array_equal(outs[1], hosts[1]), "a gradient or one of its guards was written"
    for which in (0, 2, 3):
        guard = np.ones(outs[which].shape, bool)
        for a, size in zip(starts[which], sizes):
            guard[a:a + size] = False
        assert (outs[which][guard] == NAN_WORD).all(), "a guard word was written"
    return [tuple(outs[w][starts[w][i]:starts[w][i] + sizes[i]].view(f32).copy() for w in (0, 2, 3)) for i in range(n)]


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for s, t in zip(a, b) for x, y in zip(s, t))


def _random_tensors(sizes, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [((rng.standard_normal(n)).astype(f32), (rng.standard_normal(n) * scale).astype(f32),
             (rng.standard_normal(n) * scale).astype(f32), (rng.uniform(0, 2, n) * scale * scale).astype(f32)) for n in sizes]


# ---- 1. the kernel against the truth, at the bar ----------------------------------------------------------------------
SIZES_WITH_EMPTIES = [n for i, size in enumerate(adam_ref.SIZES) for n in ([size, 0] if i % 3 == 0 else [size])]


def _split(arrays):
    out, at = [], 0
    for n in SIZES_WITH_EMPTIES:
        out.append(tuple(a[at:at + n] for a in arrays))
        at += n
    return out


@functools.lru_cache(maxsize=None)
def _survey():
    """Every case of adam_ref.cases() once (shared: leave unchanged): the ulp errors against the float64 truth of
    torch.optim.Adam(foreach=False) on this GPU and of the kernel, whether the aligned and the offset layout gave the same
    bits, and how many elements differ from the fp32 restatement."""
    dev = torch.device("cuda:0")
    n, rows = sum(adam_ref.SIZES), {}
    for i, (t, k, wd, lr) in enumerate(adam_ref.cases()):
        p, g, m, v = adam_ref.inputs(n, t, k, wd, 100 + i)
        tensors = _split((p, g, m, v))
        aligned = _native(dev, tensors, lr, wd, t)
        offset = _native(dev, tensors, lr, wd, t, mode="offset")
        got = [np.concatenate([a[q] for a in aligned]) for q in range(3)]
        want = adam_ref.truth(p, g, m, v, t, lr, wd=wd)
        ref = adam_ref.torch_adam_step(p, g, m, v, t, lr, wd, device=dev)
        unlike = None
        if k == 0:
            unlike = [int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in
                      zip(got, adam_ref.restate32(p, g, m, v, t, lr, wd=wd))]
        rows[(t, k, wd, lr)] = dict(native=[adam_ref.ulp_error(a, b) for a, b in zip(got, want)],
                                    torch=[adam_ref.ulp_error(a, b) for a, b in zip(ref, want)],
                                    same_bits=_same_bits(aligned, offset), unlike_restatement=unlike,
                                    unlike_torch=[int((a != b).sum()) for a, b in zip(got, ref)])
    return rows


def _reference_max():
    return [max(r["torch"][q] for r in _survey().values()) for q in range(3)]


def test_reference_is_bounded_on_the_cases(cuda_device):
    ref = _reference_max()
    print("\ntorch.optim.Adam(foreach=False) on the GPU, max ulp error of (p, m, v):", ["%.2f" % e for e in ref])
    assert all(np.isfinite(ref)) and max(ref) < 64


@pytest.mark.parametrize("t", adam_ref.STEPS)
def test_kernel_within_the_bar_of_the_reference(t, cuda_device):
    ref = _reference_max()
    for case, r in _survey().items():
        if case[0] != t:
            continue
        print(f"\n{case}: native {['%.2f' % e for e in r['native']]} torch {['%.2f' % e for e in r['torch']]} ulp (p, m, v); "
              f"elements unlike torch {r['unlike_torch']}, unlike the restatement {r['unlike_restatement']}")
        assert r["same_bits"], f"{case}: the 16-byte path and the dword path differ"
        for name, e, top in zip("pmv", r["native"], ref):
            assert e <= adam_ref.bar(top), f"{case} {name}: {e:.2f} ulp > 2 * {top:.2f} + 1"


# ---- 2. grouping: more tensors than a launch holds, more chunks than a grid pass ------------------------------------
def test_result_does_not_depend_on_grouping(cuda_device):
    sizes = [(37 * i) % 53 for i in range(300)]           # 300 tensors: four launches of 80, 80, 80 and 60
    sizes[7], sizes[79], sizes[80], sizes[150], sizes[299] = 4099, 1025, 257, 65537, 1023
    assert sizes.count(0) >= 5
    tensors = _random_tensors(sizes, 7)
    together = _native(cuda_device, tensors, 1e-3, 1e-2, 3, mode="offset")
    alone = [_native(cuda_device, [t], 1e-3, 1e-2, 3)[0] for t in tensors]
    assert _same_bits(together, alone)
    assert _same_bits(_native(cuda_device, tensors[:80], 1e-3, 1e-2, 3), alone[:80])      # exactly one full launch
    assert _same_bits(_native(cuda_device, tensors[:81], 1e-3, 1e-2, 3), alone[:81])


def test_more_chunks_than_the_grid_has_threads(cuda_device):
    """2.5 grid passes of chunks with a tensor boundary inside a pass; the last pass is partial."""
    sizes = [4 * GRID_THREADS + 21, 5, 4 * GRID_THREADS * 3 // 2 - 7]
    tensors = _random_tensors(sizes, 8, scale=1e-3)
    together = _native(cuda_device, tensors, 2e-4, 0.0, 1000)
    assert _same_bits(together, [_native(cuda_device, [t], 2e-4, 0.0, 1000)[0] for t in tensors])
    want = adam_ref.truth(*[np.concatenate([t[q] for t in tensors]) for q in range(4)], 1000, 2e-4)
    got = [np.concatenate([t[q] for t in together]) for q in range(3)]
    assert np.isfinite(got).all() and float(np.abs(got[0] - want[0]).max()) <= 1e-6


# ---- 3. the step and the learning rate as device words --------------------------------------------------------------
def test_step_and_lr_on_the_device(cuda_device):
    tensors = _random_tensors(adam_ref.SIZES[:17], 9)
    for t in (1, 2, 7, 999, 1000):
        by_value = _native(cuda_device, tensors, 2e-4, 1e-2, t, mode="offset")
        assert _same_bits(by_value, _native(cuda_device, tensors, 2e-4, 1e-2, 1, mode="offset", step_word=t - 1)), t
        assert _same_bits(by_value, _native(cuda_device, tensors, 2e-4, 1e-2, 0, mode="offset", step_word=t)), t
        assert _same_bits(by_value, _native(cuda_device, tensors, 7.0, 1e-2, t, mode="offset", lr_word=2e-4)), t
        assert _same_bits(by_value, _native(cuda_device, tensors, 7.0, 1e-2, 1, step_word=t - 1, lr_word=2e-4)), t
    assert not _same_bits(_native(cuda_device, tensors, 2e-4, 1e-2, 2), _native(cuda_device, tensors, 2e-4, 1e-2, 1, step_word=2))
    assert not _same_bits(_native(cuda_device, tensors, 2e-4, 1e-2, 2), _native(cuda_device, tensors, 2e-4, 1e-2, 2, lr_word=1e-3))


# ---- 4. drop-in on the three models, state_dicts across the two classes ---------------------------------------------
# The parameters are moved half a unit away from zero: the bar's unit is the ulp at the truth's value, and a parameter
# within a few updates of zero lands on a result much smaller than its operands, where torch's own error in that unit
# is unbounded (thousands of ulp on the models' own initial weights, measured on the CPU).  This is the precondition of
# the bar, kept here as adam_ref.inputs keeps it in test 1; the models, shapes and gradients are the models' own.
def _conv(dev):
    torch.manual_seed(11)
    m = hps.ConvModel(30, "ReLU", False)
    x, dy = torch.randn((3, 9, 12, 2)), torch.randn((3, 9, 21, 2))
    return m, lambda mm: mm(x.to(dev)).backward(dy.to(dev))


def _tenc(dev):
    m = hps.TransformerEnc(24, 4, 128, 42, 2, dropout=0.0)
    m.load_state_dict(tenc_train_ref.seeded_state(2, 31))
    g = torch.Generator().manual_seed(3100)
    x, dy = torch.randn((2, 9, 12, 2), generator=g), torch.randn((2, 9, 21, 2), generator=g)
    return m, lambda mm: mm(x.to(dev)).backward(dy.to(dev))


def _tpt(dev):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        m = train_model(recipe_state(40, N_TOKENS, 1, 1), 0.0)
    tok, x, dy = long_gpu._data(2, 7, 15, N_TOKENS, 7015)
    return m, lambda mm: mm(tok.to(dev), x.to(dev)).backward(dy.to(dev))


def _flat(tensors):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in tensors]) if tensors else np.zeros(0, f32)


def _checked_step(opt, t, lr, what):
    """opt.step() on parameters that all have gradients; the ulp errors of (p, m, v) against the float64 truth."""
    params = [q for g in opt.param_groups for q in g["params"] if q.grad is not None]
    before = [_flat(params), _flat([q.grad for q in params])]
    for key in ("exp_avg", "exp_avg_sq"):
        before.append(_flat([opt.state[q][key] for q in params]) if t > 1 else np.zeros_like(before[0]))
    assert all(np.isfinite(a).all() for a in before), what
    opt.step()
    want = adam_ref.truth(*before, t, lr)
    got = [_flat(params), _flat([opt.state[q]["exp_avg"] for q in params]), _flat([opt.state[q]["exp_avg_sq"] for q in params])]
    errs = [adam_ref.ulp_error(a, b) for a, b in zip(got, want)]
    print(f"\n{what}, step {t}: {['%.2f' % e for e in errs]} ulp (p, m, v) over {before[0].size} elements")
    return errs


@pytest.mark.parametrize("make", [_conv, _tenc, _tpt], ids=["ConvModel", "TransformerEnc", "TextPoseTransformer"])
def test_drop_in_and_state_dicts_across_the_classes(make, cuda_device):
    lr, ref = 2e-4, _reference_max()
    a, backward = make(cuda_device)
    b, _ = make(cuda_device)
    b.load_state_dict(a.state_dict())
    for m in (a, b):
        m.to(cuda_device).train()
        with torch.no_grad():
            for q in m.parameters():
                q.add_(torch.where(q >= 0, 0.5, -0.5))
    backward(a)
    for qa, qb in zip(a.parameters(), b.parameters()):
        assert torch.equal(qa, qb)
        qb.grad = None if qa.grad is None else qa.grad.clone()
    native, theirs = hps.Adam(a.parameters(), lr=lr), torch.optim.Adam(b.parameters(), lr=lr, foreach=False)
    versions = [q._version for q in a.parameters()]
    e_native = _checked_step(native, 1, lr, "hand_pose_sl_amd.Adam")
    _checked_step(theirs, 1, lr, "torch.optim.Adam")
    assert all(q._version > v for q, v in zip(a.parameters(), versions) if q.grad is not None)
    for name, e, top in zip("pmv", e_native, ref):
        assert e <= adam_ref.bar(top), f"{name}: {e:.2f} ulp > 2 * {top:.2f} + 1"
    # across: torch's state into the native class on b, the native state into torch's class on a
    sd_native, sd_theirs = native.state_dict(), theirs.state_dict()
    for ga, gb in zip(sd_native["param_groups"], sd_theirs["param_groups"]):       # the twin asked for foreach=False
        assert list(ga) == list(gb) and {**ga, "foreach": None} == {**gb, "foreach": None}
    assert len(sd_native["param_groups"]) == len(sd_theirs["param_groups"]) and sd_native["state"].keys() == sd_theirs["state"].keys()
    for i in sd_theirs["state"]:
        assert list(sd_native["state"][i]) == list(sd_theirs["state"][i]) and float(sd_native["state"][i]["step"]) == 1.0
    native_b, theirs_a = hps.Adam(b.parameters(), lr=lr), torch.optim.Adam(a.parameters(), lr=lr, foreach=False)
    native_b.load_state_dict(sd_theirs)
    theirs_a.load_state_dict(sd_native)
    # the continued step meets the first step's gradients again, so exp_avg keeps the sign of what it meets (the bar's
    # precondition, adam_ref.py): these models' gradients after one step flip sign in places, and there torch's own
    # exp_avg is off by 10^4 ulp at the truth's value, bit for bit as the kernel's
    for qa, qb in zip(a.parameters(), b.parameters()):
        assert (qa.grad is None and qb.grad is None) or torch.equal(qa.grad, qb.grad)
    e_native = _checked_step(native_b, 2, lr, "hand_pose_sl_amd.Adam continuing torch's state")
    _checked_step(theirs_a, 2, lr, "torch.optim.Adam continuing the native state")
    for name, e, top in zip("pmv", e_native, ref):
        assert e <= adam_ref.bar(top), f"continued {name}: {e:.2f} ulp > 2 * {top:.2f} + 1"
    assert native_b.steps_done() == 2 and all(float(s["step"]) == 2.0 for s in theirs_a.state_dict()["state"].values())
    assert all(float(s["step"]) == 2.0 for s in native_b.state_dict()["state"].values())
    # a parameter that gets a gradient only later is refused: one step count for all
    extra = torch.nn.Parameter(torch.ones(4, device=cuda_device))
    native_b.add_param_group({"params": [extra]})
    extra.grad = torch.ones_like(extra)
    with pytest.raises(RuntimeError, match="torch.optim.Adam"):
        native_b.step()


# ---- 5. the reference's loop with the native optimizer ---------------------------------------------------------------
def test_adam_trajectory_and_inference_after_updates_with_native_adam(cuda_device):
    """The body of test_train_gpu.test_adam_trajectory_and_inference_after_updates with hps.Adam in torch.optim.Adam's place."""
    r = load_train("traj_c30_b4_t64")
    m = hps.ConvModel(r["C"], "ReLU", False)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in r["state"].items()})
    m = m.to(cuda_device).eval()
    with torch.no_grad():
        m(torch.from_numpy(r["x"]).to(cuda_device))           # packs the initial weights (inference path)
    m.train()
    opt = hps.Adam(m.parameters(), lr=float(r["lr"]))
    criterion = hps.maskedPoseL1()
    x, t = torch.from_numpy(r["x"]).to(cuda_device), torch.from_numpy(r["target"]).to(cuda_device)
    lengths = [int(n) for n in r["lengths"]]
    losses = []
    for _ in range(int(r["steps"])):                          # traintest.py:94-121
        prediction = m(x)
        for i, n in enumerate(lengths):
            prediction[i, n:, :] = 0
        loss = criterion(prediction, t, lengths)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert opt.steps_done() == int(r["steps"])
    assert_within_bar(np.array(losses), r["losses64"], np.abs(r["losses32"] - r["losses64"]).max(), "losses")
    sd = m.state_dict()
    for k in KEYS:
        key = k.replace(".", "_")
        a, b = r["final64_" + key], r["final32_" + key].astype(np.float64)
        assert_within_bar(sd[k].cpu().double().numpy(), a, np.abs(b - a).max(), "final " + k)
    # the inference path repacks after the native updates: this fails without the version bump of Adam.step
    from oracle.torch_port import torch_forward
    m.eval()
    with torch.no_grad():
        y = m(x).cpu()
    ref = torch_forward(x.cpu(), {k: v.cpu() for k, v in sd.items()})
    assert float((y - ref).abs().max()) <= 2e-5


# ---- 6. a captured training step ---------------------------------------------------------------------------------------
def test_captured_step_with_native_dropout_and_adam_equals_eager(cuda_device):
    B, S, T, lr, lr2 = 2, 7, 15, 1e-3, 2.5e-4
    state = recipe_state(90, N_TOKENS, 1, 1)
    tok, x, target = (t.to(cuda_device) for t in long_gpu._data(B, S, T, N_TOKENS, 91))
    lengths = torch.tensor([T, T - 4], dtype=torch.int64, device=cuda_device)

    def make():
        m = train_model(state, 0.1, cuda_device).set_dropout_source("native", seed=5)
        return m, hps.Adam(m.parameters(), lr=lr, weight_decay=1e-2)

    def one_step(m, opt):
        opt.zero_grad(set_to_none=True)
        hps.masked_pose_l1(m(tok, x), target, lengths).backward()
        opt.step()

    m, opt = make()
    s = torch.cuda.Stream(cuda_device)                      # warm-up on a side stream, as torch's docs do: step 1
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        one_step(m, opt)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    assert opt.steps_done() == 1
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):                           # one stream: no parallel branches
        hps.masked_pose_l1(m(tok, x), target, lengths).backward()
        opt.step()
    assert opt.steps_done() == 1                            # capturing ran nothing
    graph.replay()
    graph.replay()
    assert opt.steps_done() == 3
    opt.set_lr(lr2)                                         # between replays: the next one steps with the new rate
    graph.replay()
    torch.cuda.synchronize()
    assert opt.steps_done() == 4 and opt._lr_word.cpu().numpy()[0] == f32(lr2) and opt.param_groups[0]["lr"] == lr2
    twin, twin_opt = make()
    for i in range(4):
        if i == 3:
            twin_opt.param_groups[0]["lr"] = lr2            # an eager step reads param_groups itself
        one_step(twin, twin_opt)
    assert twin_opt.steps_done() == 4
    for a, b in zip(m.parameters(), twin.parameters()):
        assert torch.equal(a, b)
    for key in ("exp_avg", "exp_avg_sq"):
        for a, b in zip(m.parameters(), twin.parameters()):
            assert torch.equal(opt.state[a][key], twin_opt.state[b][key])
    # the rate did change the fourth step: the same four steps at lr throughout end elsewhere
    same, same_opt = make()
    for _ in range(4):
        one_step(same, same_opt)
    assert any(not torch.equal(a, b) for a, b in zip(m.parameters(), same.parameters()))


# ---- 7. the C host that trains -----------------------------------------------------------------------------------------
def test_c_host_trains_the_trajectory(tmp_path, cuda_device):
    import c_train_host
    exe = c_train_host.compile_host()
    r = load_train("traj_c30_b4_t64")
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    c_train_host.write_input(inp, r)
    run = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    losses, final = c_train_host.read_output(out, r)
    assert_within_bar(losses.astype(np.float64), r["losses64"], np.abs(r["losses32"] - r["losses64"]).max(), "losses")
    for k in KEYS:
        key = k.replace(".", "_")
        a, b = r["final64_" + key], r["final32_" + key].astype(np.float64)
        assert_within_bar(final[k].astype(np.float64), a, np.abs(b - a).max(), "final " + k)
    # a truncated input is an error, not a run on garbage
    short = tmp_path / "short.bin"
    short.write_bytes(inp.read_bytes()[:-8])
    assert subprocess.run([exe, str(short), str(out)], capture_output=True, timeout=120).returncode != 0
