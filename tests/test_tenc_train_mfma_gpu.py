"""TransformerEnc training on the fp32 MFMA routes on the MI355X: `model.set_train_kernels("mfma")` (b2h_mw_sdpa,
b2h_mw_sdpa_bwd of kernel_train_attn_whole_mfma.h) and `model.set_train_linear("mfma")` (b2h_ml_linear, _dx, _dw of
kernel_train_linear_mfma.h).

The bars are test_tenc_train_gpu.py's own, unchanged: per tensor max|g - g64| <= 4 * max|g32_ref - g64| +
1e-6 * max|g64| and y within 2e-5, against float64 autograd of tenc_train_ref.port_forward with the masks the kernels
used.  That module's helpers, and those of its tests that the routes have to pass unchanged, run here with its `_model`
replaced by one that switches the model and its handle (the `mw` fixture); every model built that way is checked to
have resolved to the kernels asked for.  Shapes: T on both sides of every multiple of 16 (a tile) and of 64 (a lane's
second key), T = 0 .. 3 mod 4 (the k-step), one row, and the tile-aligned maximum 128.

Bit-equality, as built: the MFMA Linears equal the default in every bit; the MFMA attention's
forward keeps the default's chains, so y is bit-equal; its backward sums rowsum(dSd o S) from the accumulators in
another order, so the gradients are held to the bars and their largest difference is printed (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
import oracle
import test_tenc_train_gpu as base
from hand_pose_sl_amd import _lib
from tenc_train_ref import (assert_within_bar, leaf_state, masked_l1, param_keys, port_forward, port_grads, seeded_state,
                            tenc_cases)

pytestmark = pytest.mark.gpu
TOL_Y = base.TOL_Y
WORST = {"ratio": 0.0, "what": "", "y": 0.0}            # of these routes alone: base.WORST is the default route's
ATTN = {"valu": "b2h_tt_sdpa", "mfma": "b2h_mw_sdpa"}
LINEAR = {"valu": "b2h_tt_linear", "mfma": "b2h_ml_linear"}
_step, _params, _cpu = base._step, base._params, base._cpu


def _names(m, T=1):
    lib, _ = m._ensure_created()
    attn, lin = lib.b2h_tenc_train_attn_name(m._handle, T), lib.b2h_tenc_train_linear_name(m._handle)
    return (None if attn is None else attn.decode()), (None if lin is None else lin.decode())


def _set_handle(m, kernels, linear):
    lib, _ = m._ensure_created()
    assert lib.b2h_tenc_set_train_kernel(m._handle, _lib.TRAIN_KERNELS[kernels]) == _lib.OK
    assert lib.b2h_tenc_set_train_linear(m._handle, _lib.TRAIN_KERNELS[linear]) == _lib.OK


def routed(nlayers, p, state, dev, kernels="mfma", linear="mfma"):
    """A training model on the given routes; the handle too, for the tests that call the C ABI themselves."""
    m = base._model(nlayers, p, state, dev).set_train_kernels(kernels).set_train_linear(linear)
    _set_handle(m, kernels, linear)
    return m


class _Built(list):
    kernels, linear = "mfma", "mfma"

    def all_on_route(self):
        assert self and all((m.train_kernels, m.train_linear) == (self.kernels, self.linear) for m in self)
        # the handle follows the model at every training forward; this is what it was left at
        assert all(_names(m) == (ATTN[self.kernels], LINEAR[self.linear]) for m in self)


@pytest.fixture
def mw(monkeypatch):
    """test_tenc_train_gpu.py's helpers and tests on the MFMA routes; yields the models they built."""
    built = _Built()
    make = base._model

    def made(nlayers, p, state, dev):
        m = make(nlayers, p, state, dev).set_train_kernels(built.kernels).set_train_linear(built.linear)
        _set_handle(m, built.kernels, built.linear)
        built.append(m)
        return m
    monkeypatch.setattr(base, "_model", made)
    monkeypatch.setattr(base, "WORST", WORST)
    return built


_state = functools.lru_cache(maxsize=None)(seeded_state)   # read only: every model copies it


# ---- 1. sweep against float64 autograd of the port, with the masks the kernels used ------------------------------
SHAPES = [(1, 1), (3, 2), (1, 15), (3, 16), (3, 17), (2, 33), (1, 63), (1, 64), (2, 65), (3, 99), (2, 100)]
LONG = [(2, 101), (1, 113), (1, 127), (2, 128)]         # with a max_len = 128 table
ALL = [(s, 100) for s in SHAPES] + [(s, 128) for s in LONG]


@pytest.mark.parametrize("shape,max_len", ALL, ids=lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else f"pe{v}")
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("nlayers", [1, 4])
def test_sweep_against_float64_autograd(nlayers, p, shape, max_len, mw, cuda_device):
    j = [s for s, _ in ALL].index(shape)
    state = _state(nlayers, 100 + nlayers, max_len)
    base._check_case(state, nlayers, p, *shape, 1.0 if j % 2 else 1.0 / 1280, 5000 + 97 * nlayers + j, cuda_device)
    mw.all_on_route()
    assert _names(mw[0], shape[1])[0] == "b2h_mw_sdpa"
    print(f"\nmfma routes L={nlayers} p={p} {shape}: worst ratio so far {WORST['ratio']:.3f} ({WORST['what']}), "
          f"worst y error {WORST['y']:.3e}")


def test_sweep_with_randomized_layernorm_and_attention_biases(mw, cuda_device):
    base.test_sweep_with_randomized_layernorm_and_attention_biases(cuda_device)   # (3, 17) and (2, 100), p = 0.1
    mw.all_on_route()
    print(f"\nmfma routes: worst ratio so far {WORST['ratio']:.3f} ({WORST['what']}), worst y error {WORST['y']:.3e}")


# ---- 2. the reference's fixtures ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tenc_cases())
def test_gradients_match_reference_fixtures(name, mw, cuda_device):
    base.test_gradients_match_reference_fixtures(name, cuda_device)
    mw.all_on_route()


# ---- the routes against each other on one batch ------------------------------------------------------------------
def _one_step(state, nlayers, p, B, T, seed, dev, routes, scale=1.0, uniform=False):
    """One step of each (kernels, linear) route on one batch and one set of masks: route -> [y, gradients .., dx]."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((B, T, 12, 2), generator=g) - 0.5 if uniform else torch.randn((B, T, 12, 2), generator=g) * scale).to(dev)
    dy = torch.randn((B, T, 21, 2), generator=g).to(dev)
    got, masks = {}, None
    for route in routes:
        m = routed(nlayers, p, state, dev, *route)
        if masks is None:
            torch.manual_seed(seed + 1)
            masks = m._draw_dropout_masks(B, T)
        y, grads, dx = _step(m, x, dy, masks)
        assert _names(m, T) == (ATTN[route[0]], LINEAR[route[1]])
        got[route] = [y] + grads + [dx]
    return got


def _differences(a, b, nlayers):
    return [(k, float((u.double() - v.double()).abs().max()), float(v.abs().max()), torch.equal(u, v))
            for k, u, v in zip(["y"] + param_keys(nlayers) + ["dx"], a, b)]


# ---- 3. peaked attention and non-default parameters --------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T", [(3, 17), (2, 100)])
def test_gradients_under_peaked_attention_and_nondefault_params(B, T, p, mw, cuda_device):
    base.test_gradients_under_peaked_attention_and_nondefault_params(B, T, p, cuda_device)   # the bars
    mw.all_on_route()
    from test_tenc_params import _fixture
    state = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in _fixture()[0].items()}
    got = _one_step(state, 2, p, B, T, 4000 + T, cuda_device, [("mfma", "mfma"), ("valu", "valu")], uniform=True)
    diff = _differences(got[("mfma", "mfma")], got[("valu", "valu")], 2)
    print(f"\npeaked p={p} B={B} T={T}: bit-equal to the default route in {sum(d[3] for d in diff)} of {len(diff)} tensors; "
          f"largest difference {max((d[1] / max(d[2], 1e-300), d[0]) for d in diff)} (relative to the tensor's maximum)")
    assert diff[0][3], "y differs from the default route"


# ---- 4. route names, refusals and the default path ---------------------------------------------------------------
def test_route_names_refusals_and_default_path_unchanged(cuda_device):
    state = _state(2, 110)
    a, b = base._model(2, 0.1, state, cuda_device), base._model(2, 0.1, state, cuda_device)
    lib, _ = a._ensure_created()
    assert (a.train_kernels, a.train_linear) == ("valu", "valu")
    sizes = []
    for kv, kname in ((1, "b2h_mw_sdpa"), (0, "b2h_tt_sdpa")):
        for lv, lname in ((1, "b2h_ml_linear"), (0, "b2h_tt_linear")):
            assert lib.b2h_tenc_set_train_kernel(a._handle, kv) == _lib.OK
            assert lib.b2h_tenc_set_train_linear(a._handle, lv) == _lib.OK
            for T in (1, 100):
                assert _names(a, T) == (kname, lname)
            assert _names(a, 0)[0] is None and _names(a, 101)[0] is None and _names(a, 128)[0] is None  # max_len = 100
            for bad in (2, -1):                             # a refused value changes nothing
                assert lib.b2h_tenc_set_train_kernel(a._handle, bad) == _lib.ERR_INVALID
                assert lib.b2h_tenc_set_train_linear(a._handle, bad) == _lib.ERR_INVALID
                assert _names(a, 100) == (kname, lname)
            sizes.append([lib.b2h_tenc_train_bytes(a._handle, 2, T, which) for which in (0, 1) for T in (1, 17, 100)])
    assert all(s == sizes[0] for s in sizes) and all(sizes[0])   # the switches do not move the buffer sizes
    long_model = base._model(1, 0.1, _state(1, 111, 128), cuda_device)
    for kernels in ("mfma", "valu"):
        _set_handle(long_model, kernels, "valu")
        assert [_names(long_model, T)[0] for T in (1, 100, 128, 129, 0)] == [ATTN[kernels]] * 3 + [None, None]

    def step(m, B, T, seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((B, T, 12, 2), generator=g).to(cuda_device)
        dy = torch.randn((B, T, 21, 2), generator=g).to(cuda_device)
        torch.manual_seed(seed + 1)
        return _step(m, x, dy, m._draw_dropout_masks(B, T))

    def same(u, v):
        return torch.equal(u[0], v[0]) and torch.equal(u[2], v[2]) and all(torch.equal(s, t) for s, t in zip(u[1], v[1]))

    for B, T in ((3, 17), (2, 100)):
        a.set_train_kernels("mfma").set_train_linear("mfma")
        step(a, B, T, 5600 + T)                             # a ran on both MFMA routes ...
        assert _names(a, T) == ("b2h_mw_sdpa", "b2h_ml_linear")
        a.set_train_kernels("valu").set_train_linear("valu")    # ... and back on valu equals a model never switched
        assert same(step(a, B, T, 5600 + T), step(b, B, T, 5600 + T))
        assert _names(a, T) == ("b2h_tt_sdpa", "b2h_tt_linear") == _names(b, T)


# ---- 5. bit-equality ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,max_len", ALL, ids=lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else f"pe{v}")
def test_bit_equality_with_the_default_route(shape, max_len, cuda_device):
    """The MFMA Linears alone: y, dx and every gradient equal the default route's bit for bit.  Both switches: y equal
    bit for bit (the forward attention keeps the chains); the backward's rowsum is summed in another order (DESIGN.md
    section 20), so the gradients' largest difference is printed, not asserted to be zero."""
    nlayers, p = 2, 0.1
    routes = [("valu", "valu"), ("valu", "mfma"), ("mfma", "mfma")]
    got = _one_step(_state(nlayers, 120, max_len), nlayers, p, *shape, 5700 + shape[1], cuda_device, routes)
    unequal = [d[:2] for d in _differences(got[("valu", "mfma")], got[("valu", "valu")], nlayers) if not d[3]]
    assert not unequal, unequal
    diff = _differences(got[("mfma", "mfma")], got[("valu", "valu")], nlayers)
    assert diff[0][3], f"y differs from the default route by {diff[0][1]:.3e}"
    print(f"\n{shape}: both switches against the default route: {sum(d[3] for d in diff)} of {len(diff)} tensors bit-equal; "
          f"largest gradient difference {max((d[1] / max(d[2], 1e-300), d[0]) for d in diff[1:])} (relative to the tensor's maximum)")


# ---- 6. each switch alone and both together, on one batch, inside the bars ---------------------------------------
def test_each_switch_alone_and_both_inside_the_bars_on_the_same_batch(cuda_device):
    nlayers, p, B, T, seed = 2, 0.1, 2, 100, 5800
    state = _state(nlayers, 130)
    routes = [("mfma", "valu"), ("valu", "mfma"), ("mfma", "mfma")]
    got = _one_step(state, nlayers, p, B, T, seed, cuda_device, routes)
    g = torch.Generator().manual_seed(seed)                 # _one_step's batch and masks
    x = torch.randn((B, T, 12, 2), generator=g)
    dy = torch.randn((B, T, 21, 2), generator=g)
    torch.manual_seed(seed + 1)
    masks = _cpu(routed(nlayers, p, state, cuda_device)._draw_dropout_masks(B, T))
    y64, g64, dx64 = port_grads(x, state, masks, p, dy, torch.float64)
    _, g32, dx32 = port_grads(x, state, masks, p, dy, torch.float32)
    for route in routes:
        y, *grads = got[route]
        assert float((y.cpu().double() - y64).abs().max()) <= TOL_Y * max(1.0, float(y64.abs().max())), route
        for k, gg, a, b in zip(param_keys(nlayers) + ["dx"], grads, g64 + [dx64], g32 + [dx32]):
            assert_within_bar(gg.cpu().double().numpy(), a.numpy(), float((b.double() - a).abs().max()), f"{route} {k}")


# ---- 7. a backward follows its forward ---------------------------------------------------------------------------
def test_backward_runs_the_kernels_of_its_forward(cuda_device):
    B, T = 3, 33
    m = routed(2, 0.1, _state(2, 140), cuda_device)
    g = torch.Generator().manual_seed(5900)
    x = torch.randn((B, T, 12, 2), generator=g).to(cuda_device)
    dy = torch.randn((B, T, 21, 2), generator=g).to(cuda_device)
    torch.manual_seed(5901)
    masks = m._draw_dropout_masks(B, T)
    _, g_all, dx_all = _step(m, x, dy, masks)               # forward and backward on the MFMA routes
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(True)
    y = m._forward_train(xd, masks)
    m.set_train_kernels("valu").set_train_linear("valu")    # switched between the two
    _set_handle(m, "valu", "valu")                          # and the handle with it
    y.backward(dy)
    assert _names(m, T) == ("b2h_mw_sdpa", "b2h_ml_linear")     # what the backward set the handle to
    assert all(torch.equal(a, p.grad) for a, p in zip(g_all, _params(m))) and torch.equal(dx_all, xd.grad)
    _, g_valu, _ = _step(m, x, dy, masks)                   # the model says valu now: the next step runs it
    assert _names(m, T) == ("b2h_tt_sdpa", "b2h_tt_linear") and all(torch.isfinite(t).all() for t in g_valu)


# ---- 8. poisoned outputs, saved buffer and scratch; NaN right behind every operand -------------------------------
@pytest.mark.parametrize("B,T,with_dx", [(3, 17, True), (2, 100, False), (5, 1, True)])
def test_outputs_fully_written_and_scratch_contents_irrelevant(B, T, with_dx, mw, cuda_device):
    """poison.launch through the C ABI with the handle on both MFMA routes: saved and scratch buffers of exactly
    b2h_tenc_train_bytes, quiet NaNs right behind every operand; every output word is written and no bit changes
    against clean allocations.  A padded row or k-step that read past a tensor would differ."""
    base.test_outputs_fully_written_and_scratch_contents_irrelevant(B, T, with_dx, cuda_device)
    mw.all_on_route()
    lib, _ = mw[0]._ensure_created()
    on_mfma = [lib.b2h_tenc_train_bytes(mw[0]._handle, B, T, which) for which in (0, 1)]
    _set_handle(mw[0], "valu", "valu")                      # the default's sizes
    assert on_mfma == [lib.b2h_tenc_train_bytes(mw[0]._handle, B, T, which) for which in (0, 1)] and all(on_mfma)


# ---- 9. determinism ----------------------------------------------------------------------------------------------
def test_bitwise_deterministic_across_runs_streams_and_batches(mw, cuda_device):
    base.test_bitwise_deterministic_across_runs_streams_and_batches(cuda_device)   # (64, 100), p = 0.1
    mw.all_on_route()


# ---- 10. p = 0 equals eval, p = 1 drops everything ---------------------------------------------------------------
def test_p0_equals_eval_and_p1_drops_everything(mw, cuda_device):
    base.test_p0_equals_eval_and_p1_drops_everything(cuda_device)
    assert len(mw) == 2 and all((m.train_kernels, m.train_linear) == ("mfma", "mfma") for m in mw)
    assert _names(mw[1]) == ("b2h_mw_sdpa", "b2h_ml_linear")


# ---- 11. graph capture as the model's first use ------------------------------------------------------------------
def test_training_step_captured_in_graph_as_first_use_equals_eager(cuda_device):
    B, T = 8, 50
    state = _state(2, 90)
    g = torch.Generator().manual_seed(91)
    x = torch.randn((B, T, 12, 2), generator=g).to(cuda_device)
    dy = torch.randn((B, T, 21, 2), generator=g).to(cuda_device)
    eager = routed(2, 0.1, state, cuda_device)
    torch.manual_seed(92)
    masks = eager._draw_dropout_masks(B, T)
    _, eager_g, eager_dx = _step(eager, x, dy, masks)
    m = base._model(2, 0.1, state, cuda_device).set_train_kernels("mfma").set_train_linear("mfma")   # has not run yet
    xs = x.clone().requires_grad_(True)
    s = torch.cuda.Stream(cuda_device)                      # warm-up on a side stream, as torch's docs do
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        m._forward_train(xs, masks).backward(dy)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    for p in m.parameters():
        p.grad = None
    xs.grad = None
    with torch.cuda.graph(graph):                           # one stream: no parallel branches
        m._forward_train(xs, masks).backward(dy)
    for p in m.parameters():
        p.grad.fill_(float("nan"))
    xs.grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert _names(m, T) == ("b2h_mw_sdpa", "b2h_ml_linear")
    for a, p in zip(eager_g, _params(m)):
        assert torch.equal(a, p.grad)
    assert torch.equal(eager_dx, xs.grad)


# ---- 12. the reference loop body with Adam, then eval-mode inference on the updated weights ----------------------
def test_five_adam_steps_and_inference_after_updates(cuda_device):
    L, B, T, steps, lr = 2, 4, 64, 5, 2e-4
    lengths = [64, 40, 17, 64]
    state = _state(L, 70)
    g = torch.Generator().manual_seed(71)
    x = torch.rand((B, T, 12, 2), generator=g) - 0.5
    target = (torch.rand((B, T, 21, 2), generator=g) - 0.5) * 0.2
    keys = param_keys(L)
    ref = {}
    for dt in (torch.float64, torch.float32):               # the port's trajectories: the truth and the fp32 reference
        st = leaf_state(state, dt)
        opt = torch.optim.Adam([st[k] for k in keys], lr=lr)
        losses = []
        for _ in range(steps):
            loss = masked_l1(port_forward(x.to(dt), st, {}, 0.0, dt), target.to(dt), lengths)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        ref[dt] = (np.array(losses), {k: st[k].detach().double().numpy() for k in keys})
    m = routed(L, 0.0, state, cuda_device)
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    criterion = hps.maskedPoseL1()
    xd, td = x.to(cuda_device), target.to(cuda_device)
    losses = []
    for _ in range(steps):                                  # traintest.py:94-121
        prediction = m(xd)
        for i, n in enumerate(lengths):
            prediction[i, n:, :] = 0
        loss = criterion(prediction, td, lengths)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert _names(m, T) == ("b2h_mw_sdpa", "b2h_ml_linear")
    (l64, f64), (l32, f32) = ref[torch.float64], ref[torch.float32]
    assert_within_bar(np.array(losses), l64, np.abs(l32 - l64).max(), "losses")
    sd = m.state_dict()
    for k in keys:
        assert_within_bar(sd[k].cpu().double().numpy(), f64[k], np.abs(f32[k] - f64[k]).max(), "final " + k)
    m.eval()                                                # the inference path packs the updated weights
    with torch.no_grad():
        y = m(xd).cpu().numpy()
    want = oracle.transformer_forward(x.numpy(), {k: v.cpu().numpy() for k, v in sd.items()})
    assert np.abs(y - want).max() <= TOL_Y
