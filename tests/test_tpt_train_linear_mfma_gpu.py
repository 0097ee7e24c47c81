"""TextPoseTransformer training with its Linear layers on the fp32 MFMA route (`model.set_train_linear("mfma")`:
b2h_ml_linear, b2h_ml_linear_dx, b2h_ml_linear_dw of kernel_train_linear_mfma.h) on the MI355X.

The bars are the project's own (tpt_train_ref.assert_within_bar: per tensor max|g - g64| <= 4 * max|g32_ref - g64| +
1e-6 * max|g64|; y within tpt_ref.BAR * max(1, max|y64|)), and the inputs are chosen by the rule of
test_tpt_train_long_gpu.py (`_check_case`: on the CPU ports alone, no float64 ReLU input closer to zero than
RELU_MARGIN times the float32 port's rounding).  That module's helpers, and those of its tests that this route has to
pass unchanged, run here with its `train_model` replaced by one that selects the MFMA Linears (the `ml` fixture); every
model built that way is checked to have resolved to b2h_ml_linear.  The Linear kernels have no length threshold, so the
shapes lie on both sides of T = 128, where the attention changes kernels, and the longer ones run under both values of
`set_train_kernels`.  The sweep prints the worst ratio max|g - g64| / max|g32_ref - g64| and the worst y error it has
seen so far (pytest -s)."""
import ctypes

import pytest
import torch

import hand_pose_sl_amd as hps
import test_tpt_train_long_gpu as long_gpu
import tpt_geom_ref
from poison import launch as poisoned_launch
from tpt_train_ref import (assert_within_bar, cpu_masks, layer_counts, param_keys, port_grads, recipe_state,
                           tokens_with_padding, train_model)

pytestmark = pytest.mark.gpu
N_TOKENS = long_gpu.N_TOKENS
WORST = {"ratio": 0.0, "what": "", "y": 0.0}            # of this route alone: long_gpu.WORST is the default route's
_data, _step, _grads, _cpu, _tol_y = long_gpu._data, long_gpu._step, long_gpu._grads, long_gpu._cpu, long_gpu._tol_y


def _linear_name(m):
    lib, _ = m._ensure_created()
    name = lib.b2h_tpt_train_linear_name(m._handle)
    return None if name is None else name.decode()


def ml_model(state, p, dev, kernels="valu"):
    return train_model(state, p, dev).set_train_linear("mfma").set_train_kernels(kernels)


class _Built(list):
    def all_on_ml(self):
        assert self and all(m.train_linear == "mfma" for m in self)
        # the handle follows the model at every training forward; this is what it was left at
        assert all(_linear_name(m) == "b2h_ml_linear" for m in self)


@pytest.fixture
def ml(monkeypatch):
    """test_tpt_train_long_gpu.py's helpers and tests on the MFMA Linears; yields the models they built.  `ml.kernels`
    is the attention switch those models get ("valu" unless a test sets it first)."""
    built = _Built()
    built.kernels = "valu"

    def wrap(make):
        def made(state, p, dev=None):
            m = make(state, p, dev).set_train_linear("mfma").set_train_kernels(built.kernels)
            built.append(m)
            return m
        return made
    monkeypatch.setattr(long_gpu, "train_model", wrap(train_model))
    monkeypatch.setattr(tpt_geom_ref, "train_model", wrap(tpt_geom_ref.train_model))
    monkeypatch.setattr(long_gpu, "WORST", WORST)
    return built


# ---- 1. sweep against float64 autograd of the port, with the masks the kernels used ------------------------------
# Nt = B T and Ns = B S on both sides of 16 (the MFMA tile and a wave's rows), 64 (a workgroup's rows, dw's row tile)
# and 128 (two row tiles: the slab count changes), and = 0 .. 3 mod 4 (the k-step of dw, which sums over rows).
SHAPES = [(1, 1, 1), (1, 7, 15), (1, 16, 17), (3, 9, 21), (1, 40, 64), (5, 33, 13), (1, 38, 127), (1, 17, 129),
          (3, 33, 144), (2, 40, 200)]
DEEP = [(1, 7, 15), (5, 33, 13), (1, 17, 129), (2, 40, 200)]    # also with (2, 3) layers
CASES = [(layers, s, k) for layers, shapes in (((1, 1), SHAPES), ((2, 3), DEEP)) for s in shapes
         for k in (("valu", "mfma") if s[2] > 128 else ("valu",))]


@pytest.mark.parametrize("layers,shape,kernels", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(str(i) for i in v))
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_sweep_against_float64_autograd(p, layers, shape, kernels, ml, cuda_device):
    ml.kernels = kernels
    state = recipe_state(400 + 10 * layers[0] + layers[1], N_TOKENS, *layers)   # non-default biases and LayerNorms
    j = SHAPES.index(shape)
    unused = long_gpu._check_case(state, p, *shape, 1.0 if j % 2 else 1.0 / 1280, 8000 + 97 * layers[1] + j, cuda_device)
    assert N_TOKENS - 1 in unused                       # rows of unused ids are exactly zero (checked in _check_case)
    ml.all_on_ml()
    assert all(m.train_kernels == kernels for m in ml)


# ---- 2. the other geometries: K = 16, 58, 42 in the forward and dw, M = 8, 24, 42 summed over in dx --------------
@pytest.mark.parametrize("shape", [(2, 9, 33), (2, 40, 130)], ids=lambda s: "b%d_s%d_t%d" % s)
@pytest.mark.parametrize("n_joints,nout", [(8, 42), (29, 8), (21, 24)])
def test_geometries(n_joints, nout, shape, ml, cuda_device):
    (B, S, T), p = shape, 0.1
    state = tpt_geom_ref.recipe_state(420 + n_joints, N_TOKENS, n_joints, nout, 1, 2)
    m = tpt_geom_ref.train_model(state, p, cuda_device)
    g = torch.Generator().manual_seed(8300 + n_joints + T)
    tok = tokens_with_padding(B, S, N_TOKENS, g)
    x = torch.randn((B, T, n_joints, 2), generator=g)
    dy = torch.randn((B, T, nout // 2, 2), generator=g)
    torch.manual_seed(8301)
    masks = m._draw_dropout_masks(B, S, T)
    xd = x.to(cuda_device).requires_grad_(True)
    y = m._forward_train(tok.to(cuda_device), xd, masks)
    y.backward(dy.to(cuda_device))
    ml.all_on_ml()
    y64, g64, dx64 = tpt_geom_ref.port_grads(tok, x, state, _cpu(masks), p, dy, torch.float64)
    _, g32, dx32 = tpt_geom_ref.port_grads(tok, x, state, _cpu(masks), p, dy, torch.float32)
    assert float((y.detach().cpu().double() - y64).abs().max()) <= _tol_y(y64)
    for k, gg, a, b in zip(param_keys(1, 2), _grads(m), g64, g32):
        assert_within_bar(gg, a.numpy(), (b.double() - a).abs().max(), f"({n_joints},{nout}) {k}")
    assert_within_bar(xd.grad.cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "dx")


# ---- 3. the slab cap and unequal tile ownership -----------------------------------------------------------------
# (65, 3, 128): Nt = 8320, S = 64 slabs over 130 row tiles, so slabs 0 and 1 own three tiles and the others two;
# (1, 3, 260): Nt = 260, S = 3 slabs over five tiles (2, 2, 1), the last tile with 4 rows.
#
# The ReLU-margin rule cannot hold over 8320 independent frame rows: of a million ReLU inputs about six lie within the
# float32 port's rounding (4e-6) of zero whatever the draw.  So the 65 sequences of the first shape are copies of one
# (tokens and pose, at p = 0: no masks), which has the ReLU inputs of (1, 3, 128) and passes the rule as that shape
# does, while dy is drawn per sequence: every row tile adds numbers of its own to dW and db, and a tile that a slab
# skipped or took twice moves the sum by about 1 / 130 of it, far above the bar.
@pytest.mark.parametrize("shape", [(65, 3, 128), (1, 3, 260)], ids=lambda s: "b%d_s%d_t%d" % s)
def test_slab_cap_and_unequal_ownership(shape, ml, cuda_device):
    B, S, T = shape
    seed = 8400 + T

    def copies(attempt):
        tok, x, _ = _data(1, S, T, N_TOKENS, seed + 100000 * attempt)
        return tok.expand(B, -1).contiguous(), x.expand(B, -1, -1, -1).contiguous()
    if B > 1:
        long_gpu._check_case(recipe_state(431, N_TOKENS, 1, 1), 0.0, B, S, T, 1.0, seed, cuda_device, inputs=copies)
    else:
        long_gpu._check_case(recipe_state(431, N_TOKENS, 1, 1), 0.1, B, S, T, 1.0, seed, cuda_device)
    ml.all_on_ml()


# ---- 4. determinism ---------------------------------------------------------------------------------------------
def test_bitwise_deterministic_across_runs_streams_and_batches(ml, cuda_device):
    long_gpu.test_bitwise_deterministic_across_runs_streams_and_batches(cuda_device)   # (8, 40, 200), p = 0.1
    ml.all_on_ml()


# ---- 5. the padded-row rule: NaN right behind every tensor, buffers of exactly b2h_tpt_train_bytes ---------------
@pytest.mark.parametrize("shape", [(1, 7, 15), (1, 17, 129)], ids=lambda s: "b%d_s%d_t%d" % s)
def test_nan_behind_every_tensor_changes_no_bit(shape, cuda_device):
    """poison.launch: every operand sits between guard bands -- quiet NaNs right behind the last row of the tokens, the
    pose, dy, every parameter and mask; the saved buffer, the scratch, the outputs and their guards hold a NaN pattern
    -- and the same call runs again on clean, zero-filled allocations.  It asserts that every output word was written
    and that the two runs agree bit for bit.  A padded row or k-step that read past a tensor would differ."""
    (B, S, T), (ne, nd, p) = shape, (1, 2, 0.1)
    state = recipe_state(460, N_TOKENS, ne, nd)
    m = train_model(state, p, cuda_device)
    lib, _ = m._ensure_created()
    assert lib.b2h_tpt_set_train_linear(m._handle, hps._lib.TRAIN_KERNELS["mfma"]) == hps._lib.OK
    tok, x, dy = _data(B, S, T, N_TOKENS, 8500 + T)
    masks = cpu_masks(B, S, T, ne, nd, p, 8501)
    tensors = [t.detach().cpu() for t in m._tensors()]
    inputs = dict(tok=tok, x=x, dy=dy)
    inputs.update({f"p{i}": t for i, t in enumerate(tensors)})
    inputs.update({f"m{i}": t for i, t in enumerate(masks.values())})
    outs = {f"g{i}": tuple(t.shape) for i, t in enumerate(tensors)}
    outs["dx"] = (B, T, 12, 2)
    outs["y"] = (B, T, 21, 2)
    nsaved, nws = lib.b2h_tpt_train_bytes(m._handle, B, S, T, 0), lib.b2h_tpt_train_bytes(m._handle, B, S, T, 1)
    vp = ctypes.c_void_p

    def call(q):
        pa = (vp * len(tensors))(*[q[f"p{i}"] for i in range(len(tensors))])
        ma = (vp * len(masks))(*[q[f"m{i}"] for i in range(len(masks))])
        ga = (vp * len(tensors))(*[q[f"g{i}"] for i in range(len(tensors))])
        rc = lib.b2h_tpt_train_forward(m._handle, pa, q["tok"], q["x"], ma, p, q["y"], q["saved"], nsaved, B, S, T, None)
        return rc or lib.b2h_tpt_backward(m._handle, pa, q["tok"], ma, p, q["dy"], q["saved"], nsaved, q["dx"], ga,
                                          q["ws"], nws, B, S, T, None)

    res = poisoned_launch(call, inputs, outs, cuda_device, scratch={"saved": nsaved, "ws": nws})
    assert _linear_name(m) == "b2h_ml_linear"
    y64, g64, dx64 = port_grads(tok, x, state, masks, p, dy, torch.float64)
    _, g32, dx32 = port_grads(tok, x, state, masks, p, dy, torch.float32)
    assert float((res["y"].cpu().double() - y64).abs().max()) <= _tol_y(y64)
    keys = param_keys(ne, nd)
    for i, (a, b) in enumerate(zip(g64, g32)):
        assert_within_bar(res[f"g{i}"].cpu().double().numpy(), a.numpy(), (b.double() - a).abs().max(), keys[i])
    assert_within_bar(res["dx"].cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "dx")


# ---- 6. the default path is untouched ---------------------------------------------------------------------------
def _same(u, v):
    return torch.equal(u[0], v[0]) and torch.equal(u[2], v[2]) and all(torch.equal(s, t) for s, t in zip(u[1], v[1]))


def test_default_path_untouched(cuda_device):
    state = recipe_state(410, N_TOKENS, 1, 2)
    a, b = train_model(state, 0.1, cuda_device), train_model(state, 0.1, cuda_device)
    lib, _ = a._ensure_created()
    assert a.train_linear == "valu" and _linear_name(a) == "b2h_tt_linear"      # the default of a new model
    sizes = []
    for value, name in ((1, "b2h_ml_linear"), (0, "b2h_tt_linear")):
        assert lib.b2h_tpt_set_train_linear(a._handle, value) == hps._lib.OK
        assert _linear_name(a) == name
        sizes.append([lib.b2h_tpt_train_bytes(a._handle, 2, 40, T, which) for which in (0, 1) for T in (100, 200)])
    assert sizes[0] == sizes[1] and all(sizes[0])       # the switch does not move the buffer sizes
    for value in (1, 0):
        assert lib.b2h_tpt_set_train_linear(a._handle, value) == hps._lib.OK
        for bad in (2, -1):
            assert lib.b2h_tpt_set_train_linear(a._handle, bad) == hps._lib.ERR_INVALID
            assert _linear_name(a) == ("b2h_ml_linear", "b2h_tt_linear")[1 - value]   # a refused value changes nothing
        name = lib.b2h_tpt_train_attn_name(a._handle, 200)
        assert name.decode() == "b2h_lt_sdpa"           # and the attention switch does not know this one

    def step(m, B, S, T, seed):
        tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, seed))
        torch.manual_seed(seed + 1)
        return _step(m, tok, x, dy, m._draw_dropout_masks(B, S, T))

    for B, S, T in ((2, 17, 130), (2, 40, 100)):
        a.set_train_linear("mfma")
        step(a, B, S, T, 8600 + T)                      # a ran on the MFMA Linears ...
        assert _linear_name(a) == "b2h_ml_linear"
        a.set_train_linear("valu")                      # ... and back on valu equals a model never switched
        assert _same(step(a, B, S, T, 8600 + T), step(b, B, S, T, 8600 + T))
        assert _linear_name(a) == "b2h_tt_linear" and _linear_name(b) == "b2h_tt_linear"


# ---- 7. a backward follows its forward --------------------------------------------------------------------------
def test_backward_runs_the_linears_of_its_forward(cuda_device):
    B, S, T = 2, 17, 130
    m = ml_model(recipe_state(420, N_TOKENS, 1, 2), 0.1, cuda_device)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 8700))
    torch.manual_seed(8701)
    masks = m._draw_dropout_masks(B, S, T)
    _, g_all, dx_all = _step(m, tok, x, dy, masks)      # forward and backward on the MFMA Linears
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(True)
    y = m._forward_train(tok, xd, masks)
    m.set_train_linear("valu")                          # switched between the two
    lib, _ = m._ensure_created()
    assert lib.b2h_tpt_set_train_linear(m._handle, 0) == hps._lib.OK            # and the handle with it
    y.backward(dy)
    assert _linear_name(m) == "b2h_ml_linear"           # what the backward set the handle to
    assert m.train_kernels == "valu"                    # independent of the attention switch, which nobody touched
    assert all(torch.equal(a, p.grad) for a, p in zip(g_all, m._tensors())) and torch.equal(dx_all, xd.grad)
    _, g_valu, _ = _step(m, tok, x, dy, masks)          # the model says valu now: the next step runs it
    assert _linear_name(m) == "b2h_tt_linear" and all(torch.isfinite(g).all() for g in g_valu)


# ---- 8. graph capture as the model's first use -----------------------------------------------------------------
def test_training_step_captured_in_graph_as_first_use_equals_eager(cuda_device):
    B, S, T = 2, 17, 130
    state = recipe_state(490, N_TOKENS, 2, 2)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 8800))
    eager = ml_model(state, 0.1, cuda_device)
    torch.manual_seed(8801)
    masks = eager._draw_dropout_masks(B, S, T)
    _, eager_g, eager_dx = _step(eager, tok, x, dy, masks)
    m = ml_model(state, 0.1, cuda_device)               # a model that has not run yet
    xs = x.clone().requires_grad_(True)
    s = torch.cuda.Stream(cuda_device)                  # warm-up on a side stream, as torch's docs do
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        m._forward_train(tok, xs, masks).backward(dy)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    for p in m.parameters():
        p.grad = None
    xs.grad = None
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        m._forward_train(tok, xs, masks).backward(dy)
    for p in m.parameters():
        p.grad.fill_(float("nan"))
    xs.grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert _linear_name(m) == "b2h_ml_linear"
    for a, p in zip(eager_g, m._tensors()):
        assert torch.equal(a, p.grad)
    assert torch.equal(eager_dx, xs.grad)


# ---- 9. edge cases ----------------------------------------------------------------------------------------------
def test_p0_equals_eval_long_path_and_p1_within_the_bars(ml, cuda_device):
    # T = 130; p = 1 is held to the bars against float64 there, as the default route is
    long_gpu.test_p0_equals_eval_long_path_and_p1_drops_everything(cuda_device)
    ml.all_on_ml()


def test_out_of_range_device_id_poisons_its_sequence_only(ml, cuda_device):
    long_gpu.test_out_of_range_device_id_poisons_its_sequence_only(cuda_device)   # y, dx of sequence 0 == it alone
    ml.all_on_ml()


def test_limits_and_errors(ml, cuda_device):
    long_gpu.test_limits_and_errors(cuda_device)        # T = 1025 is refused, by the model and by the C ABI
    assert ml and all(m.train_linear == "mfma" for m in ml)


# ---- 10. the loop body with Adam, inference afterwards ----------------------------------------------------------
def test_adam_trajectory_and_inference_after_updates(ml, cuda_device):
    # five steps at (4, 40, 200), lengths [200, 130, 17, 200], lr 2e-4; then forward_fused in eval mode
    long_gpu.test_adam_trajectory_and_inference_after_updates(cuda_device)
    ml.all_on_ml()


# ---- 11. the two Linear routes on one batch ---------------------------------------------------------------------
def _route_difference(state, p, B, S, T, seed, dev, kernels="valu"):
    """One step of both Linear routes on one batch: [(name, max|a - b|, bit-equal)] over y, the gradients and dx."""
    ne, nd = layer_counts(state)
    models = {"mfma": ml_model(state, p, dev, kernels), "valu": train_model(state, p, dev).set_train_kernels(kernels)}
    tok, x, dy = (t.to(dev) for t in _data(B, S, T, N_TOKENS, seed))
    torch.manual_seed(seed + 1)
    masks = models["mfma"]._draw_dropout_masks(B, S, T)
    got = {}
    for name, m in models.items():
        y, grads, dx = _step(m, tok, x, dy, masks)
        assert _linear_name(m) == ("b2h_ml_linear" if name == "mfma" else "b2h_tt_linear")
        got[name] = [y] + grads + [dx]
    return [(k, float((a.double() - b.double()).abs().max()), torch.equal(a, b))
            for k, a, b in zip(["y"] + param_keys(ne, nd) + ["dx"], got["mfma"], got["valu"])]


def test_both_linear_routes_inside_the_bars_on_the_same_batch(cuda_device):
    B, S, T, p = 2, 40, 200, 0.1
    ne, nd = 1, 2
    state = recipe_state(430, N_TOKENS, ne, nd)
    tok, x, dy = _data(B, S, T, N_TOKENS, 8900)
    models = {"mfma": ml_model(state, p, cuda_device), "valu": train_model(state, p, cuda_device)}
    torch.manual_seed(8901)
    masks = models["mfma"]._draw_dropout_masks(B, S, T)
    y64, g64, dx64 = port_grads(tok, x, state, _cpu(masks), p, dy, torch.float64)
    _, g32, dx32 = port_grads(tok, x, state, _cpu(masks), p, dy, torch.float32)
    keys = param_keys(ne, nd) + ["dx"]
    truth = [g.numpy() for g in g64] + [dx64.numpy()]
    err32 = [float((b.double() - a).abs().max()) for a, b in zip(g64 + [dx64], g32 + [dx32])]
    got, raw = {}, {}
    for name, m in models.items():
        y, grads, dx = _step(m, tok.to(cuda_device), x.to(cuda_device), dy.to(cuda_device), masks)
        assert _linear_name(m) == ("b2h_ml_linear" if name == "mfma" else "b2h_tt_linear")
        assert float((y.cpu().double() - y64).abs().max()) <= _tol_y(y64), name
        raw[name] = [y] + grads + [dx]
        got[name] = [g.cpu().double().numpy() for g in grads + [dx]]
        for k, g, a, e in zip(keys, got[name], truth, err32):
            assert_within_bar(g, a, e, f"{name} {k}")
    print()
    equal = [torch.equal(a, b) for a, b in zip(raw["mfma"], raw["valu"])]
    print(f"bit-equal between the Linear routes: {sum(equal)} of {len(equal)} tensors (y, {len(keys) - 1} gradients, dx)")
    for k, a, b, e in zip(["y"] + keys, raw["mfma"], raw["valu"], equal):
        if not e:
            print(f"max|mfma - valu| {k}: {float((a.double() - b.double()).abs().max()):.3e} (max| | {float(b.abs().max()):.3e})")


# Measured on the MI355X: the two Linear routes are bit-equal on every shape of the sweep, as
# the common summation order allows.  So it is asserted: y, every gradient and dx, one step per case, no CPU reference.
@pytest.mark.parametrize("layers,shape,kernels", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(str(i) for i in v))
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_linear_routes_bit_equal_over_the_sweep(p, layers, shape, kernels, cuda_device):
    state = recipe_state(400 + 10 * layers[0] + layers[1], N_TOKENS, *layers)
    unequal = [(k, d) for k, d, equal in _route_difference(state, p, *shape, 9000, cuda_device, kernels) if not equal]
    assert not unequal, unequal
