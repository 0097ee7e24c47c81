"""TextPoseTransformer training on the MI355X (kernel_tpt_train.h and kernel_tenc_train.h through
b2h_tpt_train_forward / b2h_tpt_backward and hand_pose_sl_amd's autograd Function).

Accuracy bar, per tensor (train_ref.bar): max|g_gpu - g64| <= 4 * max|g32_ref - g64| + 1e-6 * max|g64|, with g64
float64 autograd (of the reference's own class for the fixtures, of tpt_train_ref.port_forward -- which takes the
very dropout masks the kernels used -- everywhere else) and g32_ref the same computation in float32 on the CPU.
The forward output is held to tpt_ref.BAR * max(1, max|y64|).  The sweep prints the worst ratio
max|g - g64| / max|g32_ref - g64| it has seen so far (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
import tpt_ref
from poison import launch as poisoned_launch
from tpt_train_ref import (TRAIN_CASES, assert_within_bar, cpu_masks, leaf_state, load_train, mask_shapes, masked_l1,
                           param_keys, port_forward, port_grads, recipe_state, tokens_with_padding, train_model)

pytestmark = pytest.mark.gpu
N_TOKENS = 50


def _grads(m):
    return [p.grad.detach().cpu().double().numpy() for p in m._tensors()]


def _cpu(masks):
    return {k: v.cpu() for k, v in masks.items()}


def _tol_y(y64):
    return tpt_ref.BAR * max(1.0, float(y64.abs().max()))


def _data(B, S, T, n_tokens, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    tok = tokens_with_padding(B, S, n_tokens, g)
    return tok, torch.randn((B, T, 12, 2), generator=g) * scale, torch.randn((B, T, 21, 2), generator=g)


# ---- 1. the reference's fixtures ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRAIN_CASES)
def test_gradients_match_reference_fixtures(name, cuda_device):
    r = load_train(name)
    m = train_model(r["state"], 0.0, cuda_device)
    tokens = torch.from_numpy(r["tokens"]).to(cuda_device)
    x = torch.from_numpy(r["x"]).to(cuda_device).requires_grad_(True)
    target = torch.from_numpy(r["target"]).to(cuda_device)
    lengths = [int(n) for n in r["lengths"]]
    prediction = m(tokens, x)                           # traintest.py:105-107
    for i, n in enumerate(lengths):                     # mask_output (steps/utils.py:309-312), in place
        prediction[i, n:, :] = 0
    loss = hps.maskedPoseL1()(prediction, target, lengths)
    assert loss.grad_fn is not None
    loss.backward()
    assert_within_bar(np.array(loss.item()), r["loss64"], abs(float(r["loss32"]) - float(r["loss64"])), f"{name} loss")
    stored = 0
    for k, g in zip(param_keys(r["n_enc"], r["n_dec"]), _grads(m)):
        if "g64_" + k in r:
            assert_within_bar(g, r["g64_" + k], r["err32_" + k], f"{name} {k}")
            stored += 1
    assert stored >= 30
    assert_within_bar(x.grad.cpu().double().numpy(), r["dx64"], r["err32_dx"], f"{name} dx")


# ---- 2. sweep against float64 autograd of the port, with the masks the kernels used --------------------------
# S and T on both sides of the 16-row linear tiles and of the 64-lane halves of a softmax row, S < T and S > T, the
# LDS maximum (128, 128), and row counts whose two slab counts differ ((17, 40, 100): 6 and 14)
SHAPES = [(1, 1, 1), (2, 1, 17), (2, 17, 1), (3, 15, 16), (3, 16, 15), (2, 17, 33), (1, 64, 65), (2, 65, 63), (2, 40, 100),
          (1, 128, 100), (1, 100, 128), (2, 128, 128), (17, 40, 100)]
WORST = {"ratio": 0.0, "what": "", "y": 0.0}


def _check_case(state, p, B, S, T, scale, seed, dev):
    n_tokens = state["token_embedding.weight"].shape[0]
    tok, x, dy = _data(B, S, T, n_tokens, seed, scale)
    if S > 1:
        assert (tok[:, -1] == 0).all()                  # padding fills the tail of every row
    m = train_model(state, p, dev)
    torch.manual_seed(seed)
    masks = m._draw_dropout_masks(B, S, T)
    assert bool(masks) == (p > 0)
    xd = x.to(dev).requires_grad_(True)
    y = m._forward_train(tok.to(dev), xd, masks)
    y.backward(dy.to(dev))
    cm = _cpu(masks)
    y64, g64, dx64 = port_grads(tok, x, state, cm, p, dy, torch.float64)
    _, g32, dx32 = port_grads(tok, x, state, cm, p, dy, torch.float32)
    n_enc, n_dec = m._geom[5], m._geom[6]
    what = f"L=({n_enc},{n_dec}) p={p} B={B} S={S} T={T} scale={scale:.2g}"
    err_y = float((y.detach().cpu().double() - y64).abs().max())
    WORST["y"] = max(WORST["y"], err_y)
    assert err_y <= _tol_y(y64), f"{what}: y {err_y:.3e}"
    keys = param_keys(n_enc, n_dec)
    got = _grads(m)
    todo = [(k, gg, a.numpy(), b.double().numpy()) for k, gg, a, b in zip(keys, got, g64, g32)]
    todo.append(("dx", xd.grad.cpu().double().numpy(), dx64.numpy(), dx32.double().numpy()))
    for k, gg, a, b in todo:
        err32 = np.abs(b - a).max()
        if err32 > 0:
            ratio = float(np.abs(gg - a).max() / err32)
            if ratio > WORST["ratio"]:
                WORST.update(ratio=ratio, what=f"{what} {k}")
        assert_within_bar(gg, a, err32, f"{what} {k}")
    unused = sorted(set(range(n_tokens)) - set(tok.reshape(-1).tolist()))
    table = got[keys.index("token_embedding.weight")]
    assert not table[unused].any()                      # rows of ids the batch does not contain: exactly zero
    print(f"\n{what}: worst ratio so far {WORST['ratio']:.3f} ({WORST['what']}), worst y error {WORST['y']:.3e}")
    return unused


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d_s%d_t%d" % s)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("layers", [(1, 1), (2, 3)], ids=lambda l: "e%d_d%d" % l)
def test_sweep_against_float64_autograd(layers, p, shape, cuda_device):
    state = recipe_state(100 + 10 * layers[0] + layers[1], N_TOKENS, *layers)   # non-default biases and LayerNorms
    j = SHAPES.index(shape)
    unused = _check_case(state, p, *shape, 1.0 if j % 2 else 1.0 / 1280, 1000 + 97 * layers[1] + j, cuda_device)
    assert N_TOKENS - 1 in unused                       # at least one id is never used


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_sweep_with_a_single_token_vocabulary(p, cuda_device):
    _check_case(recipe_state(131, 1, 1, 1), p, 3, 9, 17, 1.0, 3000, cuda_device)


# ---- 3. seed and mask order -----------------------------------------------------------------------------------
def _step(m, tok, x, dy, masks=None):
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(True)
    y = m(tok, xd) if masks is None else m._forward_train(tok, xd, masks)
    y.backward(dy)
    return y.detach().clone(), [p.grad.clone() for p in m._tensors()], xd.grad.clone()


def test_dropout_follows_the_seed_and_the_given_masks(cuda_device):
    B, S, T, p = 3, 11, 37, 0.1
    m = train_model(recipe_state(40, N_TOKENS, 2, 2), p, cuda_device)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 41))
    torch.manual_seed(7)
    y1, g1, dx1 = _step(m, tok, x, dy)
    torch.manual_seed(7)
    y2, g2, dx2 = _step(m, tok, x, dy)
    torch.manual_seed(7)
    masks = m._draw_dropout_masks(B, S, T)
    y3, g3, dx3 = _step(m, tok, x, dy, masks)
    assert torch.equal(y1, y2) and torch.equal(y1, y3) and torch.equal(dx1, dx2) and torch.equal(dx1, dx3)
    for a, b, c in zip(g1, g2, g3):
        assert torch.equal(a, b) and torch.equal(a, c)
    torch.manual_seed(8)
    assert not torch.equal(_step(m, tok, x, dy)[0], y1)
    # the documented order and shapes
    assert [(k, tuple(v.shape)) for k, v in masks.items()] == mask_shapes(B, S, T, 2, 2)
    assert list(masks)[:5] == [("enc", 0, "attn"), ("enc", 0, "drop1"), ("enc", 0, "ff"), ("enc", 0, "drop2"), ("enc", 1, "attn")]
    assert list(masks)[8:14] == [("dec", 0, n) for n in ("self_attn", "drop1", "cross_attn", "drop2", "ff", "drop3")]
    assert masks[("dec", 1, "cross_attn")].shape == (B, 4, T, S) and masks[("enc", 1, "attn")].shape == (B, 4, S, S)
    assert all(v.dtype == torch.uint8 and v.device.type == "cuda" for v in masks.values())


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_keep_rates(p, cuda_device):
    m = train_model(recipe_state(42, N_TOKENS, 1, 1), p, cuda_device)
    torch.manual_seed(9)
    for k, v in m._draw_dropout_masks(16, 40, 100).items():
        assert int(v.max()) <= 1
        sigma = (p * (1 - p) / v.numel()) ** 0.5
        assert abs(float(v.float().mean()) - (1 - p)) <= 5 * sigma, k


# ---- 4. p = 0 and p = 1 ---------------------------------------------------------------------------------------
def test_p0_equals_eval_and_p1_drops_everything(cuda_device):
    state = recipe_state(43, N_TOKENS, 2, 2)
    B, S, T = 3, 9, 17
    tok, x, dy = _data(B, S, T, N_TOKENS, 44)
    m = train_model(state, 0.0, cuda_device)
    assert m._draw_dropout_masks(B, S, T) == {}
    y_train = m(tok.to(cuda_device), x.to(cuda_device))
    assert y_train.grad_fn is not None
    with torch.no_grad():
        y_eval = m.eval()(tok.to(cuda_device), x.to(cuda_device))
    y64 = tpt_ref.Checker(m, torch.float64)(tok, x)
    assert float((y_train.detach() - y_eval).abs().max()) <= _tol_y(y64)
    assert float((y_train.detach().cpu().double() - y64).abs().max()) <= _tol_y(y64)
    m = train_model(state, 1.0, cuda_device)
    torch.manual_seed(1)
    masks = m._draw_dropout_masks(B, S, T)
    assert not any(bool(v.any()) for v in masks.values())
    y, grads, dx = _step(m, tok.to(cuda_device), x.to(cuda_device), dy.to(cuda_device), masks)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all() and all(torch.isfinite(t).all() for t in grads)
    y64, g64, dx64 = port_grads(tok, x, state, _cpu(masks), 1.0, dy, torch.float64)
    _, g32, dx32 = port_grads(tok, x, state, _cpu(masks), 1.0, dy, torch.float32)
    assert float((y.cpu().double() - y64).abs().max()) <= _tol_y(y64)
    for k, got, a, b in zip(param_keys(2, 2), grads, g64, g32):
        assert_within_bar(got.cpu().double().numpy(), a.numpy(), (b.double() - a).abs().max(), f"p=1 {k}")
    assert_within_bar(dx.cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "p=1 dx")


# ---- 5. determinism -------------------------------------------------------------------------------------------
def test_bitwise_deterministic_across_runs_streams_and_batches(cuda_device):
    B, S, T = 64, 40, 100
    m = train_model(recipe_state(50, N_TOKENS, 2, 2), 0.1, cuda_device)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 51))   # 2560 ids over 50 table rows, mostly 0
    torch.manual_seed(52)
    masks = m._draw_dropout_masks(B, S, T)
    _, g1, dx1 = _step(m, tok, x, dy, masks)
    _, g2, dx2 = _step(m, tok, x, dy, masks)
    s = torch.cuda.Stream(cuda_device)
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        _, g3, dx3 = _step(m, tok, x, dy, masks)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    for a, b, c in zip(g1, g2, g3):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(dx1, dx2) and torch.equal(dx1, dx3)
    for i in (0, 17, 63):                                # dx of a sequence alone == inside the batch
        mi = {k: v[i:i + 1].contiguous() for k, v in masks.items()}
        _, _, dxi = _step(m, tok[i:i + 1], x[i:i + 1], dy[i:i + 1], mi)
        assert torch.equal(dxi[0], dx1[i])


# ---- 6. poisoned outputs, saved buffer and scratch ------------------------------------------------------------
@pytest.mark.parametrize("B,S,T,with_dx", [(3, 9, 17, True), (2, 40, 100, False), (5, 1, 1, True)])
def test_outputs_fully_written_and_scratch_contents_irrelevant(B, S, T, with_dx, cuda_device):
    ne, nd, p = 1, 2, 0.1
    state = recipe_state(60, N_TOKENS, ne, nd)
    m = train_model(state, p, cuda_device)
    lib, _ = m._ensure_created()
    tok, x, dy = _data(B, S, T, N_TOKENS, 61)
    masks = cpu_masks(B, S, T, ne, nd, p, 62)
    tensors = [t.detach().cpu() for t in m._tensors()]
    inputs = dict(tok=tok, x=x, dy=dy)
    inputs.update({f"p{i}": t for i, t in enumerate(tensors)})
    inputs.update({f"m{i}": t for i, t in enumerate(masks.values())})
    outs = {f"g{i}": tuple(t.shape) for i, t in enumerate(tensors)}
    if with_dx:
        outs["dx"] = (B, T, 12, 2)
    outs["y"] = (B, T, 21, 2)
    nsaved, nws = lib.b2h_tpt_train_bytes(m._handle, B, S, T, 0), lib.b2h_tpt_train_bytes(m._handle, B, S, T, 1)
    N = max(B * S, B * T)                                # the formulas of include/b2h.h
    assert nsaved == B * S * (1040 + 4624 * ne + 1024 * nd) + B * T * (1136 + 6688 * nd)
    assert nws == N * 3584 + B * S * 2048 + min(max((N + 127) // 128, 1), 64) * 198144
    vp = ctypes.c_void_p

    def call(q):
        pa = (vp * len(tensors))(*[q[f"p{i}"] for i in range(len(tensors))])
        ma = (vp * len(masks))(*[q[f"m{i}"] for i in range(len(masks))])
        ga = (vp * len(tensors))(*[q[f"g{i}"] for i in range(len(tensors))])
        rc = lib.b2h_tpt_train_forward(m._handle, pa, q["tok"], q["x"], ma, p, q["y"], q["saved"], nsaved, B, S, T, None)
        return rc or lib.b2h_tpt_backward(m._handle, pa, q["tok"], ma, p, q["dy"], q["saved"], nsaved, q.get("dx"), ga,
                                          q["ws"], nws, B, S, T, None)

    res = poisoned_launch(call, inputs, outs, cuda_device, scratch={"saved": nsaved, "ws": nws})
    y64, g64, dx64 = port_grads(tok, x, state, masks, p, dy, torch.float64)
    _, g32, dx32 = port_grads(tok, x, state, masks, p, dy, torch.float32)
    assert float((res["y"].cpu().double() - y64).abs().max()) <= _tol_y(y64)
    keys = param_keys(ne, nd)
    for i, (a, b) in enumerate(zip(g64, g32)):
        assert_within_bar(res[f"g{i}"].cpu().double().numpy(), a.numpy(), (b.double() - a).abs().max(), keys[i])
    if with_dx:
        assert_within_bar(res["dx"].cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "dx")
    unused = sorted(set(range(N_TOKENS)) - set(tok.reshape(-1).tolist()))
    table = res[f"g{keys.index('token_embedding.weight')}"].cpu()
    assert unused and table[unused].view(torch.int32).eq(0).all()   # +0 bits, over the poison


# ---- 7. the reference loop body with Adam, then eval-mode inference on the updated weights -------------------
def test_adam_trajectory_and_inference_after_updates(cuda_device):
    ne, nd, B, S, T, steps, lr = 2, 2, 4, 20, 64, 10, 2e-4
    lengths = [64, 40, 17, 64]
    state = recipe_state(70, N_TOKENS, ne, nd)
    g = torch.Generator().manual_seed(71)
    tok = tokens_with_padding(B, S, N_TOKENS, g)
    x = torch.rand((B, T, 12, 2), generator=g) - 0.5
    target = (torch.rand((B, T, 21, 2), generator=g) - 0.5) * 0.2
    keys = param_keys(ne, nd)
    ref = {}
    for dt in (torch.float64, torch.float32):              # the port's trajectories: the truth and the fp32 reference
        st = leaf_state(state, dt)
        opt = torch.optim.Adam([st[k] for k in keys], lr=lr)
        losses = []
        for _ in range(steps):
            loss = masked_l1(port_forward(tok, x.to(dt), st, {}, 0.0, dt), target.to(dt), lengths)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        ref[dt] = (np.array(losses), {k: st[k].detach().double().numpy() for k in keys})
    m = train_model(state, 0.0, cuda_device)
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    criterion = hps.maskedPoseL1()
    kd, xd, td = tok.to(cuda_device), x.to(cuda_device), target.to(cuda_device)
    losses = []
    for _ in range(steps):                                 # traintest.py:105-121
        prediction = m(kd, xd)
        for i, n in enumerate(lengths):
            prediction[i, n:, :] = 0
        loss = criterion(prediction, td, lengths)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    l64, f64 = ref[torch.float64]
    l32, f32 = ref[torch.float32]
    assert_within_bar(np.array(losses), l64, np.abs(l32 - l64).max(), "losses")
    sd = m.state_dict()
    for k in keys:
        assert_within_bar(sd[k].cpu().double().numpy(), f64[k], np.abs(f32[k] - f64[k]).max(), "final " + k)
    m.eval()                                               # the inference path packs the updated weights
    with torch.no_grad():
        y = m(kd, xd).cpu().double()
    y64 = tpt_ref.Checker(m, torch.float64)(tok, x)
    assert float((y - y64).abs().max()) <= _tol_y(y64)


# ---- 8. unchanged calls ---------------------------------------------------------------------------------------
def test_eval_and_no_grad_calls_unchanged(cuda_device):
    m = train_model(recipe_state(80, N_TOKENS, 1, 1), 0.1, cuda_device)
    tok, x, _ = (t.to(cuda_device) for t in _data(3, 12, 70, N_TOKENS, 81))
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"inference-only.*model\.eval\(\)"):
        m(tok, x)                                          # training mode, p > 0, no_grad: refused as before
    m.eval()
    y_eval = m(tok, x)                                     # eval under grad: the inference kernels
    with torch.no_grad():
        y_nograd = m(tok, x)
    assert y_eval.grad_fn is None and y_nograd.grad_fn is None and torch.equal(y_nograd, y_eval)
    m.train()
    for p in m.parameters():                               # frozen parameters, input requiring a gradient: dx only
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
        m(tok, x)                                          # nothing requires a gradient: the inference path again
    xd = x.clone().requires_grad_(True)
    y = m(tok, xd)
    assert y.grad_fn is not None
    y.sum().backward()
    assert xd.grad is not None and all(p.grad is None for p in m.parameters())


# ---- 9. graph capture -----------------------------------------------------------------------------------------
def test_training_step_captured_in_graph_equals_eager(cuda_device):
    B, S, T = 8, 20, 50
    m = train_model(recipe_state(90, N_TOKENS, 2, 2), 0.1, cuda_device)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 91))
    torch.manual_seed(92)
    masks = m._draw_dropout_masks(B, S, T)
    _, eager_g, eager_dx = _step(m, tok, x, dy, masks)
    xs = x.clone().requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    s = torch.cuda.Stream(cuda_device)                     # warm-up on a side stream, as torch's docs do
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        m._forward_train(tok, xs, masks).backward(dy)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    for p in m.parameters():
        p.grad = None
    xs.grad = None
    with torch.cuda.graph(graph):                          # one stream: no parallel branches
        m._forward_train(tok, xs, masks).backward(dy)
    for p in m.parameters():
        p.grad.fill_(float("nan"))
    xs.grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, p in zip(eager_g, m._tensors()):
        assert torch.equal(a, p.grad)
    assert torch.equal(eager_dx, xs.grad)


# ---- 10. a token id outside the table, on the device ----------------------------------------------------------
def test_out_of_range_device_id_poisons_its_sequence_only(cuda_device):
    B, S, T = 3, 9, 17
    m = train_model(recipe_state(95, N_TOKENS, 1, 2), 0.1, cuda_device)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 96))
    torch.manual_seed(97)
    masks = m._draw_dropout_masks(B, S, T)
    y0, _, dx0 = _step(m, tok, x, dy, masks)
    for bad in (N_TOKENS, -1):
        t = tok.clone()
        t[1, 2] = bad                                      # ids on the device are not checked on the host
        y, grads, dx = _step(m, t, x, dy, masks)           # the backward returns OK
        assert torch.isnan(y[1]).all()
        for i in (0, 2):
            assert torch.equal(y[i], y0[i]) and torch.equal(dx[i], dx0[i])
