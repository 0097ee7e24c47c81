"""TransformerEnc training on the MI355X (kernel_tenc_train.h through b2h_tenc_train_forward / b2h_tenc_backward
and hand_pose_sl_amd's autograd Function).

Accuracy bar, per tensor (train_ref.bar): max|g_gpu - g64| <= 4 * max|g32_ref - g64| + 1e-6 * max|g64|, with g64
float64 autograd (of the reference's own class for the fixtures, of tenc_train_ref.port_forward -- which takes
the very dropout masks the kernels used -- everywhere else) and g32_ref the same computation in float32 on the
CPU.  The forward output is held to test_transformer_enc.py's 2e-5.  The sweep prints the worst ratio
max|g - g64| / max|g32_ref - g64| it saw (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
import oracle
from hand_pose_sl_amd import _lib
from poison import launch as poisoned_launch
from tenc_train_ref import (NAMES, assert_within_bar, leaf_state, load_tenc, masked_l1, param_keys, port_forward,
                            port_grads, seeded_state, tenc_cases)

pytestmark = pytest.mark.gpu
TOL_Y = 2e-5


def _model(nlayers, p, state, dev):
    m = hps.TransformerEnc(24, 4, 128, 42, nlayers, dropout=p)
    if state["pos_encoder.pe"].shape[0] != 100:
        m.pos_encoder = hps.PositionalEncoding(24, p, max_len=state["pos_encoder.pe"].shape[0])
    m.load_state_dict(state)
    return m.to(dev).train()


def _params(m):
    return m._tensors()[1:]


def _grads(m):
    return [p.grad.detach().cpu().double().numpy() for p in _params(m)]


def _cpu(masks):
    return {k: v.cpu() for k, v in masks.items()}


# ---- 1. the reference's fixtures ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tenc_cases())
def test_gradients_match_reference_fixtures(name, cuda_device):
    r = load_tenc(name)
    m = _model(r["nlayers"], 0.0, r["state"], cuda_device)
    x = torch.from_numpy(r["x"]).to(cuda_device).requires_grad_(True)
    target = torch.from_numpy(r["target"]).to(cuda_device)
    lengths = [int(n) for n in r["lengths"]]
    prediction = m(x)
    for i, n in enumerate(lengths):                     # mask_output (steps/utils.py:309-312), in place
        prediction[i, n:, :] = 0
    loss = hps.maskedPoseL1()(prediction, target, lengths)
    assert loss.grad_fn is not None
    loss.backward()
    assert_within_bar(np.array(loss.item()), r["loss64"], abs(float(r["loss32"]) - float(r["loss64"])), f"{name} loss")
    for k, g in zip(param_keys(r["nlayers"]), _grads(m)):
        assert_within_bar(g, r["g64_" + k], r["err32_" + k], f"{name} {k}")
    assert_within_bar(x.grad.cpu().double().numpy(), r["dx64"], r["err32_dx"], f"{name} dx")


# ---- 2. sweep against float64 autograd of the port, with the masks the kernels used --------------------------
SHAPES = [(1, 1), (3, 2), (1, 15), (3, 16), (3, 17), (2, 33), (1, 64), (3, 99), (2, 100), (17, 100)]
LONG = [(2, 101), (1, 113), (2, 128)]                   # with a max_len = 128 table
WORST = {"ratio": 0.0, "what": "", "y": 0.0}


def _check_case(state, nlayers, p, B, T, scale, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, T, 12, 2), generator=g) * scale
    dy = torch.randn((B, T, 21, 2), generator=g)
    m = _model(nlayers, p, state, dev)
    torch.manual_seed(seed)
    masks = m._draw_dropout_masks(B, T)
    assert bool(masks) == (p > 0)
    xd = x.to(dev).requires_grad_(True)
    y = m._forward_train(xd, masks)
    y.backward(dy.to(dev))
    cm = _cpu(masks)
    y64, g64, dx64 = port_grads(x, state, cm, p, dy, torch.float64)
    _, g32, dx32 = port_grads(x, state, cm, p, dy, torch.float32)
    what = f"L={nlayers} p={p} B={B} T={T} scale={scale:.2g}"
    err_y = float((y.detach().cpu().double() - y64).abs().max())
    WORST["y"] = max(WORST["y"], err_y)
    assert err_y <= TOL_Y * max(1.0, float(y64.abs().max())), f"{what}: y {err_y:.3e}"
    todo = [(k, gg, a.numpy(), b.double().numpy()) for k, gg, a, b in zip(param_keys(nlayers), _grads(m), g64, g32)]
    todo.append(("dx", xd.grad.cpu().double().numpy(), dx64.numpy(), dx32.double().numpy()))
    for k, got, a, b in todo:
        err32 = np.abs(b - a).max()
        if err32 > 0:
            ratio = float(np.abs(got - a).max() / err32)
            if ratio > WORST["ratio"]:
                WORST.update(ratio=ratio, what=f"{what} {k}")
        assert_within_bar(got, a, err32, f"{what} {k}")


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("nlayers", [1, 4])
def test_sweep_against_float64_autograd(nlayers, p, cuda_device):
    state = seeded_state(nlayers, 100 + nlayers)
    for j, (B, T) in enumerate(SHAPES):
        _check_case(state, nlayers, p, B, T, 1.0 if j % 2 else 1.0 / 1280, 1000 + 97 * nlayers + j, cuda_device)
    state = seeded_state(nlayers, 100 + nlayers, max_len=128)
    for j, (B, T) in enumerate(LONG):
        _check_case(state, nlayers, p, B, T, 1.0 / 1280 if j % 2 else 1.0, 2000 + 97 * nlayers + j, cuda_device)
    print(f"\nsweep L={nlayers} p={p}: worst ratio so far {WORST['ratio']:.3f} ({WORST['what']}), worst y error {WORST['y']:.3e}")


def test_sweep_with_randomized_layernorm_and_attention_biases(cuda_device):
    """The default init leaves gamma = 1, beta = 0 and the attention biases 0: a kernel that dropped one would pass."""
    state = seeded_state(2, 31)
    g = torch.Generator().manual_seed(32)
    for k, v in state.items():
        if "norm" in k and k.endswith("weight"):
            v.copy_(1.0 + 0.5 * (torch.rand(v.shape, generator=g) - 0.5))
        elif "norm" in k or k.endswith("in_proj_bias") or k.endswith("out_proj.bias"):
            v.copy_(0.5 * torch.randn(v.shape, generator=g))
    for j, (B, T) in enumerate([(3, 17), (2, 100)]):
        _check_case(state, 2, 0.1, B, T, 1.0, 3000 + j, cuda_device)


# ---- 3. dropout behaviour -------------------------------------------------------------------------------------
def _step(m, x, dy, masks=None):
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(True)
    y = m(xd) if masks is None else m._forward_train(xd, masks)
    y.backward(dy)
    return y.detach().clone(), [p.grad.clone() for p in _params(m)], xd.grad.clone()


def test_dropout_follows_the_seed_and_the_given_masks(cuda_device):
    B, T, p = 3, 37, 0.1
    m = _model(2, p, seeded_state(2, 40), cuda_device)
    g = torch.Generator().manual_seed(41)
    x = torch.randn((B, T, 12, 2), generator=g).to(cuda_device)
    dy = torch.randn((B, T, 21, 2), generator=g).to(cuda_device)
    torch.manual_seed(7)
    y1, g1, dx1 = _step(m, x, dy)
    torch.manual_seed(7)
    y2, g2, dx2 = _step(m, x, dy)
    torch.manual_seed(7)
    masks = m._draw_dropout_masks(B, T)
    y3, g3, dx3 = _step(m, x, dy, masks)
    assert torch.equal(y1, y2) and torch.equal(y1, y3) and torch.equal(dx1, dx2) and torch.equal(dx1, dx3)
    for a, b, c in zip(g1, g2, g3):
        assert torch.equal(a, b) and torch.equal(a, c)
    torch.manual_seed(8)
    assert not torch.equal(_step(m, x, dy)[0], y1)
    # the documented order and shapes
    keys = ["pos"] + [(l, n) for l in range(2) for n in NAMES]
    assert list(masks) == keys
    assert masks["pos"].shape == (B, T, 24) and masks[(1, "attn")].shape == (B, 4, T, T) and masks[(0, "ff")].shape == (B, T, 128)
    assert all(v.dtype == torch.uint8 and v.device.type == "cuda" for v in masks.values())


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_keep_rates(p, cuda_device):
    m = _model(2, p, seeded_state(2, 42), cuda_device)
    torch.manual_seed(9)
    for k, v in m._draw_dropout_masks(16, 100).items():
        assert int(v.max()) <= 1
        sigma = (p * (1 - p) / v.numel()) ** 0.5
        assert abs(float(v.float().mean()) - (1 - p)) <= 5 * sigma, k


def test_p0_equals_eval_and_p1_drops_everything(cuda_device):
    state = seeded_state(2, 43)
    g = torch.Generator().manual_seed(44)
    x = torch.randn((3, 17, 12, 2), generator=g)
    dy = torch.randn((3, 17, 21, 2), generator=g)
    m = _model(2, 0.0, state, cuda_device)
    assert m._draw_dropout_masks(3, 17) == {}
    y_train = m(x.to(cuda_device))
    assert y_train.grad_fn is not None
    with torch.no_grad():
        y_eval = m.eval()(x.to(cuda_device))
    assert float((y_train.detach() - y_eval).abs().max()) <= TOL_Y
    m = _model(2, 1.0, state, cuda_device)
    torch.manual_seed(1)
    masks = m._draw_dropout_masks(3, 17)
    assert not any(bool(v.any()) for v in masks.values())
    y, grads, dx = _step(m, x.to(cuda_device), dy.to(cuda_device), masks)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all() and all(torch.isfinite(t).all() for t in grads)
    y64, g64, dx64 = port_grads(x, state, _cpu(masks), 1.0, dy, torch.float64)
    _, g32, dx32 = port_grads(x, state, _cpu(masks), 1.0, dy, torch.float32)
    assert float((y.cpu().double() - y64).abs().max()) <= TOL_Y * max(1.0, float(y64.abs().max()))
    for k, got, a, b in zip(param_keys(2), grads, g64, g32):
        assert_within_bar(got.cpu().double().numpy(), a.numpy(), (b.double() - a).abs().max(), f"p=1 {k}")
    assert_within_bar(dx.cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "p=1 dx")


# ---- 4. determinism -------------------------------------------------------------------------------------------
def test_bitwise_deterministic_across_runs_streams_and_batches(cuda_device):
    B, T = 64, 100
    m = _model(2, 0.1, seeded_state(2, 50), cuda_device)
    g = torch.Generator().manual_seed(51)
    x = torch.randn((B, T, 12, 2), generator=g).to(cuda_device)
    dy = torch.randn((B, T, 21, 2), generator=g).to(cuda_device)
    torch.manual_seed(52)
    masks = m._draw_dropout_masks(B, T)
    _, g1, dx1 = _step(m, x, dy, masks)
    _, g2, dx2 = _step(m, x, dy, masks)
    s = torch.cuda.Stream(cuda_device)
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        _, g3, dx3 = _step(m, x, dy, masks)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    for a, b, c in zip(g1, g2, g3):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(dx1, dx2) and torch.equal(dx1, dx3)
    for i in (0, 17, 63):                                # dx of a sequence alone == inside the batch
        mi = {k: v[i:i + 1].contiguous() for k, v in masks.items()}
        _, _, dxi = _step(m, x[i:i + 1], dy[i:i + 1], mi)
        assert torch.equal(dxi[0], dx1[i])


# ---- 5. poisoned outputs, saved buffer and scratch ------------------------------------------------------------
@pytest.mark.parametrize("B,T,with_dx", [(3, 17, True), (2, 100, False), (5, 1, True)])
def test_outputs_fully_written_and_scratch_contents_irrelevant(B, T, with_dx, cuda_device):
    L, p = 2, 0.1
    state = seeded_state(L, 60)
    m = _model(L, p, state, cuda_device)
    lib, _ = m._ensure_created()
    g = torch.Generator().manual_seed(61)
    x = torch.randn((B, T, 12, 2), generator=g)
    dy = torch.randn((B, T, 21, 2), generator=g)
    masks = {"pos": (torch.rand((B, T, 24), generator=g) >= p).to(torch.uint8)}
    for l in range(L):
        masks[(l, "attn")] = (torch.rand((B, 4, T, T), generator=g) >= p).to(torch.uint8)
        for n in NAMES[1:]:
            masks[(l, n)] = (torch.rand((B, T, 128), generator=g) >= p).to(torch.uint8)
    tensors = [t.detach().cpu() for t in m._tensors()]
    inputs = dict(x=x, dy=dy)
    inputs.update({f"p{i}": t for i, t in enumerate(tensors)})
    inputs.update({f"m{i}": t for i, t in enumerate(masks.values())})
    outs = {f"g{i}": tuple(t.shape) for i, t in enumerate(tensors[1:])}
    if with_dx:
        outs["dx"] = (B, T, 12, 2)
    outs["y"] = (B, T, 21, 2)
    nsaved, nws = lib.b2h_tenc_train_bytes(m._handle, B, T, 0), lib.b2h_tenc_train_bytes(m._handle, B, T, 1)
    assert nsaved == B * T * (608 + 4624 * L) and nws > 0
    vp = ctypes.c_void_p

    def call(q):
        pa = (vp * len(tensors))(*[q[f"p{i}"] for i in range(len(tensors))])
        ma = (vp * len(masks))(*[q[f"m{i}"] for i in range(len(masks))])
        ga = (vp * (len(tensors) - 1))(*[q[f"g{i}"] for i in range(len(tensors) - 1)])
        rc = lib.b2h_tenc_train_forward(m._handle, pa, q["x"], ma, p, q["y"], q["saved"], nsaved, B, T, None)
        return rc or lib.b2h_tenc_backward(m._handle, pa, ma, p, q["dy"], q["saved"], nsaved, q.get("dx"), ga, q["ws"],
                                           nws, B, T, None)

    res = poisoned_launch(call, inputs, outs, cuda_device, scratch={"saved": nsaved, "ws": nws})
    y64, g64, dx64 = port_grads(x, state, masks, p, dy, torch.float64)
    _, g32, dx32 = port_grads(x, state, masks, p, dy, torch.float32)
    assert float((res["y"].cpu().double() - y64).abs().max()) <= TOL_Y * max(1.0, float(y64.abs().max()))
    for i, (a, b) in enumerate(zip(g64, g32)):
        assert_within_bar(res[f"g{i}"].cpu().double().numpy(), a.numpy(), (b.double() - a).abs().max(), f"g{i}")
    if with_dx:
        assert_within_bar(res["dx"].cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "dx")


# ---- 6. the reference loop body with Adam, then eval-mode inference on the updated weights -------------------
def test_adam_trajectory_and_inference_after_updates(cuda_device):
    L, B, T, steps, lr = 2, 4, 64, 10, 2e-4
    lengths = [64, 40, 17, 64]
    state = seeded_state(L, 70)
    g = torch.Generator().manual_seed(71)
    x = torch.rand((B, T, 12, 2), generator=g) - 0.5
    target = (torch.rand((B, T, 21, 2), generator=g) - 0.5) * 0.2
    keys = param_keys(L)
    ref = {}
    for dt in (torch.float64, torch.float32):              # the port's trajectories: the truth and the fp32 reference
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
    m = _model(L, 0.0, state, cuda_device)
    m.eval()
    with torch.no_grad():
        m(x.to(cuda_device))                               # packs the initial weights (inference path)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    criterion = hps.maskedPoseL1()
    xd, td = x.to(cuda_device), target.to(cuda_device)
    losses = []
    for _ in range(steps):                                 # traintest.py:94-121
        prediction = m(xd)
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
    m.eval()                                               # the inference path repacks after the in-place updates
    with torch.no_grad():
        y = m(xd).cpu().numpy()
    want = oracle.transformer_forward(x.numpy(), {k: v.cpu().numpy() for k, v in sd.items()})
    assert np.abs(y - want).max() <= TOL_Y


# ---- 7. unchanged calls ---------------------------------------------------------------------------------------
def test_eval_and_no_grad_calls_unchanged(cuda_device):
    m = _model(2, 0.1, seeded_state(2, 80), cuda_device)
    x = (torch.rand((3, 70, 12, 2), generator=torch.Generator().manual_seed(81)) - 0.5).to(cuda_device)
    with torch.no_grad():
        y_nograd = m(x)                                    # training mode, no_grad: the inference kernels, no dropout
    m.eval()
    y_eval = m(x)
    assert y_eval.grad_fn is None and y_nograd.grad_fn is None and torch.equal(y_nograd, y_eval)
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        m.forward_fused(x)
    with torch.no_grad():
        m.forward_fused(x)
    for p in m.parameters():                               # frozen parameters, input requiring a gradient: dx only
        p.requires_grad_(False)
    assert m(x).grad_fn is None
    xd = x.clone().requires_grad_(True)
    y = m(xd)
    assert y.grad_fn is not None
    y.sum().backward()
    assert xd.grad is not None and all(p.grad is None for p in m.parameters())


# ---- 8. graph capture -----------------------------------------------------------------------------------------
def test_training_step_captured_in_graph_equals_eager(cuda_device):
    B, T = 8, 50
    m = _model(2, 0.1, seeded_state(2, 90), cuda_device)
    g = torch.Generator().manual_seed(91)
    x = torch.randn((B, T, 12, 2), generator=g).to(cuda_device)
    dy = torch.randn((B, T, 21, 2), generator=g).to(cuda_device)
    torch.manual_seed(92)
    masks = m._draw_dropout_masks(B, T)
    _, eager_g, eager_dx = _step(m, x, dy, masks)
    xs = x.clone().requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    s = torch.cuda.Stream(cuda_device)                     # warm-up on a side stream, as torch's docs do
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        m._forward_train(xs, masks).backward(dy)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    for p in m.parameters():
        p.grad = None
    xs.grad = None
    with torch.cuda.graph(graph):
        m._forward_train(xs, masks).backward(dy)
    for p in m.parameters():
        p.grad.fill_(float("nan"))
    xs.grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, p in zip(eager_g, _params(m)):
        assert torch.equal(a, p.grad)
    assert torch.equal(eager_dx, xs.grad)


# ---- 9. trained-like weights: the state of tests/golden/tenc_params.npz ---------------------------------------
# Every parameter non-default, layer 1's heads 0 and 1 peaked (logits ~30), head 3 with every real-key logit <= -20
# (test_tenc_params.py has it for inference).  The draws are chosen on the CPU ports alone, by the rules of the
# TextPoseTransformer stress tests (tests/tpt_stress_ref.py): no float64 ReLU input closer to zero than RELU_MARGIN times
# the float32 port's largest rounding of any, and the float32 port's own gradients within CAP_G32 of float64 per
# tensor, so that the relative bar stays sharp.  Measured on the CPU: the float32 port is 1e-6 .. 2e-6 off in y and
# 1e-6 .. 3e-6 (relative) in the gradients at both shapes and both p, and every draw of 8 keeps the margin.  The
# file's near-eps LayerNorm variant (`lnvar__*`) stays out: its float32 port is 7e-4 .. 7e-2 off in the gradients and
# no draw of 8 keeps the margin (2e-3 of rounding in every ReLU input of layer 1).
RELU_MARGIN, CAP_G32 = 2.0, 1e-3


def _watched(fn, name):
    """fn() with torch.nn.functional.relu or torch.softmax watched: (result, float64 copies of its first arguments)."""
    import torch.nn.functional as F
    mod = F if name == "relu" else torch
    seen, real = [], getattr(mod, name)

    def watched(h, *a, **kw):
        seen.append(h.detach().double())
        return real(h, *a, **kw)
    setattr(mod, name, watched)
    try:
        return fn(), seen
    finally:
        setattr(mod, name, real)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T", [(3, 17), (2, 100)])
def test_gradients_under_peaked_attention_and_nondefault_params(B, T, p, cuda_device):
    from test_tenc_params import _fixture
    state = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in _fixture()[0].items()}
    m = _model(2, p, state, cuda_device)
    keys = param_keys(2) + ["dx"]
    for attempt in range(16):                              # the inputs are chosen on the CPU ports alone
        g = torch.Generator().manual_seed(4000 + T + 100000 * attempt)
        x = torch.rand((B, T, 12, 2), generator=g) - 0.5   # the scale of the fixture's inputs, which set the logits
        dy = torch.randn((B, T, 21, 2), generator=g)
        torch.manual_seed(4000 + T + 100000 * attempt)
        masks = m._draw_dropout_masks(B, T)
        assert bool(masks) == (p > 0)
        cm = _cpu(masks)
        (y64, g64, dx64), pre64 = _watched(lambda: port_grads(x, state, cm, p, dy, torch.float64), "relu")
        (y32, g32, dx32), pre32 = _watched(lambda: port_grads(x, state, cm, p, dy, torch.float32), "relu")
        pre64, pre32 = (torch.cat([t.reshape(-1) for t in pre]) for pre in (pre64, pre32))
        nearest, rounding = float(pre64.abs().min()), float((pre32 - pre64).abs().max())
        rel = max((float((b.double() - a).abs().max() / a.abs().max()), k) for k, a, b in zip(keys, g64 + [dx64], g32 + [dx32]))
        # the regime, on the float64 port (what make_golden.py:tenc_params_case built): layer 1's heads 0 and 1 reach
        # logits beyond 20, head 3's real keys all lie below -20
        _, scores = _watched(lambda: port_forward(x.double(), {k: v.double() for k, v in state.items()}, cm, p, torch.float64),
                             "softmax")
        peak, top3 = float(scores[1][:, :2].abs().max()), float(scores[1][:, 3].max())
        admitted = nearest >= RELU_MARGIN * rounding and rel[0] <= CAP_G32 and peak >= 20.0 and top3 <= -20.0
        print(f"\ndraw {attempt}: a ReLU input at {nearest:.2e} from zero, fp32 rounding {rounding:.2e}, float32 gradients {rel}; "
              f"layer 1: max |logit| of heads 0, 1 {peak:.1f}, mean row-maximum probability "
              f"{float(torch.softmax(scores[1][:, :2], -1).max(-1).values.mean()):.2f}; head 3 max logit {top3:.1f}")
        if admitted:
            break
    assert admitted
    xd = x.to(cuda_device).requires_grad_(True)
    y = m._forward_train(xd, masks)
    y.backward(dy.to(cuda_device))
    what = f"tenc_params p={p} B={B} T={T}"
    err32_y = float((y32.double() - y64).abs().max())
    bar_y = max(TOL_Y * max(1.0, float(y64.abs().max())), 4 * err32_y)   # the rule of test_tenc_params.py, k = 4
    err_y = float((y.detach().cpu().double() - y64).abs().max())
    worst = (0.0, "")
    for k, got, a, b in zip(keys, _grads(m) + [xd.grad.cpu().double().numpy()], g64 + [dx64], g32 + [dx32]):
        err32 = float((b.double() - a).abs().max())
        worst = max(worst, (float(np.abs(got - a.numpy()).max()) / max(err32, 1e-300), k))
    print(f"\n{what}: y error {err_y:.3e} (bar {bar_y:.3e}, float32 port {err32_y:.3e}); worst max|g - g64| / max|g32 - g64| "
          f"{worst[0]:.3f} ({worst[1]}); float32 port's worst gradient error {rel[0]:.2e} of the maximum ({rel[1]})")
    assert err_y <= bar_y, f"{what}: y {err_y:.3e} > bar {bar_y:.3e}"
    for k, got, a, b in zip(keys, _grads(m) + [xd.grad.cpu().double().numpy()], g64 + [dx64], g32 + [dx32]):
        assert_within_bar(got, a.numpy(), float((b.double() - a).abs().max()), f"{what} {k}")
