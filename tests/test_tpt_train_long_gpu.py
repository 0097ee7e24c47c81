"""TextPoseTransformer training beyond 128 frames on the MI355X: the blocked attention kernels of
kernel_train_attn_long.h (query blocks of QB = 64 rows, key blocks of KB = 128 rows, an online softmax that saves each
row's log-sum-exp, a key-owner and a query-owner backward) through b2h_tpt_train_forward / b2h_tpt_backward and the
autograd Function, at the trainer's default of 200 frames and up to 1024.

The bars are those of test_tpt_train_gpu.py (tpt_train_ref.assert_within_bar): per tensor
max|g - g64| <= 4 * max|g32_ref - g64| + 1e-6 * max|g64|, with g64 float64 autograd of tpt_train_ref.port_forward
(which takes the very dropout masks the kernels used; of the reference's own class for the fixture) and g32_ref the
same computation in float32 on the CPU; the forward output is held to tpt_ref.BAR * max(1, max|y64|).  The sweep
prints the worst ratio max|g - g64| / max|g32_ref - g64| and the worst y error it has seen so far (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
import tpt_geom_ref
import tpt_ref
from poison import launch as poisoned_launch
from tpt_train_ref import (assert_within_bar, cpu_masks, leaf_state, load_train, masked_l1, param_keys, port_forward,
                           port_grads, recipe_state, tokens_with_padding, train_model)

pytestmark = pytest.mark.gpu
N_TOKENS = 50
LONG_CASE = "long_train_e2_d2_b2_s40_t200"
QB, KB = 64, 128                                        # kLtQb, kLtKb of kernel_train_attn_long.h


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


def _step(m, tok, x, dy, masks=None):
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(True)
    y = m(tok, xd) if masks is None else m._forward_train(tok, xd, masks)
    y.backward(dy)
    return y.detach().clone(), [p.grad.clone() for p in m._tensors()], xd.grad.clone()


# ---- 1. the reference's fixture at the trainer's length ----------------------------------------------------------
def test_gradients_match_reference_fixture_at_200_frames(cuda_device):
    r = load_train(LONG_CASE)
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
    assert_within_bar(np.array(loss.item()), r["loss64"], abs(float(r["loss32"]) - float(r["loss64"])), "loss")
    stored = 0
    for k, g in zip(param_keys(r["n_enc"], r["n_dec"]), _grads(m)):
        if "g64_" + k in r:
            assert_within_bar(g, r["g64_" + k], r["err32_" + k], k)
            stored += 1
    assert stored >= 30
    assert_within_bar(x.grad.cpu().double().numpy(), r["dx64"], r["err32_dx"], "dx")


# ---- 2. sweep against float64 autograd of the port, with the masks the kernels used ------------------------------
# The issue's six shapes, then T on both sides of every multiple of QB and KB between 128 and two full key blocks plus
# a partial one: 129 = KB + 1 = 2 QB + 1 and 257 = 2 KB + 1 = 4 QB + 1 are among the six; 3 QB -+ 1 and 2 KB - 1, 2 KB here.
SHAPES = [(2, 1, 129), (2, 17, 130), (1, 128, 129), (2, 40, 200), (1, 40, 257), (3, 33, 144),
          (1, 9, 3 * QB - 1), (1, 9, 3 * QB), (1, 9, 3 * QB + 1), (1, 9, 2 * KB - 1), (1, 9, 2 * KB)]
WORST = {"ratio": 0.0, "what": "", "y": 0.0}
# The model's gradient jumps where a ReLU input crosses zero, and fp32 cannot tell the side of an input that lies closer
# to zero than its own rounding (128-term sums of O(1) products: a few 1e-6).  Such a draw has no gradient to fp32
# accuracy: the float32 port itself then errs by 1e-3 of the gradient, a thousand times its usual error, in whichever
# unit it flips, and another summation order flips another unit.  So the sweep measures the rounding on the reference
# alone -- the largest difference between the float32 and the float64 port over all ReLU inputs of the draw -- and takes
# the first seed whose float64 ReLU inputs all stay further from zero than RELU_MARGIN times that.
RELU_MARGIN = 2.0


def _port_grads_and_relu_inputs(tok, x, state, masks, p, dy, dtype):
    """port_grads in `dtype` and the inputs of every ReLU of that forward (float64 copies)."""
    import torch.nn.functional as F
    seen, relu = [], F.relu

    def watched(h, *a, **kw):
        seen.append(h.detach().double().reshape(-1))
        return relu(h, *a, **kw)
    F.relu = watched
    try:
        return port_grads(tok, x, state, masks, p, dy, dtype), torch.cat(seen)
    finally:
        F.relu = relu


def _check_case(state, p, B, S, T, scale, seed, dev, x=None, inputs=None, admit=None, y_bar=None, also32=None):
    """One training step on `dev` against float64 autograd of the port.  The keywords (tests/test_tpt_stress_gpu.py)
    default to what this function has always done: `inputs(attempt)` -> (tokens, x) replaces the draw's tokens and
    poses; `admit(tokens, x, y64, y32, g64, g32)` -> None, or the reason why the CPU ports refuse the draw (gradients
    in param_keys order, then dx), a further condition on the draw beside the ReLU margin; `y_bar(y64, y32)` -> the
    bar on max|y - y64| in place of the fixed _tol_y; `also32`, a second float32 CPU port with port_grads' signature:
    a tensor's err32 is then the larger of the two ports' errors."""
    n_tokens = state["token_embedding.weight"].shape[0]
    m = train_model(state, p, dev)
    for attempt in range(16):                           # the inputs are chosen on the CPU ports alone
        tok, xr, dy = _data(B, S, T, n_tokens, seed + 100000 * attempt, scale)
        xr = xr if x is None else x
        if inputs is not None:
            tok, xr = inputs(attempt)
        torch.manual_seed(seed + 100000 * attempt)
        masks = m._draw_dropout_masks(B, S, T)
        assert bool(masks) == (p > 0)
        cm = _cpu(masks)
        (y64, g64, dx64), pre64 = _port_grads_and_relu_inputs(tok, xr, state, cm, p, dy, torch.float64)
        (y32, g32, dx32), pre32 = _port_grads_and_relu_inputs(tok, xr, state, cm, p, dy, torch.float32)
        nearest, rounding = float(pre64.abs().min()), float((pre32 - pre64).abs().max())
        refused = None if admit is None else admit(tok, xr, y64, y32, g64 + [dx64], g32 + [dx32])
        if nearest >= RELU_MARGIN * rounding and refused is None:
            break
        print(f"\nseed {seed + 100000 * attempt}: a ReLU input at {nearest:.2e} from zero, fp32 rounding {rounding:.2e}"
              f"{'' if refused is None else '; ' + refused}: next draw")
    assert nearest >= RELU_MARGIN * rounding and refused is None, refused
    tol_y = _tol_y(y64) if y_bar is None else y_bar(y64, y32)
    x = xr
    xd = x.to(dev).requires_grad_(True)
    y = m._forward_train(tok.to(dev), xd, masks)
    y.backward(dy.to(dev))
    n_enc, n_dec = m._geom[5], m._geom[6]
    what = f"L=({n_enc},{n_dec}) p={p} B={B} S={S} T={T} scale={scale:.2g}"
    err_y = float((y.detach().cpu().double() - y64).abs().max())
    WORST["y"] = max(WORST["y"], err_y)
    WORST["y_ratio"] = max(WORST.get("y_ratio", 0.0), err_y / tol_y)
    print(f"\n{what}: y error {err_y:.3e} (bar {tol_y:.3e})")
    assert err_y <= tol_y, f"{what}: y {err_y:.3e} > bar {tol_y:.3e}"
    keys = param_keys(n_enc, n_dec)
    got = _grads(m)
    ports32 = [g32 + [dx32]]
    if also32 is not None:
        _, ga, dxa = also32(tok, x, state, cm, p, dy, torch.float32)
        ports32.append(ga + [dxa])
    todo = [(k, gg, a.numpy(), max(float((b[i].double() - a).abs().max()) for b in ports32))
            for i, (k, gg, a) in enumerate(zip(keys + ["dx"], got + [xd.grad.cpu().double().numpy()], g64 + [dx64]))]
    worst_here = (0.0, "")
    for k, gg, a, err32 in todo:
        if err32 > 0:
            ratio = float(np.abs(gg - a).max() / err32)
            worst_here = max(worst_here, (ratio, k))
            if ratio > WORST["ratio"]:
                WORST.update(ratio=ratio, what=f"{what} {k}")
    print(f"{what}: worst ratio {worst_here[0]:.3f} ({worst_here[1]}); so far {WORST['ratio']:.3f} ({WORST['what']}), "
          f"worst y error {WORST['y']:.3e}")
    for k, gg, a, err32 in todo:
        assert_within_bar(gg, a, err32, f"{what} {k}")
    unused = sorted(set(range(n_tokens)) - set(tok.reshape(-1).tolist()))
    table = got[keys.index("token_embedding.weight")]
    assert not table[unused].any()                      # rows of ids the batch does not contain: exactly zero
    return unused


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d_s%d_t%d" % s)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("layers", [(1, 1), (2, 3)], ids=lambda l: "e%d_d%d" % l)
def test_sweep_against_float64_autograd(layers, p, shape, cuda_device):
    state = recipe_state(100 + 10 * layers[0] + layers[1], N_TOKENS, *layers)   # non-default biases and LayerNorms
    j = SHAPES.index(shape)
    unused = _check_case(state, p, *shape, 1.0 if j % 2 else 1.0 / 1280, 5000 + 97 * layers[1] + j, cuda_device)
    assert N_TOKENS - 1 in unused                       # at least one id is never used


def test_sweep_at_the_frame_limit(cuda_device):
    _check_case(recipe_state(111, N_TOKENS, 1, 1), 0.1, 1, 16, 1024, 1.0, 5100, cuda_device)


# ---- 3. the running maximum moves: every row's largest score lies in a later key block than the first -------------
def test_row_maximum_in_a_later_key_block(cuda_device):
    """A pose ramp x_t = v + (t / T) u + noise.  The first self-attention sees h_t = W x_t + b unnormalised, so with a
    large constant v every query is close to q = Wq (W v + b) + bq and the score of key j grows by
    (t_j / T) q_h . Wk_h W u / sqrt(32) in head h.  u solves q_h . Wk_h W u = 80 for all four heads (a 4 x 24 system,
    from the weights alone), so every row's scores rise by about 14 from the first key to the last: the running maximum
    moves in every key block and the online softmax rescales its sums, forward and backward.  That every row of
    every head peaks behind the first block is checked on the float64 port before the kernels run."""
    B, S, T = 1, 9, 2 * KB + 44
    state = recipe_state(111, N_TOKENS, 1, 1)
    st = {k: v.double() for k, v in state.items()}
    g = torch.Generator().manual_seed(5200)
    tok = tokens_with_padding(B, S, N_TOKENS, g)
    v = 5.0 * torch.randn((24,), generator=g).double()
    W, b = st["pose2hidden_projection.weight"], st["pose2hidden_projection.bias"]
    ipw, ipb = (st["transformer.decoder.layers.0.self_attn.in_proj_" + n] for n in ("weight", "bias"))
    q = ipw[:128] @ (W @ v + b) + ipb[:128]
    G = torch.stack([W.T @ ipw[128 + 32 * h:160 + 32 * h].T @ q[32 * h:32 * h + 32] for h in range(4)])
    u = torch.linalg.pinv(G) @ torch.full((4,), 80.0, dtype=torch.float64)
    ramp = torch.arange(T, dtype=torch.float64).reshape(1, T, 1) / T
    x = (v + ramp * u + 0.05 * torch.randn((B, T, 24), generator=g).double()).reshape(B, T, 12, 2).float()
    trace = {}
    port_forward(tok, x.double(), st, {}, 0.0, torch.float64, trace)
    probs = trace[("dec", 0, "self_probs")]
    assert bool((probs.argmax(-1) >= KB).all())         # a property of the input, on the float64 port
    assert float(probs.max(-1).values.mean()) > 5.0 / T  # and the rows are far from uniform
    _check_case(state, 0.1, B, S, T, 1.0, 5201, cuda_device, x=x)


# ---- 4. the other geometries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_joints,nout", [(8, 42), (29, 8)])
def test_geometries(n_joints, nout, cuda_device):
    B, S, T, p = 2, 40, 130, 0.1
    state = tpt_geom_ref.recipe_state(120 + n_joints, N_TOKENS, n_joints, nout, 1, 2)
    m = tpt_geom_ref.train_model(state, p, cuda_device)
    g = torch.Generator().manual_seed(5300 + n_joints)
    tok = tokens_with_padding(B, S, N_TOKENS, g)
    x = torch.randn((B, T, n_joints, 2), generator=g)
    dy = torch.randn((B, T, nout // 2, 2), generator=g)
    torch.manual_seed(5301)
    masks = m._draw_dropout_masks(B, S, T)
    xd = x.to(cuda_device).requires_grad_(True)
    y = m._forward_train(tok.to(cuda_device), xd, masks)
    y.backward(dy.to(cuda_device))
    y64, g64, dx64 = tpt_geom_ref.port_grads(tok, x, state, _cpu(masks), p, dy, torch.float64)
    _, g32, dx32 = tpt_geom_ref.port_grads(tok, x, state, _cpu(masks), p, dy, torch.float32)
    assert float((y.detach().cpu().double() - y64).abs().max()) <= _tol_y(y64)
    for k, gg, a, b in zip(param_keys(1, 2), _grads(m), g64, g32):
        assert_within_bar(gg, a.numpy(), (b.double() - a).abs().max(), f"({n_joints},{nout}) {k}")
    assert_within_bar(xd.grad.cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "dx")


# ---- 5. determinism ---------------------------------------------------------------------------------------------------
def test_bitwise_deterministic_across_runs_streams_and_batches(cuda_device):
    B, S, T = 8, 40, 200
    m = train_model(recipe_state(50, N_TOKENS, 2, 2), 0.1, cuda_device)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 5400))
    torch.manual_seed(5401)
    masks = m._draw_dropout_masks(B, S, T)
    y1, g1, dx1 = _step(m, tok, x, dy, masks)
    y2, g2, dx2 = _step(m, tok, x, dy, masks)
    s = torch.cuda.Stream(cuda_device)
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        y3, g3, dx3 = _step(m, tok, x, dy, masks)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    for a, b, c in zip(g1, g2, g3):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(y1, y2) and torch.equal(y1, y3) and torch.equal(dx1, dx2) and torch.equal(dx1, dx3)
    pick = torch.tensor([7, 0, 3], device=cuda_device)  # the same sequences inside another batch, in another order
    mi = {k: v[pick].contiguous() for k, v in masks.items()}
    yi, _, dxi = _step(m, tok[pick], x[pick], dy[pick], mi)
    assert torch.equal(yi, y1[pick]) and torch.equal(dxi, dx1[pick])


# ---- 6. poisoned outputs, saved buffer and scratch ---------------------------------------------------------------
@pytest.mark.parametrize("with_dx", [True, False])
def test_outputs_fully_written_and_scratch_contents_irrelevant(with_dx, cuda_device):
    B, S, T = 2, 9, 130
    ne, nd, p = 1, 2, 0.1
    state = recipe_state(60, N_TOKENS, ne, nd)
    m = train_model(state, p, cuda_device)
    lib, _ = m._ensure_created()
    tok, x, dy = _data(B, S, T, N_TOKENS, 5500)
    masks = cpu_masks(B, S, T, ne, nd, p, 5501)
    tensors = [t.detach().cpu() for t in m._tensors()]
    inputs = dict(tok=tok, x=x, dy=dy)
    inputs.update({f"p{i}": t for i, t in enumerate(tensors)})
    inputs.update({f"m{i}": t for i, t in enumerate(masks.values())})
    outs = {f"g{i}": tuple(t.shape) for i, t in enumerate(tensors)}
    if with_dx:
        outs["dx"] = (B, T, 12, 2)
    outs["y"] = (B, T, 21, 2)
    nsaved, nws = lib.b2h_tpt_train_bytes(m._handle, B, S, T, 0), lib.b2h_tpt_train_bytes(m._handle, B, S, T, 1)
    N = max(B * S, B * T)                                # the formulas of include/b2h.h, with the terms of T > 128
    assert nsaved == B * S * (1040 + 4624 * ne + 1024 * nd) + B * T * (1136 + 6688 * nd) + B * T * 32 * nd
    assert nws == N * 3584 + B * S * 2048 + min(max((N + 127) // 128, 1), 64) * 198144 + B * T * 32
    vp = ctypes.c_void_p

    def call(q, saved_bytes=nsaved, ws_bytes=nws):
        pa = (vp * len(tensors))(*[q[f"p{i}"] for i in range(len(tensors))])
        ma = (vp * len(masks))(*[q[f"m{i}"] for i in range(len(masks))])
        ga = (vp * len(tensors))(*[q[f"g{i}"] for i in range(len(tensors))])
        rc = lib.b2h_tpt_train_forward(m._handle, pa, q["tok"], q["x"], ma, p, q["y"], q["saved"], saved_bytes, B, S, T, None)
        return rc or lib.b2h_tpt_backward(m._handle, pa, q["tok"], ma, p, q["dy"], q["saved"], nsaved, q.get("dx"), ga,
                                          q["ws"], ws_bytes, B, S, T, None)

    seen = {}

    def checked_call(q):                                 # one byte less of either buffer is refused before any launch
        if not seen:
            assert call(q, saved_bytes=nsaved - 1) == hps._lib.ERR_INVALID
            assert call(q, ws_bytes=nws - 1) == hps._lib.ERR_INVALID
            seen["done"] = True
        return call(q)

    res = poisoned_launch(checked_call, inputs, outs, cuda_device, scratch={"saved": nsaved, "ws": nws})
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


# ---- 7. edge cases ------------------------------------------------------------------------------------------------
def test_p0_equals_eval_long_path_and_p1_drops_everything(cuda_device):
    state = recipe_state(43, N_TOKENS, 2, 2)
    B, S, T = 2, 9, 130
    tok, x, dy = _data(B, S, T, N_TOKENS, 5600)
    m = train_model(state, 0.0, cuda_device)
    assert m._draw_dropout_masks(B, S, T) == {}
    y_train = m(tok.to(cuda_device), x.to(cuda_device))
    assert y_train.grad_fn is not None
    with torch.no_grad():
        y_eval = m.eval().forward_long(tok.to(cuda_device), x.to(cuda_device))
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


def test_out_of_range_device_id_poisons_its_sequence_only(cuda_device):
    B, S, T = 2, 9, 130
    m = train_model(recipe_state(95, N_TOKENS, 1, 2), 0.1, cuda_device)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 5700))
    torch.manual_seed(5701)
    masks = m._draw_dropout_masks(B, S, T)
    m0 = {k: v[:1].contiguous() for k, v in masks.items()}
    y0, g0, dx0 = _step(m, tok[:1], x[:1], dy[:1], m0)     # sequence 0 alone, clean
    assert torch.isfinite(y0).all() and all(torch.isfinite(t).all() for t in g0)
    ti = param_keys(1, 2).index("token_embedding.weight")
    for bad in (N_TOKENS, -1):
        t = tok.clone()
        t[1, 2] = bad                                      # ids on the device are not checked on the host
        y, grads, dx = _step(m, t, x, dy, masks)           # the backward returns OK
        assert torch.isnan(y[1]).all()
        assert torch.equal(y[0], y0[0]) and torch.equal(dx[0], dx0[0])
        # the embedding gradient adds its rows in ascending token position: a row that stays finite got nothing
        # from sequence 1, so it holds the sums of sequence 0 alone, bit for bit
        rows = torch.isfinite(grads[ti]).all(dim=1)
        only0 = sorted(set(tok[0].tolist()) - set(t[1].tolist()))
        assert only0 and rows[only0].all() and grads[ti][only0].abs().sum() > 0
        assert torch.equal(grads[ti][rows], g0[ti][rows])


def test_limits_and_errors(cuda_device):
    m = train_model(recipe_state(96, N_TOKENS, 1, 1), 0.0, cuda_device)
    lib, _ = m._ensure_created()
    tok = torch.zeros((1, 5), dtype=torch.int64, device=cuda_device)
    with pytest.raises(RuntimeError, match="1024"):
        m(tok, torch.zeros((1, 1025, 12, 2), device=cuda_device))
    with pytest.raises(RuntimeError, match="128"):
        m(torch.zeros((1, 129), dtype=torch.int64, device=cuda_device), torch.zeros((1, 200, 12, 2), device=cuda_device))
    params = m._tensors()
    pa = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
    buf = torch.zeros((1 << 16,), dtype=torch.uint8, device=cuda_device)
    vp = ctypes.c_void_p(buf.data_ptr())
    args = lambda T: (m._handle, pa, vp, vp, None, 0.0, vp, vp, buf.numel(), 1, 5, T, None)   # noqa: E731
    assert lib.b2h_tpt_train_forward(*args(1025)) == hps._lib.ERR_SHAPE
    assert lib.b2h_tpt_train_forward(*args(0)) == hps._lib.ERR_SHAPE
    saved = lambda T: lib.b2h_tpt_train_bytes(m._handle, 1, 5, T, 0)   # noqa: E731
    # linear in T up to 128; beyond, the log-sum-exp rows of the one decoder layer's two attentions come on top
    assert saved(1024) - saved(128) - 14 * (saved(128) - saved(64)) == 1024 * 32


# ---- 8. graph capture, the loop body with Adam, inference afterwards, and T <= 128 unchanged ----------------------
def test_training_step_captured_in_graph_equals_eager(cuda_device):
    B, S, T = 2, 17, 130
    m = train_model(recipe_state(90, N_TOKENS, 2, 2), 0.1, cuda_device)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 5800))
    torch.manual_seed(5801)
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


def test_adam_trajectory_and_inference_after_updates(cuda_device):
    ne, nd, B, S, T, steps, lr = 1, 2, 4, 40, 200, 5, 2e-4
    lengths = [200, 130, 17, 200]
    state = recipe_state(70, N_TOKENS, ne, nd)
    g = torch.Generator().manual_seed(5900)
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
    m.eval()                                               # the long inference path packs the updated weights
    with torch.no_grad():
        y = m.forward_fused(kd, xd, dif_encoding=False, normalize=False, denormalize=False).cpu().double()
    y64 = tpt_ref.Checker(m, torch.float64)(tok, x)
    assert float((y - y64).abs().max()) <= _tol_y(y64)


def test_short_shape_still_matches_float64(cuda_device):
    """T <= 128 takes the kernels it always took: one of the existing sweep's shapes as a cross-check of the dispatch."""
    _check_case(recipe_state(123, N_TOKENS, 2, 3), 0.1, 2, 40, 100, 1.0, 6000, cuda_device)
