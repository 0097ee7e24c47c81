"""ConvModel training on the MI355X (kernel_train.h through b2h_train_forward / b2h_backward and the loss
gradients, through hand_pose_sl_amd's autograd Functions).

Accuracy bar, per tensor (train_ref.bar): max|g_gpu - g64| <= 4 * max|g32_ref - g64| + 1e-6 * max|g64|, with
g64 float64 autograd (of the reference's own classes for the fixtures, of the oracle's torch port for the
sweep) and g32_ref the same computation in float32 on the CPU: as accurate as the reference's own fp32
training.  The 10-step Adam trajectory is held to the same rule, applied to its losses and final state."""
import ctypes

import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
from hand_pose_sl_amd import _lib
from poison import launch as poisoned_launch
from train_ref import KEYS, assert_within_bar, load_train, port_grads, reference_loss, train_cases

pytestmark = pytest.mark.gpu


def _model(C, pos_emb, state, dev):
    m = hps.ConvModel(C, "ReLU", pos_emb)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    return m.to(dev).train()


def _grads(m):
    sd = dict(m.named_parameters())
    return [sd[k].grad.detach().cpu().double().numpy() for k in KEYS]


def _state(C, pos_emb, seed):
    torch.manual_seed(seed)
    return {k: v.detach().clone() for k, v in hps.ConvModel(C, "ReLU", pos_emb).state_dict().items()}


# ---- 1. the reference's fixtures ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", train_cases("grad_"))
def test_gradients_match_reference_fixtures(name, cuda_device):
    r = load_train(name)
    m = _model(r["C"], r["pos_emb"], r["state"], cuda_device)
    x = torch.from_numpy(r["x"]).to(cuda_device).requires_grad_(True)
    target = torch.from_numpy(r["target"]).to(cuda_device)
    lengths = [int(n) for n in r["lengths"]]
    prediction = m(x)
    for i, n in enumerate(lengths):                     # mask_output (steps/utils.py:309-312), in place
        prediction[i, n:, :] = 0
    if str(r["loss_kind"]) == "L1":
        loss = hps.maskedPoseL1()(prediction, target, lengths)
    else:
        loss = hps.poderatedPoseL1()(prediction, target, lengths, torch.from_numpy(r["scores"]).to(cuda_device))
    assert loss.grad_fn is not None
    loss.backward()
    assert np.isnan(loss.item()) == np.isnan(float(r["loss64"]))
    for k, g in zip(KEYS, _grads(m)):
        key = k.replace(".", "_")
        assert_within_bar(g, r["g64_" + key], r["err32_" + key], f"{name} {k}")
    assert_within_bar(x.grad.cpu().double().numpy(), r["dx64"], r["err32_dx"], f"{name} dx")


# ---- 2. sweep against float64 autograd of the torch port ------------------------------------------------------
SHAPES = [(1, 1), (3, 2), (3, 3), (1, 5), (3, 8), (3, 9), (1, 16), (3, 17), (3, 63), (1, 64), (3, 65), (3, 200),
          (1, 201), (1, 600), (128, 64)]


def _check_case(C, pos_emb, B, T, scale, seed, dev):
    state = _state(C, pos_emb, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((B, T, 12, 2), generator=g) * scale
    dy = torch.randn((B, T, 21, 2), generator=g)
    y64, g64, dx64 = port_grads(x, state, dy, pos_emb, torch.float64)
    y32, g32, dx32 = port_grads(x, state, dy, pos_emb, torch.float32)
    m = _model(C, pos_emb, state, dev)
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    y.backward(dy.to(dev))
    what = f"C={C} pos_emb={pos_emb} B={B} T={T} scale={scale}"
    err_y = float((y.detach().cpu().double() - y64).abs().max())
    assert err_y <= 2e-5 * max(1.0, float(y64.abs().max())), f"{what}: y {err_y:.3e}"   # test_gpu_parity's fp32 bar
    for k, gg, a, b in zip(KEYS, _grads(m), g64, g32):
        assert_within_bar(gg, a.numpy(), (b.double() - a).abs().max(), f"{what} {k}")
    assert_within_bar(xd.grad.cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), f"{what} dx")


@pytest.mark.parametrize("C", [1, 7, 16, 30, 32, 33, 64, 65, 128])
def test_sweep_against_float64_autograd(C, cuda_device):
    for j, (B, T) in enumerate(SHAPES):
        _check_case(C, False, B, T, 1.0 if j % 2 else 1.0 / 1280, 1000 + 31 * C + j, cuda_device)
    for j, B in enumerate((1, 3, 128)):
        _check_case(C, True, B, 100, 1.0 if j % 2 else 1.0 / 1280, 5000 + 31 * C + j, cuda_device)


def test_large_batch_many_slabs(cuda_device):
    m = _model(30, False, _state(30, False, 7), cuda_device)
    lib, _ = m._ensure_created()
    B, T = 1024, 200
    # 1024 x 5 tiles of 40 frames: the 2048-slab cap, two or three tiles summed per slab
    assert lib.b2h_backward_workspace_bytes(m._handle, B, T) == 2048 * ((sum(p.numel() for p in m.parameters()) + 3) // 4 * 4) * 4
    _check_case(30, False, B, T, 1.0, 77, cuda_device)


# ---- 3. determinism -------------------------------------------------------------------------------------------
def _run(m, x, dy):
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(True)
    m(xd).backward(dy)
    return [p.grad.clone() for p in m.parameters()], xd.grad.clone()


def test_bitwise_deterministic_across_runs_streams_and_batches(cuda_device):
    m = _model(30, False, _state(30, False, 11), cuda_device)
    g = torch.Generator().manual_seed(12)
    x = torch.randn((300, 203, 12, 2), generator=g).to(cuda_device)
    dy = torch.randn((300, 203, 21, 2), generator=g).to(cuda_device)
    g1, dx1 = _run(m, x, dy)
    g2, dx2 = _run(m, x, dy)
    s = torch.cuda.Stream(cuda_device)
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        g3, dx3 = _run(m, x, dy)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    for a, b, c in zip(g1, g2, g3):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(dx1, dx2) and torch.equal(dx1, dx3)
    for i in (0, 17, 299):                               # dx of a sequence alone == inside the batch
        _, dxi = _run(m, x[i:i + 1], dy[i:i + 1])
        assert torch.equal(dxi[0], dx1[i])


# ---- 4. poisoned outputs and workspace ------------------------------------------------------------------------
@pytest.mark.parametrize("C,pos_emb,B,T,with_dx", [(30, False, 3, 77, True), (30, False, 2, 9, False),
                                                    (65, True, 2, 100, True), (8, False, 5, 1, True)])
def test_outputs_fully_written_and_workspace_contents_irrelevant(C, pos_emb, B, T, with_dx, cuda_device):
    m = _model(C, pos_emb, _state(C, pos_emb, 21), cuda_device)
    lib, _ = m._ensure_created()
    g = torch.Generator().manual_seed(22)
    x = torch.randn((B, T, 12, 2), generator=g)
    dy = torch.randn((B, T, 21, 2), generator=g)
    params = {f"p{i}": p.detach().cpu() for i, p in enumerate(m._params())}
    outs = {f"g{i}": tuple(p.shape) for i, p in enumerate(m._params())}
    if with_dx:
        outs["dx"] = (B, T, 12, 2)
    outs["y"] = (B, T, 21, 2)
    nbytes = lib.b2h_backward_workspace_bytes(m._handle, B, T)
    vp = ctypes.c_void_p

    def call(p):
        pa = (vp * 8)(*[p[f"p{i}"] for i in range(8)])
        ga = (vp * 8)(*[p[f"g{i}"] for i in range(8)])
        rc = lib.b2h_train_forward(m._handle, pa, p["x"], p["y"], B, T, None)
        return rc or lib.b2h_backward(m._handle, pa, p["x"], p["dy"], p.get("dx"), ga, B, T, p["ws"], nbytes, None)

    res = poisoned_launch(call, dict(x=x, dy=dy, **params), outs, cuda_device, scratch={"ws": nbytes})
    y64, g64, dx64 = port_grads(x, {k: v.cpu() for k, v in m.state_dict().items()}, dy, pos_emb, torch.float64)
    _, g32, dx32 = port_grads(x, {k: v.cpu() for k, v in m.state_dict().items()}, dy, pos_emb, torch.float32)
    for i, (a, b) in enumerate(zip(g64, g32)):
        assert_within_bar(res[f"g{i}"].cpu().double().numpy(), a.numpy(), (b.double() - a).abs().max(), f"g{i}")
    if with_dx:
        assert_within_bar(res["dx"].cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "dx")


# ---- 5. loss gradients ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["L1", "confL1"])
def test_loss_gradients_match_reference_criteria(kind, cuda_device):
    B, T = 6, 37
    lengths = [37, 0, 1, 20, 50, 36]
    g = torch.Generator().manual_seed(40)
    pred = torch.randn((B, T, 21, 2), generator=g, dtype=torch.float64)
    pred[0, 3, 4, 1] = 0.25                                   # a tie: sign(0) = 0
    tgt = torch.randn((B, T, 21, 2), generator=g, dtype=torch.float64)
    tgt[0, 3, 4, 1] = 0.25
    scores = torch.rand((B, T, 21), generator=g, dtype=torch.float64)
    want = {}
    for dt in (torch.float64, torch.float32):
        p = pred.detach().to(dt).clone().requires_grad_(True)
        loss = reference_loss(p.clone(), tgt.to(dt), lengths, scores.to(dt), kind)
        (loss * 3.0).backward()
        want[dt] = p.grad.double()
    p = pred.float().to(cuda_device).requires_grad_(True)
    t, s = tgt.float().to(cuda_device), scores.float().to(cuda_device)
    loss = hps.masked_pose_l1(p, t, lengths) if kind == "L1" else hps.weighted_pose_l1(p, t, lengths, s)
    assert np.isnan(loss.item())                               # lengths[1] == 0: NaN as torch's empty mean
    (loss * 3.0).backward()
    got = p.grad.cpu().double()
    assert not got[1].any() and not got[2, 1:].any() and not got[3, 20:].any() and got[0, 3, 4, 1] == 0
    assert_within_bar(got.numpy(), want[torch.float64].numpy(), (want[torch.float32] - want[torch.float64]).abs().max(), kind)
    # values unchanged when no gradient is needed
    with torch.no_grad():
        l2 = hps.masked_pose_l1(p, t, lengths) if kind == "L1" else hps.weighted_pose_l1(p, t, lengths, s)
    assert torch.equal(loss.detach(), l2) or (np.isnan(loss.item()) and np.isnan(l2.item()))


# ---- 6./7. the reference loop body with Adam, then eval-mode inference on the updated weights ----------------
def test_adam_trajectory_and_inference_after_updates(cuda_device):
    r = load_train("traj_c30_b4_t64")
    m = _model(r["C"], False, r["state"], cuda_device)
    m.eval()
    with torch.no_grad():
        m(torch.from_numpy(r["x"]).to(cuda_device))           # packs the initial weights (inference path)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=float(r["lr"]))
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
    assert_within_bar(np.array(losses), r["losses64"], np.abs(r["losses32"] - r["losses64"]).max(), "losses")
    sd = m.state_dict()
    for k in KEYS:
        key = k.replace(".", "_")
        a, b = r["final64_" + key], r["final32_" + key].astype(np.float64)
        assert_within_bar(sd[k].cpu().double().numpy(), a, np.abs(b - a).max(), "final " + k)
    # 7. the inference path repacks after the in-place updates
    from oracle.torch_port import torch_forward
    m.eval()
    with torch.no_grad():
        y = m(x).cpu()
    ref = torch_forward(x.cpu(), {k: v.cpu() for k, v in sd.items()})
    assert float((y - ref).abs().max()) <= 2e-5


def test_eval_and_no_grad_calls_unchanged(cuda_device):
    st = _state(30, False, 50)
    m = _model(30, False, st, cuda_device)
    x = (torch.rand((3, 70, 12, 2), generator=torch.Generator().manual_seed(51)) - 0.5).to(cuda_device)
    with torch.no_grad():
        y_nograd = m(x)                                        # training mode, no_grad: inference kernel
    m.eval()
    y_eval = m(x)
    assert y_eval.grad_fn is None and torch.equal(y_nograd, y_eval)
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        m.forward_fused(x)
    # frozen parameters, input requiring a gradient: differentiable now (was a detached output)
    for p in m.parameters():
        p.requires_grad_(False)
    xd = x.clone().requires_grad_(True)
    y = m(xd)
    assert y.grad_fn is not None
    y.sum().backward()
    assert xd.grad is not None and all(p.grad is None for p in m.parameters())


# ---- 8. graph capture -----------------------------------------------------------------------------------------
def test_training_step_captured_in_graph_equals_eager(cuda_device):
    m = _model(30, False, _state(30, False, 60), cuda_device)
    g = torch.Generator().manual_seed(61)
    x = torch.randn((16, 120, 12, 2), generator=g).to(cuda_device)
    dy = torch.randn((16, 120, 21, 2), generator=g).to(cuda_device)
    eager_g, eager_dx = _run(m, x, dy)
    xs = x.clone().requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    s = torch.cuda.Stream(cuda_device)                        # warm-up on a side stream, as torch's docs do
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        m(xs).backward(dy)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    for p in m.parameters():
        p.grad = None
    xs.grad = None
    with torch.cuda.graph(graph):
        m(xs).backward(dy)
    for p in m.parameters():
        p.grad.fill_(float("nan"))
    xs.grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, p in zip(eager_g, m.parameters()):
        assert torch.equal(a, p.grad)
    assert torch.equal(eager_dx, xs.grad)
