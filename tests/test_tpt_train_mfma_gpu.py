"""TextPoseTransformer training beyond 128 frames on the fp32 MFMA route (`model.set_train_kernels("mfma")`:
b2h_mt_sdpa, b2h_mt_sdpa_bwd_q, b2h_mt_sdpa_bwd_kv of kernel_train_attn_mfma.h) on the MI355X.

The bars are the project's own (tpt_train_ref.assert_within_bar: per tensor max|g - g64| <= 4 * max|g32_ref - g64| +
1e-6 * max|g64|; y within tpt_ref.BAR * max(1, max|y64|)), and the inputs are chosen by the rule of
test_tpt_train_long_gpu.py (`_check_case`: on the CPU ports alone, no float64 ReLU input closer to zero than
RELU_MARGIN times the float32 port's rounding).  That module's helpers, and those of its tests that this route has to
pass unchanged, run here with its `train_model` replaced by one that selects the MFMA route (the `mfma` fixture);
every model built that way is checked to have resolved to b2h_mt_sdpa.  The sweep prints the worst ratio
max|g - g64| / max|g32_ref - g64| and the worst y error it has seen so far (pytest -s)."""
import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
import test_tpt_train_long_gpu as long_gpu
import tpt_geom_ref
from tpt_train_ref import (assert_within_bar, param_keys, port_grads, recipe_state, train_model)

pytestmark = pytest.mark.gpu
N_TOKENS = long_gpu.N_TOKENS
WORST = {"ratio": 0.0, "what": "", "y": 0.0}            # of this route alone: long_gpu.WORST is the default route's
_data, _step, _grads, _cpu, _tol_y = long_gpu._data, long_gpu._step, long_gpu._grads, long_gpu._cpu, long_gpu._tol_y


def _attn_name(m, T):
    lib, _ = m._ensure_created()
    name = lib.b2h_tpt_train_attn_name(m._handle, T)
    return None if name is None else name.decode()


def mfma_model(state, p, dev):
    return train_model(state, p, dev).set_train_kernels("mfma")


class _Built(list):
    def all_on_mfma(self, T):
        assert self and all(m.train_kernels == "mfma" for m in self)
        # the handle follows the model at every training forward; this is what it was left at
        assert all(_attn_name(m, T) == "b2h_mt_sdpa" for m in self)


@pytest.fixture
def mfma(monkeypatch):
    """test_tpt_train_long_gpu.py's helpers and tests on the MFMA route; yields the models they built."""
    built = _Built()

    def wrap(make):
        def made(state, p, dev=None):
            m = make(state, p, dev).set_train_kernels("mfma")
            built.append(m)
            return m
        return made
    monkeypatch.setattr(long_gpu, "train_model", wrap(train_model))
    monkeypatch.setattr(tpt_geom_ref, "train_model", wrap(tpt_geom_ref.train_model))
    monkeypatch.setattr(long_gpu, "WORST", WORST)
    return built


# ---- 1. the reference's fixture at the trainer's length ----------------------------------------------------------
def test_gradients_match_reference_fixture_at_200_frames(mfma, cuda_device):
    long_gpu.test_gradients_match_reference_fixture_at_200_frames(cuda_device)
    mfma.all_on_mfma(200)


# ---- 2. sweep against float64 autograd of the port, with the masks the kernels used ------------------------------
# The smallest shapes that cover every edge of the tiling: T on both sides of multiples of 16 (the MFMA tile), 64 and
# 128; T = 0, 1, 2, 3 mod 4 (the k-step, where keys or queries are summed over); one tile-aligned T (144) and one half
# tile (200); S = 1 (one valid key in a tile and in a k-step), S = 1, 2, 3 mod 4, S one past a tile, a full block.
SHAPES = [(2, 1, 129), (2, 17, 130), (1, 128, 129), (2, 40, 200), (3, 33, 144), (1, 7, 191), (1, 38, 192), (1, 7, 193),
          (1, 38, 255), (1, 7, 256), (1, 40, 257)]
DEEP = [(2, 1, 129), (2, 17, 130), (2, 40, 200), (1, 40, 257)]   # also with (2, 3) layers
CASES = [((1, 1), s) for s in SHAPES] + [((2, 3), s) for s in DEEP]


@pytest.mark.parametrize("layers,shape", CASES, ids=lambda v: "x".join(str(i) for i in v))
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_sweep_against_float64_autograd(p, layers, shape, mfma, cuda_device):
    state = recipe_state(300 + 10 * layers[0] + layers[1], N_TOKENS, *layers)   # non-default biases and LayerNorms
    j = SHAPES.index(shape)
    unused = long_gpu._check_case(state, p, *shape, 1.0 if j % 2 else 1.0 / 1280, 7000 + 97 * layers[1] + j, cuda_device)
    assert N_TOKENS - 1 in unused                       # rows of unused ids are exactly zero (checked in _check_case)
    mfma.all_on_mfma(shape[2])


# ---- 3. the frame limit ---------------------------------------------------------------------------------------------
def test_sweep_at_the_frame_limit(mfma, cuda_device):
    long_gpu.test_sweep_at_the_frame_limit(cuda_device)    # (1, 16, 1024), p = 0.1
    mfma.all_on_mfma(1024)


# ---- 4. the running maximum moves -------------------------------------------------------------------------------
def test_row_maximum_in_a_later_key_block(mfma, cuda_device):
    long_gpu.test_row_maximum_in_a_later_key_block(cuda_device)   # T = 2 * 128 + 44; the property is checked on float64
    mfma.all_on_mfma(2 * 128 + 44)


# ---- 5. the other geometries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_joints,nout", [(8, 42), (29, 8)])
def test_geometries(n_joints, nout, mfma, cuda_device):
    long_gpu.test_geometries(n_joints, nout, cuda_device)   # (2, 40, 130), p = 0.1, through tpt_geom_ref
    mfma.all_on_mfma(130)


# ---- 6. determinism ---------------------------------------------------------------------------------------------
def test_bitwise_deterministic_across_runs_streams_and_batches(mfma, cuda_device):
    long_gpu.test_bitwise_deterministic_across_runs_streams_and_batches(cuda_device)   # (8, 40, 200), p = 0.1
    mfma.all_on_mfma(200)


# ---- 7. route and default path ----------------------------------------------------------------------------------
def test_route_names_and_default_path_unchanged(cuda_device):
    state = recipe_state(310, N_TOKENS, 1, 2)
    a, b = mfma_model(state, 0.1, cuda_device), train_model(state, 0.1, cuda_device)
    lib, _ = a._ensure_created()
    assert b.train_kernels == "valu" and _attn_name(b, 129) == "b2h_lt_sdpa"    # the default of a new model
    for value, name in ((1, "b2h_mt_sdpa"), (0, "b2h_lt_sdpa")):
        assert lib.b2h_tpt_set_train_kernel(a._handle, value) == hps._lib.OK
        assert _attn_name(a, 129) == name and _attn_name(a, 1024) == name
        assert _attn_name(a, 128) == "b2h_tt_sdpa" and _attn_name(a, 1) == "b2h_tt_sdpa"
        assert _attn_name(a, 0) is None
    assert lib.b2h_tpt_set_train_kernel(a._handle, 2) == hps._lib.ERR_INVALID
    assert lib.b2h_tpt_set_train_kernel(a._handle, -1) == hps._lib.ERR_INVALID
    assert _attn_name(a, 129) == "b2h_lt_sdpa"          # a refused value changes nothing

    def step(m, B, S, T, seed):
        tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, seed))
        torch.manual_seed(seed + 1)
        return _step(m, tok, x, dy, m._draw_dropout_masks(B, S, T))

    def same(u, v):
        return torch.equal(u[0], v[0]) and torch.equal(u[2], v[2]) and all(torch.equal(s, t) for s, t in zip(u[1], v[1]))
    step(a, 2, 17, 130, 7100)                           # a ran on mfma ...
    assert _attn_name(a, 130) == "b2h_mt_sdpa"
    a.set_train_kernels("valu")                         # ... and back on valu equals a model never switched
    assert same(step(a, 2, 17, 130, 7100), step(b, 2, 17, 130, 7100))
    assert _attn_name(a, 130) == "b2h_lt_sdpa"
    a.set_train_kernels("mfma")
    for B, S, T in ((2, 9, 128), (2, 40, 100)):         # no effect up to 128 frames
        assert same(step(a, B, S, T, 7110 + T), step(b, B, S, T, 7110 + T))
        assert _attn_name(a, T) == "b2h_tt_sdpa"


# ---- 8. a backward follows its forward --------------------------------------------------------------------------
def test_backward_runs_the_route_of_its_forward(cuda_device):
    B, S, T = 2, 17, 130
    m = mfma_model(recipe_state(320, N_TOKENS, 1, 2), 0.1, cuda_device)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 7200))
    torch.manual_seed(7201)
    masks = m._draw_dropout_masks(B, S, T)
    _, g_all, dx_all = _step(m, tok, x, dy, masks)      # forward and backward on mfma
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(True)
    y = m._forward_train(tok, xd, masks)
    m.set_train_kernels("valu")                         # switched between the two
    y.backward(dy)
    assert _attn_name(m, T) == "b2h_mt_sdpa"            # what the backward set the handle to
    assert all(torch.equal(a, p.grad) for a, p in zip(g_all, m._tensors())) and torch.equal(dx_all, xd.grad)
    _, g_valu, _ = _step(m, tok, x, dy, masks)          # the model says valu now: the next step runs it
    assert _attn_name(m, T) == "b2h_lt_sdpa" and all(torch.isfinite(g).all() for g in g_valu)


# ---- 9. poisoned outputs, saved buffer and scratch --------------------------------------------------------------
class _HandleOnMfma:
    """For callers of the C ABI itself: the model's handle set to B2H_TRAIN_MFMA as soon as it exists."""

    def __init__(self, m):
        self.m = m

    def __getattr__(self, name):
        return getattr(self.m, name)

    def _ensure_created(self):
        lib, dev = self.m._ensure_created()
        assert lib.b2h_tpt_set_train_kernel(self.m._handle, hps._lib.TRAIN_KERNELS["mfma"]) == hps._lib.OK
        return lib, dev


@pytest.mark.parametrize("with_dx", [True, False])
def test_outputs_fully_written_and_scratch_contents_irrelevant(with_dx, monkeypatch, cuda_device):
    B, S, T = 2, 9, 130
    m = train_model(recipe_state(60, N_TOKENS, 1, 2), 0.1, cuda_device)
    lib, _ = m._ensure_created()
    sizes = []
    for value in (0, 1, 0):
        assert lib.b2h_tpt_set_train_kernel(m._handle, value) == hps._lib.OK
        sizes.append([lib.b2h_tpt_train_bytes(m._handle, B, S, T, which) for which in (0, 1)])
    assert sizes[0] == sizes[1] == sizes[2] and all(sizes[0])       # the switch does not move the buffer sizes
    built = []

    def made(state, p, dev=None):
        built.append(_HandleOnMfma(train_model(state, p, dev)))
        return built[-1]
    monkeypatch.setattr(long_gpu, "train_model", made)
    # buffers of exactly b2h_tpt_train_bytes, poisoned; every output fully written; the scratch's contents irrelevant
    long_gpu.test_outputs_fully_written_and_scratch_contents_irrelevant(with_dx, cuda_device)
    assert len(built) == 1 and _attn_name(built[0].m, T) == "b2h_mt_sdpa"


# ---- 10. edge cases ---------------------------------------------------------------------------------------------
def test_p0_equals_eval_long_path_and_p1_drops_everything(mfma, cuda_device):
    long_gpu.test_p0_equals_eval_long_path_and_p1_drops_everything(cuda_device)   # T = 130
    mfma.all_on_mfma(130)
    # p = 1: the all-dropped result the default route gives
    state, (B, S, T) = recipe_state(43, N_TOKENS, 2, 2), (2, 9, 130)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 5600))
    out = []
    for m in (mfma_model(state, 1.0, cuda_device), train_model(state, 1.0, cuda_device)):
        torch.manual_seed(1)
        out.append(_step(m, tok, x, dy, m._draw_dropout_masks(B, S, T)))
    assert torch.equal(out[0][0], out[1][0])            # y: no attention output survives, the rest is the same kernels
    for k, a, b in zip(param_keys(2, 2), out[0][1], out[1][1]):
        # attention gradients are exact zeros on both routes; everything downstream of them is the same kernels
        assert torch.equal(a, b), k
    assert torch.equal(out[0][2], out[1][2])


def test_out_of_range_device_id_poisons_its_sequence_only(mfma, cuda_device):
    long_gpu.test_out_of_range_device_id_poisons_its_sequence_only(cuda_device)   # y, dx of sequence 0 == it alone
    mfma.all_on_mfma(130)
    # and sequence 0 of the poisoned batch lies inside the bars (a NaN that crossed a padded row would show here)
    B, S, T, p = 2, 9, 130, 0.1
    state = recipe_state(95, N_TOKENS, 1, 2)
    m = mfma_model(state, p, cuda_device)
    tok, x, dy = _data(B, S, T, N_TOKENS, 5700)
    torch.manual_seed(5701)
    masks = m._draw_dropout_masks(B, S, T)
    bad = tok.clone()
    bad[1, 2] = N_TOKENS
    y, _, dx = _step(m, bad.to(cuda_device), x.to(cuda_device), dy.to(cuda_device), masks)
    assert torch.isnan(y[1]).all() and torch.isfinite(y[0]).all() and torch.isfinite(dx[0]).all()
    m0 = {k: v[:1].cpu() for k, v in masks.items()}
    y64, _, dx64 = port_grads(tok[:1], x[:1], state, m0, p, dy[:1], torch.float64)
    _, _, dx32 = port_grads(tok[:1], x[:1], state, m0, p, dy[:1], torch.float32)
    assert float((y[:1].cpu().double() - y64).abs().max()) <= _tol_y(y64)
    assert_within_bar(dx[:1].cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "dx of sequence 0")


def test_limits_and_errors(mfma, cuda_device):
    long_gpu.test_limits_and_errors(cuda_device)        # T = 1025 is refused, by the model and by the C ABI
    assert mfma and all(m.train_kernels == "mfma" for m in mfma)


# ---- 11. graph capture as the model's first use -----------------------------------------------------------------
def test_training_step_captured_in_graph_as_first_use_equals_eager(cuda_device):
    B, S, T = 2, 17, 130
    state = recipe_state(90, N_TOKENS, 2, 2)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 5800))
    eager = mfma_model(state, 0.1, cuda_device)
    torch.manual_seed(5801)
    masks = eager._draw_dropout_masks(B, S, T)
    _, eager_g, eager_dx = _step(eager, tok, x, dy, masks)
    m = mfma_model(state, 0.1, cuda_device)             # a model that has not run yet
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
    assert _attn_name(m, T) == "b2h_mt_sdpa"
    for a, p in zip(eager_g, m._tensors()):
        assert torch.equal(a, p.grad)
    assert torch.equal(eager_dx, xs.grad)


# ---- 12. the loop body with Adam, inference afterwards ----------------------------------------------------------
def test_adam_trajectory_and_inference_after_updates(mfma, cuda_device):
    # five steps at (4, 40, 200), lengths [200, 130, 17, 200], lr 2e-4; then forward_fused in eval mode
    long_gpu.test_adam_trajectory_and_inference_after_updates(cuda_device)
    mfma.all_on_mfma(200)


# ---- 13. the two routes agree -----------------------------------------------------------------------------------
def test_both_routes_inside_the_bars_on_the_same_batch(cuda_device):
    B, S, T, p = 2, 40, 200, 0.1
    ne, nd = 1, 2
    state = recipe_state(330, N_TOKENS, ne, nd)
    tok, x, dy = _data(B, S, T, N_TOKENS, 7300)
    models = {"mfma": mfma_model(state, p, cuda_device), "valu": train_model(state, p, cuda_device)}
    torch.manual_seed(7301)
    masks = models["mfma"]._draw_dropout_masks(B, S, T)
    y64, g64, dx64 = port_grads(tok, x, state, _cpu(masks), p, dy, torch.float64)
    _, g32, dx32 = port_grads(tok, x, state, _cpu(masks), p, dy, torch.float32)
    keys = param_keys(ne, nd) + ["dx"]
    truth = [g.numpy() for g in g64] + [dx64.numpy()]
    err32 = [float((b.double() - a).abs().max()) for a, b in zip(g64 + [dx64], g32 + [dx32])]
    got = {}
    for name, m in models.items():
        y, grads, dx = _step(m, tok.to(cuda_device), x.to(cuda_device), dy.to(cuda_device), masks)
        assert _attn_name(m, T) == ("b2h_mt_sdpa" if name == "mfma" else "b2h_lt_sdpa")
        assert float((y.cpu().double() - y64).abs().max()) <= _tol_y(y64), name
        got[name] = [g.cpu().double().numpy() for g in grads + [dx]]
        for k, g, a, e in zip(keys, got[name], truth, err32):
            assert_within_bar(g, a, e, f"{name} {k}")
    print()
    for k, a, b in zip(keys, got["mfma"], got["valu"]):   # recorded, not required: the routes may produce equal bits
        print(f"max|g_mfma - g_valu| {k}: {np.abs(a - b).max():.3e} (max|g| {np.abs(b).max():.3e})")
