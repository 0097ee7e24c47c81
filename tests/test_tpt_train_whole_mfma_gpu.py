"""TextPoseTransformer training with `model.set_train_whole("mfma")` on the MI355X: every attention of at most
128 x 128 -- the encoder's self-attention (S x S) at every T, and up to 128 frames the decoder's self-attention (T x T)
and cross-attention (T x S) -- on b2h_mw_sdpa / b2h_mw_sdpa_bwd of kernel_train_attn_whole_mfma.h, which until now
only ever ran with Tq = Tk (TransformerEnc).

The bars are test_tpt_train_gpu.py's own, unchanged: per tensor max|g - g64| <= 4 * max|g32_ref - g64| +
1e-6 * max|g64| and y within tpt_ref.BAR * max(1, max|y64|), against float64 autograd of tpt_train_ref.port_forward
with the masks the kernels used.  That module's helpers, and those of its tests that the route has to pass unchanged,
run here with its `train_model` replaced by one that switches the model and its handle (the `mw` fixture); every model
built that way is checked to have resolved to b2h_mw_sdpa in the encoder and, at T <= 128, in the decoder.  Its SHAPES
have S != T in both directions on both sides of a 16-row tile and of lane 64 (a lane's second key), one row, one key,
and the LDS maximum (128, 128).

Bit-equality, as built (DESIGN.md sections 25 and 30): the forward keeps one ascending chain per element for any
(Tq, Tk), so y equals the default route's bit for bit; the backward sums rowsum(dSd o S) from the accumulators in another
order, so the gradients are held to the bars and their largest difference from the default is printed (pytest -s)."""
import pytest
import torch

import hand_pose_sl_amd as hps
import test_graph_trainer_gpu as gt
import test_tpt_train_gpu as base
import test_tpt_train_long_gpu as long_gpu
from hand_pose_sl_amd import _lib
from tpt_train_ref import TRAIN_CASES, assert_within_bar, param_keys, port_grads, recipe_state, train_model

pytestmark = pytest.mark.gpu
N_TOKENS = base.N_TOKENS
SHAPES = base.SHAPES
WORST = {"ratio": 0.0, "what": "", "y": 0.0}            # of this route alone: base.WORST is the default route's
ATTN = {"valu": "b2h_tt_sdpa", "mfma": "b2h_mw_sdpa"}
BLOCKED = {"valu": "b2h_lt_sdpa", "mfma": "b2h_mt_sdpa"}
_data, _step, _cpu, _tol_y = base._data, base._step, base._cpu, base._tol_y


def _names(m, T):
    """(the encoder's attention kernel, the decoder's at T frames) as the handle stands."""
    lib, _ = m._ensure_created()
    enc, dec = lib.b2h_tpt_train_enc_attn_name(m._handle), lib.b2h_tpt_train_attn_name(m._handle, T)
    return (None if enc is None else enc.decode()), (None if dec is None else dec.decode())


def _set_handle(m, whole):
    lib, _ = m._ensure_created()
    assert lib.b2h_tpt_set_train_whole(m._handle, _lib.TRAIN_KERNELS[whole]) == _lib.OK


def whole_model(state, p, dev, whole="mfma", kernels="valu", linear="valu"):
    """A training model on the given routes; the handle too, for the tests that call the C ABI themselves."""
    m = train_model(state, p, dev).set_train_whole(whole).set_train_kernels(kernels).set_train_linear(linear)
    _set_handle(m, whole)
    return m


class _Built(list):
    def all_on_route(self):
        assert self and all(m.train_whole == "mfma" for m in self)
        # the handle follows the model at every training forward; this is what it was left at
        for m in self:
            assert _names(m, 1) == _names(m, 128) == ("b2h_mw_sdpa", "b2h_mw_sdpa")
            assert _names(m, 129) == ("b2h_mw_sdpa", BLOCKED[m.train_kernels])


@pytest.fixture
def mw(monkeypatch):
    """test_tpt_train_gpu.py's (and test_tpt_train_long_gpu.py's) helpers and tests on the route; yields the models."""
    built = _Built()

    def made(state, p, dev=None):
        m = train_model(state, p, dev).set_train_whole("mfma").set_train_kernels(getattr(built, "kernels", "valu"))
        _set_handle(m, "mfma")
        built.append(m)
        return m
    monkeypatch.setattr(base, "train_model", made)
    monkeypatch.setattr(long_gpu, "train_model", made)
    monkeypatch.setattr(base, "WORST", WORST)
    monkeypatch.setattr(long_gpu, "WORST", WORST)
    return built


# ---- 1. sweep against float64 autograd of the port, and the reference's fixtures ---------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d_s%d_t%d" % s)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("layers", [(1, 1), (2, 3)], ids=lambda l: "e%d_d%d" % l)
def test_sweep_against_float64_autograd(layers, p, shape, mw, cuda_device):
    base.test_sweep_against_float64_autograd(layers, p, shape, cuda_device)
    mw.all_on_route()


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_gradients_match_reference_fixtures(name, mw, cuda_device):
    base.test_gradients_match_reference_fixtures(name, cuda_device)
    mw.all_on_route()


# ---- 2. beyond 128 frames: the encoder on the pair, the decoder blocked ------------------------------------------
@pytest.mark.parametrize("kernels", ["valu", "mfma"])
def test_long_case_encoder_on_the_pair_decoder_blocked(kernels, mw, cuda_device):
    mw.kernels = kernels
    long_gpu._check_case(recipe_state(341, N_TOKENS, 2, 2), 0.1, 1, 40, 130, 1.0, 8100, cuda_device)
    mw.all_on_route()
    m = mw[0]
    assert _names(m, 130) == ("b2h_mw_sdpa", BLOCKED[kernels])
    _set_handle(m, "valu")                              # the new switch does not move the decoder beyond 128 frames
    assert _names(m, 130) == ("b2h_tt_sdpa", BLOCKED[kernels])


# ---- 3. against the default route on the same batch, masks and seeds ---------------------------------------------
def _both_routes(state, p, B, S, T, seed, dev, routes):
    """One step per route (keywords of whole_model) on one batch and one set of masks: [y, gradients .., dx] each."""
    tok, x, dy = (t.to(dev) for t in _data(B, S, T, N_TOKENS, seed))
    got, masks = [], None
    for route in routes:
        m = whole_model(state, p, dev, **route)
        if masks is None:
            torch.manual_seed(seed + 1)
            masks = m._draw_dropout_masks(B, S, T)
        y, grads, dx = _step(m, tok, x, dy, masks)
        assert _names(m, T)[0] == ATTN[route.get("whole", "mfma")]
        got.append([y] + grads + [dx])
    return got, masks


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d_s%d_t%d" % s)
def test_y_bit_equal_to_the_default_route_and_gradients_inside_the_bars(shape, cuda_device):
    ne, nd, p = 2, 2, 0.1
    state = recipe_state(350, N_TOKENS, ne, nd)
    B, S, T = shape
    seed = 8200 + SHAPES.index(shape)
    (new, old), masks = _both_routes(state, p, B, S, T, seed, cuda_device, [dict(whole="mfma"), dict(whole="valu")])
    keys = ["y"] + param_keys(ne, nd) + ["dx"]
    rel = max((float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-300), k)
              for k, a, b in zip(keys[1:], new[1:], old[1:]))
    print(f"\n{shape}: {sum(torch.equal(a, b) for a, b in zip(new, old))} of {len(keys)} tensors bit-equal to the default "
          f"route; largest gradient difference {rel[0]:.3e} of the tensor's maximum ({rel[1]})")
    assert torch.equal(new[0], old[0]), f"y differs from the default route by {float((new[0] - old[0]).abs().max()):.3e}"
    tok, x, dy = _data(B, S, T, N_TOKENS, seed)
    y64, g64, dx64 = port_grads(tok, x, state, _cpu(masks), p, dy, torch.float64)
    _, g32, dx32 = port_grads(tok, x, state, _cpu(masks), p, dy, torch.float32)
    assert float((new[0].cpu().double() - y64).abs().max()) <= _tol_y(y64)
    for k, g, a, b in zip(keys[1:], new[1:], g64 + [dx64], g32 + [dx32]):
        assert_within_bar(g.cpu().double().numpy(), a.numpy(), float((b.double() - a).abs().max()), f"{shape} {k}")


# ---- 4. the default path is untouched; a backward follows its forward --------------------------------------------
def _same(u, v):
    return torch.equal(u[0], v[0]) and torch.equal(u[2], v[2]) and all(torch.equal(s, t) for s, t in zip(u[1], v[1]))


def test_route_names_refusals_and_default_path_unchanged(cuda_device):
    state = recipe_state(360, N_TOKENS, 1, 2)
    a, b = train_model(state, 0.1, cuda_device), train_model(state, 0.1, cuda_device)
    lib, _ = a._ensure_created()
    assert a.train_whole == "valu" and _names(a, 100) == ("b2h_tt_sdpa", "b2h_tt_sdpa")   # the default of a new model
    sizes = []
    for kv in (0, 1):
        assert lib.b2h_tpt_set_train_kernel(a._handle, kv) == _lib.OK
        blocked = BLOCKED["mfma" if kv else "valu"]
        for wv, name in ((1, "b2h_mw_sdpa"), (0, "b2h_tt_sdpa")):
            assert lib.b2h_tpt_set_train_whole(a._handle, wv) == _lib.OK
            for T in (1, 100, 128):
                assert _names(a, T) == (name, name)
            for T in (129, 1024):
                assert _names(a, T) == (name, blocked)  # beyond 128 frames the decoder decides as before
            assert _names(a, 0) == (name, None)
            for bad in (2, -1):                         # a refused value changes nothing
                assert lib.b2h_tpt_set_train_whole(a._handle, bad) == _lib.ERR_INVALID
                assert lib.b2h_last_error()
                assert _names(a, 100) == (name, name) and _names(a, 129) == (name, blocked)
            sizes.append([lib.b2h_tpt_train_bytes(a._handle, 2, S, T, which)
                          for which in (0, 1) for S, T in ((1, 1), (40, 100), (128, 128), (40, 130))])
    assert all(s == sizes[0] for s in sizes) and all(sizes[0])   # the switch does not move the buffer sizes

    def step(m, B, S, T, seed):
        tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, seed))
        torch.manual_seed(seed + 1)
        return _step(m, tok, x, dy, m._draw_dropout_masks(B, S, T))

    for B, S, T in ((3, 9, 17), (2, 40, 100), (1, 40, 130)):
        a.set_train_whole("mfma")
        step(a, B, S, T, 8300 + T)                      # a ran on the pair ...
        assert _names(a, T)[0] == "b2h_mw_sdpa"
        a.set_train_whole("valu")                       # ... and back on valu equals a model never switched
        assert _same(step(a, B, S, T, 8300 + T), step(b, B, S, T, 8300 + T))
        assert _names(a, T) == _names(b, T) == ("b2h_tt_sdpa", "b2h_tt_sdpa" if T <= 128 else "b2h_lt_sdpa")


def test_backward_runs_the_kernels_of_its_forward(cuda_device):
    B, S, T = 3, 17, 33
    m = whole_model(recipe_state(370, N_TOKENS, 1, 2), 0.1, cuda_device)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 8400))
    torch.manual_seed(8401)
    masks = m._draw_dropout_masks(B, S, T)
    _, g_all, dx_all = _step(m, tok, x, dy, masks)      # forward and backward on the pair
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(True)
    y = m._forward_train(tok, xd, masks)
    m.set_train_whole("valu")                           # switched between the two
    _set_handle(m, "valu")                              # and the handle with it
    y.backward(dy)
    assert _names(m, T) == ("b2h_mw_sdpa", "b2h_mw_sdpa")   # what the backward set the handle to
    assert all(torch.equal(a, p.grad) for a, p in zip(g_all, m._tensors())) and torch.equal(dx_all, xd.grad)
    _, g_valu, _ = _step(m, tok, x, dy, masks)          # the model says valu now: the next step runs it
    assert _names(m, T) == ("b2h_tt_sdpa", "b2h_tt_sdpa") and all(torch.isfinite(g).all() for g in g_valu)


# ---- 5. poisoned outputs, saved buffer and scratch; NaN right behind every operand; p = 0, 1; determinism --------
@pytest.mark.parametrize("B,S,T,with_dx", [(3, 9, 17, True), (2, 40, 100, False), (5, 1, 1, True)])
def test_outputs_fully_written_and_scratch_contents_irrelevant(B, S, T, with_dx, mw, cuda_device):
    """poison.launch through the C ABI with the handle on the route: saved and scratch buffers of exactly
    b2h_tpt_train_bytes, quiet NaNs right behind every operand; every output word is written and no bit changes against
    clean allocations.  A padded query row, key row or k-step that read past a tensor would differ."""
    base.test_outputs_fully_written_and_scratch_contents_irrelevant(B, S, T, with_dx, cuda_device)
    mw.all_on_route()


def test_p0_equals_eval_and_p1_drops_everything(mw, cuda_device):
    base.test_p0_equals_eval_and_p1_drops_everything(cuda_device)
    assert len(mw) == 2
    mw.all_on_route()


def test_bitwise_deterministic_across_runs_streams_and_batches(cuda_device):
    """base.test_bitwise_deterministic_across_runs_streams_and_batches at (8, 40, 100): two runs, a side stream, and
    dx of the sequences 0, 3 and 7 alone against their rows inside the batch."""
    B, S, T = 8, 40, 100
    dev = cuda_device
    m = whole_model(recipe_state(50, N_TOKENS, 2, 2), 0.1, dev)
    tok, x, dy = (t.to(dev) for t in _data(B, S, T, N_TOKENS, 51))
    torch.manual_seed(52)
    masks = m._draw_dropout_masks(B, S, T)
    _, g1, dx1 = _step(m, tok, x, dy, masks)
    _, g2, dx2 = _step(m, tok, x, dy, masks)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        _, g3, dx3 = _step(m, tok, x, dy, masks)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    for a, b, c in zip(g1, g2, g3):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(dx1, dx2) and torch.equal(dx1, dx3)
    for i in (0, 3, 7):                                 # dx of a sequence alone == inside the batch
        mi = {k: v[i:i + 1].contiguous() for k, v in masks.items()}
        _, _, dxi = _step(m, tok[i:i + 1], x[i:i + 1], dy[i:i + 1], mi)
        assert torch.equal(dxi[0], dx1[i])
    assert _names(m, T) == ("b2h_mw_sdpa", "b2h_mw_sdpa")


# ---- 6. graph capture ---------------------------------------------------------------------------------------------
def test_training_step_captured_in_graph_equals_eager(mw, cuda_device):
    base.test_training_step_captured_in_graph_equals_eager(cuda_device)   # (8, 20, 50), p = 0.1
    mw.all_on_route()


def test_training_step_captured_in_graph_as_first_use_equals_eager(cuda_device):
    B, S, T = 8, 20, 50
    state = recipe_state(90, N_TOKENS, 2, 2)
    tok, x, dy = (t.to(cuda_device) for t in _data(B, S, T, N_TOKENS, 91))
    eager = whole_model(state, 0.1, cuda_device)
    torch.manual_seed(92)
    masks = eager._draw_dropout_masks(B, S, T)
    _, eager_g, eager_dx = _step(eager, tok, x, dy, masks)
    m = train_model(state, 0.1, cuda_device).set_train_whole("mfma")   # a model that has not run yet
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
    assert _names(m, T) == ("b2h_mw_sdpa", "b2h_mw_sdpa")
    for a, p in zip(eager_g, m._tensors()):
        assert torch.equal(a, p.grad)
    assert torch.equal(eager_dx, xs.grad)


def test_trainer_recaptures_when_the_whole_route_changes(cuda_device):
    """GraphTrainer.epoch() across a set_train_whole change: two captures, and the parameters and Adam moments of
    train_epoch on a twin (test_graph_trainer_gpu._compare; the HDF5 fixture's 5 utterances at B = 2)."""
    def switch(model, opt):
        model.set_train_whole("mfma")
    trainer, m = gt._compare(cuda_device, gt._tpt, lambda: hps.DeviceLoader(gt._h5(), 2, 7, selection="first"),
                             between=switch, epochs=3, captures=2)
    assert trainer.replays == 4                         # 6 full steps: one eager and one capture per route
    assert m.train_whole == "mfma" and _names(m, 7) == ("b2h_mw_sdpa", "b2h_mw_sdpa")


# ---- 7. each switch alone and all three, on one batch, inside the bars -------------------------------------------
@pytest.mark.parametrize("B,S,T", [(2, 40, 100), (1, 40, 130)])
def test_each_switch_alone_and_all_three_inside_the_bars_on_the_same_batch(B, S, T, cuda_device):
    ne, nd, p, seed = 1, 2, 0.1, 8500 + T
    state = recipe_state(380, N_TOKENS, ne, nd)
    routes = [dict(whole="valu"), dict(whole="mfma"), dict(whole="valu", kernels="mfma"), dict(whole="valu", linear="mfma"),
              dict(whole="mfma", kernels="mfma", linear="mfma")]
    got, masks = _both_routes(state, p, B, S, T, seed, cuda_device, routes)
    tok, x, dy = _data(B, S, T, N_TOKENS, seed)
    y64, g64, dx64 = port_grads(tok, x, state, _cpu(masks), p, dy, torch.float64)
    _, g32, dx32 = port_grads(tok, x, state, _cpu(masks), p, dy, torch.float32)
    for route, (y, *grads) in zip(routes, got):
        assert float((y.cpu().double() - y64).abs().max()) <= _tol_y(y64), route
        for k, g, a, b in zip(param_keys(ne, nd) + ["dx"], grads, g64 + [dx64], g32 + [dx32]):
            assert_within_bar(g.cpu().double().numpy(), a.numpy(), float((b.double() - a).abs().max()), f"{route} {k}")
    if T <= 128:                                        # set_train_kernels alone changes nothing up to 128 frames
        assert all(torch.equal(a, b) for a, b in zip(got[0], got[2]))
