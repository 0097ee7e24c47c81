"""TextPoseTransformer on the GPU: parity with the reference's fixtures and, over a shape sweep, with the float64
checker (tpt_ref.Checker); batch independence and determinism bit for bit; poisoned output and workspace through the
C ABI; out-of-range token ids on the device; the shape limits.  One bound everywhere: max|y - y64| <= 2e-5, the
project's fp32 transformer bar (DESIGN.md sections 2, 9, 12) -- at least 10x the reference's own fp32 error on the
fixtures (tests/test_tpt_cpu.py asserts <= 2e-6 there) with outputs of magnitude ~2."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import poison
from tpt_ref import BAR, CASES, Checker, case_model, inputs, load_case, recipe_model

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 17), (3, 16, 16), (2, 17, 33), (2, 40, 100), (2, 128, 128), (3, 33, 128), (3, 128, 15)]
LAYERS = [(1, 1), (4, 4), (5, 2)]   # (encoder, decoder) layers; (4, 4) fills the memory K, V launch's eight stages
                                    # exactly, test_more_than_four_decoder_layers needs a second launch


def _sweep_recipe(n_enc, n_dec):
    # (4, 4) is the fixtures' default model itself
    return recipe_model(7, 1000, 4, 4) if (n_enc, n_dec) == (4, 4) else recipe_model(20 + n_enc, 100, n_enc, n_dec)


@functools.lru_cache(maxsize=None)
def sweep_model(n_enc, n_dec):
    """(CPU model by the fixtures' recipe, its float64 checker), built once and left unchanged."""
    model = _sweep_recipe(n_enc, n_dec)
    return model, Checker(model, torch.float64)


@functools.lru_cache(maxsize=None)
def gpu_model(n_enc, n_dec):
    return _sweep_recipe(n_enc, n_dec).to("cuda:0")


def err_of(y, ref):
    return float((y.detach().cpu().double() - torch.as_tensor(ref).double()).abs().max())


@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_reference(cuda_device, name):
    r = load_case(name)
    model = case_model(name).to(cuda_device)
    y = model(torch.from_numpy(r["tokens"]), torch.from_numpy(r["pose"]))
    assert y.shape == (r["B"], r["T"], 21, 2) and y.dtype == torch.float32 and y.grad_fn is None and not y.requires_grad
    err = err_of(y, r["y64"])
    print(f"{name}: max|y - y64| = {err:.3e}   (reference fp32: {np.abs(r['y32'] - r['y64']).max():.3e})")
    assert err <= BAR


@pytest.mark.parametrize("layers", LAYERS, ids=lambda l: f"enc{l[0]}_dec{l[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d_s%d_t%d" % s)
def test_shape_sweep(cuda_device, shape, layers):
    B, S, T = shape
    cpu, check = sweep_model(*layers)
    tok, pose = inputs(B, S, T, cpu.n_tokens, 1000 * S + T)
    y = gpu_model(*layers)(tok.to(cuda_device), pose.to(cuda_device))
    err = err_of(y, check(tok, pose))
    print(f"{shape} {layers}: max|y - y64| = {err:.3e}")
    assert err <= BAR


def test_more_than_four_decoder_layers(cuda_device):
    """Five decoder layers: the memory's K and V take a second chain launch (eight stages = four layers each)."""
    cpu = recipe_model(31, 100, 1, 5)
    tok, pose = inputs(3, 40, 33, 100, 5)
    y = recipe_model(31, 100, 1, 5).to(cuda_device)(tok, pose)
    assert err_of(y, Checker(cpu)(tok, pose)) <= BAR


def test_more_than_one_block_per_workgroup(cuda_device):
    """330 sequences = 258 blocks of 128 frames (104 of 128 tokens): the persistent chain's workgroups walk over
    more than one block each."""
    cpu, check = sweep_model(4, 4)
    tok, pose = inputs(330, 40, 100, cpu.n_tokens, 9)
    y = gpu_model(4, 4)(tok.to(cuda_device), pose.to(cuda_device))
    assert bool(torch.isfinite(y).all())
    pick = [0, 165, 329]
    err = err_of(y[pick], check(tok[pick], pose[pick]))
    print(f"(330, 40, 100) sequences {pick}: max|y - y64| = {err:.3e}")
    assert err <= BAR


def test_text_is_used(cuda_device):
    """Other token ids change the output, and the new output is again the checker's: the memory path is read."""
    r = load_case("default_b3_s40_t100")
    cpu, check = sweep_model(4, 4)
    model = gpu_model(4, 4)
    tok, pose = torch.from_numpy(r["tokens"]), torch.from_numpy(r["pose"])
    other = (tok + 17) % r["n_tokens"]
    y, y2 = model(tok, pose), model(other, pose)
    assert err_of(y, r["y64"]) <= BAR
    assert float((y - y2).abs().max()) > 1e-3
    assert err_of(y2, check(other, pose)) <= BAR


def test_batch_independence_and_determinism(cuda_device):
    cpu, _ = sweep_model(4, 4)
    model = gpu_model(4, 4)
    tok, pose = inputs(7, 40, 100, cpu.n_tokens, 11)
    tok, pose = tok.to(cuda_device), pose.to(cuda_device)
    y = model(tok, pose)
    assert torch.equal(y, model(tok, pose))                              # run to run
    for b in (0, 3, 6):                                                  # alone == inside the batch of 7
        assert torch.equal(model(tok[b:b + 1], pose[b:b + 1])[0], y[b]), b
    side = torch.cuda.Stream(cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        ys = model(tok, pose)
    side.synchronize()
    assert torch.equal(ys, y)                                            # on a second stream


def _abi(model):
    """(lib, handle) of a mirror whose weights are packed."""
    lib, _ = model._ensure_handle()
    return lib, model._handle


def _ws_bytes(model, B, S, T):
    lib, h = _abi(model)
    n = lib.b2h_tpt_workspace_bytes(h, B, S, T)
    per_token = 4 * (5 * 128 + 2 * 128 * model._geom[6])
    assert n == B * S * per_token + B * T * 3584                         # a pure function of (B, S, T) and the layers
    return n


def _call(model, B, S, T, ws_key="ws", ws_bytes=None):
    lib, h = _abi(model)
    nbytes = ws_bytes if ws_bytes is not None else _ws_bytes(model, B, S, T)
    return lambda p: lib.b2h_tpt_forward(h, p["tokens"], p["x"], p["y"], B, S, T, p[ws_key], nbytes, None)


@pytest.mark.parametrize("shape", [(3, 40, 100), (300, 17, 1)], ids=lambda s: "b%d_s%d_t%d" % s)
def test_poisoned_output_and_workspace(cuda_device, shape):
    B, S, T = shape
    cpu, check = sweep_model(4, 4)
    model = gpu_model(4, 4)
    tok, pose = inputs(B, S, T, cpu.n_tokens, 13)
    out = poison.launch(_call(model, B, S, T), {"tokens": tok, "x": pose}, {"y": (B, T, 21, 2)}, cuda_device,
                        scratch={"ws": _ws_bytes(model, B, S, T)})
    pick = [0, B // 2, B - 1]
    assert err_of(out["y"][pick], check(tok[pick], pose[pick])) <= BAR


def test_dirty_workspace_of_a_larger_call(cuda_device):
    """A workspace left behind by a (40, 128, 128) call: smaller calls read no word they have not written."""
    cpu, check = sweep_model(4, 4)
    model = gpu_model(4, 4)
    big = _ws_bytes(model, 40, 128, 128)
    dirty = poison.Guarded(big, poison.POISON, poison.POISON, cuda_device)
    tok, pose = inputs(40, 128, 128, cpu.n_tokens, 15)
    gi = {"tokens": poison.guarded_input(tok, True, cuda_device), "x": poison.guarded_input(pose, True, cuda_device)}
    gy = poison.guarded_output(4 * 40 * 128 * 42, True, cuda_device)
    rc = _call(model, 40, 128, 128, ws_bytes=big)({"tokens": gi["tokens"].ptr, "x": gi["x"].ptr, "y": gy.ptr, "ws": dirty.ptr})
    torch.cuda.synchronize(cuda_device)
    assert rc == 0 and dirty.guards_intact() and gy.guards_intact()
    assert int((gy.body == poison._i32(poison.POISON)).sum()) == 0
    for B, S, T in ((7, 9, 33), (3, 128, 128)):
        tok, pose = inputs(B, S, T, cpu.n_tokens, 17 + B)
        out = poison.launch(_call(model, B, S, T, ws_bytes=big), {"tokens": tok, "x": pose}, {"y": (B, T, 21, 2)},
                            cuda_device, scratch={"ws": dirty})
        assert err_of(out["y"], check(tok, pose)) <= BAR, (B, S, T)


def test_out_of_range_ids_on_the_device(cuda_device):
    """Ids n_tokens and -1 in one sequence: nothing outside the table is read (64 KB guard bands around every
    operand, so even a wrong gather would stay inside an allocation), that sequence's output is NaN, the others are
    the clean run's bit for bit."""
    cpu, _ = sweep_model(1, 1)
    model = gpu_model(1, 1)
    B, S, T = 3, 9, 20
    tok, pose = inputs(B, S, T, cpu.n_tokens, 19)
    bad = tok.clone()
    bad[1, 2], bad[1, 7] = cpu.n_tokens, -1
    ys = []
    for t in (tok, bad):
        gt, gx = poison.guarded_input(t, True, cuda_device), poison.guarded_input(pose, True, cuda_device)
        gy = poison.guarded_output(4 * B * T * 42, True, cuda_device)
        gw = poison.guarded_output(_ws_bytes(model, B, S, T), True, cuda_device)
        rc = _call(model, B, S, T)({"tokens": gt.ptr, "x": gx.ptr, "y": gy.ptr, "ws": gw.ptr})
        torch.cuda.synchronize(cuda_device)
        assert rc == 0
        assert all(g.guards_intact() for g in (gt, gx, gy, gw))
        assert torch.equal(gt.body, t.to(cuda_device).reshape(-1).view(torch.int32))
        ys.append(gy.view(torch.float32, (B, T, 21, 2)).clone())
    clean, got = ys
    assert bool(torch.isfinite(clean).all())
    assert bool(torch.isnan(got[1]).all())
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    # the Python mirror passes device ids through unchecked (no synchronisation): the same NaN rows
    y = model(bad.to(cuda_device), pose.to(cuda_device))
    assert bool(torch.isnan(y[1]).all()) and torch.equal(y[0], clean[0])
    with pytest.raises(IndexError):
        model(bad, pose)                                                  # host ids: nn.Embedding's error


def test_errors_and_weight_replacement(cuda_device):
    from hand_pose_sl_amd import _lib
    cpu = recipe_model(41, 60, 1, 1)
    model = recipe_model(41, 60, 1, 1).to(cuda_device)
    pose = torch.zeros((2, 129, 12, 2))
    with pytest.raises(RuntimeError, match="128"):
        model(torch.zeros((2, 129), dtype=torch.int64), pose[:, :5])       # S = 129
    with pytest.raises(RuntimeError, match="128"):
        model(torch.zeros((2, 5), dtype=torch.int64), pose)                # T = 129
    y = model(torch.zeros((0, 5), dtype=torch.int64), torch.zeros((0, 9, 12, 2)))
    assert y.shape == (0, 9, 21, 2) and y.device.type == "cuda"
    lib, h = _abi(model)
    assert lib.b2h_tpt_forward(h, None, None, None, 2, 5, 9, None, 0, None) == _lib.ERR_INVALID       # NULL pointers
    ws = torch.empty(_ws_bytes(model, 2, 5, 9), dtype=torch.uint8, device=cuda_device)
    tok, x = inputs(2, 5, 9, 60, 23)
    tokd, xd, yd = tok.to(cuda_device), x.to(cuda_device), torch.empty((2, 9, 21, 2), device=cuda_device)
    args = (ctypes.c_void_p(tokd.data_ptr()), ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(yd.data_ptr()))
    assert lib.b2h_tpt_forward(h, *args, 2, 5, 9, ctypes.c_void_p(ws.data_ptr()), ws.numel() - 1, None) == _lib.ERR_INVALID
    assert lib.b2h_tpt_forward(h, *args, 2, 0, 9, ctypes.c_void_p(ws.data_ptr()), ws.numel(), None) == _lib.ERR_SHAPE
    assert lib.b2h_tpt_forward(h, *args, 2, 5, 0, ctypes.c_void_p(ws.data_ptr()), ws.numel(), None) == _lib.ERR_SHAPE
    assert lib.b2h_tpt_forward(h, None, None, None, 0, 5, 9, None, 0, None) == _lib.OK   # B == 0: nothing to touch
    fresh = ctypes.c_void_p()
    assert lib.b2h_tpt_create(60, 24, 4, 128, 42, 1, 1, ctypes.byref(fresh)) == 0
    assert lib.b2h_tpt_forward(fresh, *args, 2, 5, 9, ctypes.c_void_p(ws.data_ptr()), ws.numel(), None) == _lib.ERR_NO_WEIGHTS
    arr = (ctypes.c_void_p * 38)()
    assert lib.b2h_tpt_load_weights(fresh, arr, 38, 1) == _lib.ERR_INVALID              # 39 tensors expected
    lib.b2h_tpt_destroy(fresh)
    # an in-place update of a parameter is seen by the next forward
    before = model(tok, x)
    assert err_of(before, Checker(cpu)(tok, x)) <= BAR
    with torch.no_grad():
        for m in (cpu, model):
            m.transformer.decoder.layers[0].multihead_attn.in_proj_bias.add_(0.25)
            m.token_embedding.weight.add_(0.125)
    after = model(tok, x)
    assert float((after - before).abs().max()) > 1e-3
    assert err_of(after, Checker(cpu)(tok, x)) <= BAR
