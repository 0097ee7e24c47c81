"""TextPoseTransformer with `set_precision("f16x3")` on the GPU: every Linear and both attention products on three
v_mfma_f32_16x16x32_f16 of f16 hi + lo operands, Q, K, V projected inside the attention kernels (b2h_attn_qkv_h3 for
the two self-attentions, b2h_attn_cross_h3 for the memory).  The bound is the fp32 path's, everywhere:
max|y - y64| <= tpt_ref.BAR = 2e-5 against the float64 checker.  A CPU emulation of the split (operands rounded to
f16 hi + lo, hi.hi + hi.lo + lo.hi, fp32 elsewhere) gives 1.3e-6 .. 2.3e-6 on the fixtures and at worst 3.1e-6 over
the sweep below, so the bar has about 6x room over the arithmetic itself."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import poison
from test_tpt_gpu import err_of, sweep_model   # the CPU models and float64 checkers, built once for both files
from tpt_ref import BAR, CASES, Checker, build, case_model, inputs, load_case, recipe_model

pytestmark = pytest.mark.gpu

# tests/test_tpt_gpu.py's sweep: fewer query tiles than key tiles (3, 128, 15: one wave projects eight key tiles), more
# query tiles than key tiles (2, 1, 17), (2, 17, 33), (2, 40, 100): idle projector waves; odd key-tile counts at S = 1,
# 33, 40 (the zeroed V^T slots); S and T on both sides of a tile edge; the single row
SHAPES = [(1, 1, 1), (2, 1, 17), (3, 16, 16), (2, 17, 33), (2, 40, 100), (2, 128, 128), (3, 33, 128), (3, 128, 15)]
LAYERS = [(1, 1), (4, 4), (5, 2)]


@functools.lru_cache(maxsize=None)
def gpu_model(n_enc, n_dec):
    cpu, _ = sweep_model(n_enc, n_dec)
    model = build(cpu.n_tokens, n_enc, n_dec).eval()
    model.load_state_dict(cpu.state_dict())
    return model.to("cuda:0").set_precision("f16x3")


@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_reference(cuda_device, name):
    r = load_case(name)
    model = case_model(name).to(cuda_device).set_precision("f16x3")
    y = model(torch.from_numpy(r["tokens"]), torch.from_numpy(r["pose"]))
    assert y.shape == (r["B"], r["T"], 21, 2) and y.dtype == torch.float32
    err = err_of(y, r["y64"])
    print(f"f16x3 {name}: max|y - y64| = {err:.3e}   (reference fp32: {np.abs(r['y32'] - r['y64']).max():.3e})")
    assert err <= BAR


@pytest.mark.parametrize("layers", LAYERS, ids=lambda l: f"enc{l[0]}_dec{l[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d_s%d_t%d" % s)
def test_shape_sweep(cuda_device, shape, layers):
    B, S, T = shape
    cpu, check = sweep_model(*layers)
    tok, pose = inputs(B, S, T, cpu.n_tokens, 1000 * S + T)
    y = gpu_model(*layers)(tok.to(cuda_device), pose.to(cuda_device))
    err = err_of(y, check(tok, pose))
    print(f"f16x3 {shape} {layers}: max|y - y64| = {err:.3e}")
    assert err <= BAR


@pytest.mark.parametrize("shape", [(330, 40, 100), (200, 128, 15)], ids=lambda s: "b%d_s%d_t%d" % s)
def test_persistent_workgroups_walk_several_passes(cuda_device, shape):
    """The attention grids serve 64 sequences per pass on 256 CUs: several passes, both K/V buffers."""
    B, S, T = shape
    cpu, check = sweep_model(4, 4)
    tok, pose = inputs(B, S, T, cpu.n_tokens, 9)
    y = gpu_model(4, 4)(tok.to(cuda_device), pose.to(cuda_device))
    assert bool(torch.isfinite(y).all())
    pick = [0, B // 2, B - 1]
    err = err_of(y[pick], check(tok[pick], pose[pick]))
    print(f"f16x3 {shape} sequences {pick}: max|y - y64| = {err:.3e}")
    assert err <= BAR


def test_batch_independence_and_determinism(cuda_device):
    """135 sequences = passes 0, 1, 2 of a 64-sequence grid: a sequence's bits do not depend on the slot, the pass or
    the K/V buffer that handled it."""
    cpu, _ = sweep_model(4, 4)
    model = gpu_model(4, 4)
    tok, pose = inputs(135, 40, 100, cpu.n_tokens, 11)
    tok, pose = tok.to(cuda_device), pose.to(cuda_device)
    y = model(tok, pose)
    assert torch.equal(y, model(tok, pose))                              # run to run
    for b in (0, 64, 70, 134):                                           # alone == inside the batch
        assert torch.equal(model(tok[b:b + 1], pose[b:b + 1])[0], y[b]), b
    side = torch.cuda.Stream(cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        ys = model(tok, pose)
    side.synchronize()
    assert torch.equal(ys, y)                                            # on a second stream


def test_the_switch(cuda_device):
    from hand_pose_sl_amd import _lib
    cpu = recipe_model(43, 80, 2, 2)
    model = recipe_model(43, 80, 2, 2).to(cuda_device)
    tok, pose = inputs(5, 40, 100, 80, 21)
    want = Checker(cpu)(tok, pose)
    y0 = model(tok, pose)
    y1 = model.set_precision("f16x3")(tok, pose)
    y2 = model.set_precision("fp32")(tok, pose)
    assert torch.equal(y0, y2)                                           # fp32 is bit for bit what it was
    assert err_of(y0, want) <= BAR and err_of(y1, want) <= BAR
    assert not torch.equal(y1, y0)                                       # and f16x3 is another computation
    lib, h = model._ensure_handle()[0], model._handle
    assert lib.b2h_tpt_set_kernel(h, 2) == _lib.ERR_INVALID and lib.b2h_tpt_set_kernel(h, -1) == _lib.ERR_INVALID
    with torch.no_grad():
        model.hidden2pose_projection.weight[0, 0] = 70000.0
    with pytest.raises(RuntimeError, match="f16 range"):
        model.set_precision("f16x3")(tok, pose)
    assert model.set_precision("fp32")(tok, pose).shape == (5, 100, 21, 2)


def _abi(model):
    """(lib, handle) of a mirror whose weights are packed, with the f16x3 kernels selected."""
    lib, _ = model._ensure_handle()
    assert lib.b2h_tpt_set_kernel(model._handle, 1) == 0
    return lib, model._handle


def _ws_bytes(model, B, S, T):
    lib, h = _abi(model)
    return lib.b2h_tpt_workspace_bytes(h, B, S, T)


def _call(model, B, S, T, ws_bytes=None):
    lib, h = _abi(model)
    nbytes = ws_bytes if ws_bytes is not None else _ws_bytes(model, B, S, T)
    return lambda p: lib.b2h_tpt_forward(h, p["tokens"], p["x"], p["y"], B, S, T, p["ws"], nbytes, None)


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
    """Ids n_tokens and -1 in sequence 1: nothing outside the table is read (guard bands around every operand), that
    sequence's output is NaN, the others are the clean run's bit for bit (NaN memory rows stay in their sequence)."""
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


def test_in_place_weight_edits_are_repacked(cuda_device):
    """The per-head [Q_h | K_h | V_h] blobs and the embedding table follow an in-place edit of the parameters."""
    cpu = recipe_model(41, 60, 1, 1)
    model = recipe_model(41, 60, 1, 1).to(cuda_device).set_precision("f16x3")
    tok, x = inputs(2, 5, 9, 60, 23)
    before = model(tok, x)
    assert err_of(before, Checker(cpu)(tok, x)) <= BAR
    with torch.no_grad():
        for m in (cpu, model):
            m.transformer.decoder.layers[0].multihead_attn.in_proj_weight.add_(0.03)
            m.transformer.encoder.layers[0].self_attn.in_proj_bias.add_(0.25)
            m.transformer.decoder.layers[0].self_attn.in_proj_bias.add_(0.25)
            m.token_embedding.weight.add_(0.125)
    after = model(tok, x)
    assert float((after - before).abs().max()) > 1e-3
    assert err_of(after, Checker(cpu)(tok, x)) <= BAR


def test_training_is_unaffected(cuda_device):
    """_TptTrainFn is exact fp32 whatever the precision: output and every gradient bit for bit."""
    src = recipe_model(45, 70, 2, 2).state_dict()
    tok, pose = inputs(3, 9, 20, 70, 25)
    tok, pose = tok.to(cuda_device), pose.to(cuda_device)
    results = []
    for precision in ("fp32", "f16x3"):
        model = build(70, 2, 2, dropout=0.0)
        model.load_state_dict(src)
        model = model.to(cuda_device).set_precision(precision).train()
        y = model(tok, pose)
        assert y.requires_grad
        y.square().sum().backward()
        results.append((y.detach(), [p.grad for p in model.parameters()]))
    (y0, g0), (y1, g1) = results
    assert torch.equal(y0, y1)
    assert len(g0) == len(g1) and all(a is not None and torch.equal(a, b) for a, b in zip(g0, g1))
