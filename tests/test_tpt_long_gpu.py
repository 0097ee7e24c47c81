"""TextPoseTransformer.forward_fused / b2h_tpt_forward_fused on the GPU: targets of more than 128 frames (the
reference's CLIs default to 200), the item transforms inside the model's kernels, the CLI and validate().

Everything is compared with tpt_ref.Checker -- the mirror's own torch modules on the CPU in float64 -- at
tpt_ref.BAR = 2e-5 on max|y - y64| (times the factor in pixel units), in both arithmetics.  The reference's own
fp32 forward is within 3e-6 of float64 on every input used here (measured on the CPU: 1.3e-6 to 2.9e-6; outputs
have magnitude 2 to 3), so the bar keeps about 7x room."""
import ctypes
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import poison
from conftest import load_golden
from tpt_ref import BAR, TPT, Checker, inputs, recipe_model

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "f16x3"]
FACTOR = 1280.0
OFF = dict(dif_encoding=False, normalize=False, denormalize=False, mask_tail=False)


def _recipe(n_enc, n_dec):
    return recipe_model(7, 1000, 4, 4) if (n_enc, n_dec) == (4, 4) else recipe_model(20 + n_enc, 100, n_enc, n_dec)


@functools.lru_cache(maxsize=None)
def cpu_model(n_enc, n_dec):
    """(CPU model by the fixtures' recipe, its float64 checker), built once and left unchanged."""
    model = _recipe(n_enc, n_dec)
    return model, Checker(model, torch.float64)


@functools.lru_cache(maxsize=None)
def gpu_model(n_enc, n_dec):
    return _recipe(n_enc, n_dec).to("cuda:0")


def model_for(layers, precision):
    return gpu_model(*layers).set_precision(precision)


@functools.lru_cache(maxsize=None)
def reference(layers, shape):
    """(tokens, pose, float64 prediction) of tpt_ref.inputs at `shape`: computed once, shared, left unchanged."""
    B, S, T = shape
    cpu, check = cpu_model(*layers)
    tok, pose = inputs(B, S, T, cpu.n_tokens, 1000 * S + T)
    return tok, pose, check(tok, pose)


def err_of(y, ref):
    return float((y.detach().cpu().double() - torch.as_tensor(ref).double()).abs().max())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", [(2, 40, 100), (3, 33, 128)], ids=lambda s: "b%d_s%d_t%d" % s)
def test_same_bits_below_the_limit(cuda_device, shape, precision):
    B, S, T = shape
    model = model_for((4, 4), precision)
    tok, pose = inputs(B, S, T, 1000, 1000 * S + T)
    tok, pose = tok.to(cuda_device), pose.to(cuda_device)
    assert torch.equal(model.forward_fused(tok, pose, **OFF), model(tok, pose))


SWEEP = [((4, 4), s) for s in [(2, 1, 129), (2, 17, 130), (3, 33, 144), (2, 40, 200), (1, 128, 257), (2, 40, 512)]] + \
        [((1, 1), (1, 16, 1024)), ((1, 1), (2, 17, 130)), ((5, 2), (2, 40, 200))]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("layers,shape", SWEEP, ids=lambda v: "_".join(str(i) for i in v))
def test_shape_sweep(cuda_device, layers, shape, precision):
    tok, pose, ref = reference(layers, shape)
    y = model_for(layers, precision).forward_fused(tok.to(cuda_device), pose.to(cuda_device), **OFF)
    assert y.shape == ref.shape and y.dtype == torch.float32
    err = err_of(y, ref)
    print(f"{shape} {layers} {precision}: max|y - y64| = {err:.3e}")
    assert err <= BAR


@functools.lru_cache(maxsize=None)
def long_fixture():
    with np.load(os.path.join(TPT, "long_default_b2_s40_t200.npz")) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("setting", ["norm", "chest"])
def test_the_references_fixture(cuda_device, setting, precision):
    """The reference's own pipeline at its CLI's default shape: transforms, model, mask_output, prediction *= 1280."""
    r = long_fixture()
    model = model_for((4, 4), precision)
    chest = setting == "chest"
    y = model.forward_fused(torch.from_numpy(r["tokens"]), torch.from_numpy(r["body"]), torch.from_numpy(r["n_frames"]),
                            dif_encoding=chest, normalize=True, denormalize=True, mask_tail=chest)
    err = err_of(y, r["y64_" + setting])
    ref32 = np.abs(r["y32_" + setting].astype(np.float64) - r["y64_" + setting]).max()
    print(f"{setting} {precision}: max|y - y64| = {err:.3e} px (reference fp32: {ref32:.3e} px)")
    assert err <= BAR * FACTOR
    if chest:
        n = int(r["n_frames"][1])
        assert n < y.shape[1] and bool((y[1, n:] == 0.0).all()) and bool((y[1, :n] != 0.0).any())


FLAGS = {"chest": dict(dif_encoding=True), "normalize": dict(normalize=True), "denormalize": dict(denormalize=True),
         "mask": dict(mask_tail=True), "all": dict(dif_encoding=True, normalize=True, denormalize=True, mask_tail=True)}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("shape", [(3, 40, 200), (3, 9, 20)], ids=lambda s: "b%d_s%d_t%d" % s)
def test_each_flag_alone_and_all_together(cuda_device, shape, flags, precision):
    B, S, T = shape
    cpu, check = cpu_model(4, 4)
    g = torch.Generator().manual_seed(100 * S + T)
    tok = torch.randint(0, cpu.n_tokens, (B, S), generator=g)
    body = torch.rand((B, T, 12, 2), generator=g) * FACTOR
    n_frames = torch.tensor([T, 1, T - 63])
    kw = dict(OFF, **FLAGS[flags])
    # the transforms restated in float64 (steps/utils.py:180-210,309-312; traintest.py:270-271)
    x = body.double()
    if kw["dif_encoding"]:
        x = x - x[:, :, 1:2]
    if kw["normalize"]:
        x = x / FACTOR
    want = check(tok, x)
    if kw["denormalize"]:
        want = want * FACTOR
    if kw["mask_tail"]:
        for i, n in enumerate(n_frames.tolist()):
            want[i, n:] = 0
    y = model_for((4, 4), precision).forward_fused(tok.to(cuda_device), body.to(cuda_device), n_frames, factor=FACTOR, **kw)
    err = err_of(y, want)
    bar = BAR * FACTOR if kw["denormalize"] else BAR
    print(f"{shape} {flags} {precision}: max|y - y64| = {err:.3e} (bar {bar:.1e})")
    assert err <= bar
    if kw["mask_tail"]:
        for i, n in enumerate(n_frames.tolist()):
            assert bool((y[i, max(n, 0):] == 0.0).all())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_running_maximum_moves_to_later_key_blocks(cuda_device, precision):
    B, S, T = 2, 40, 300
    cpu, check = cpu_model(4, 4)
    tok, pose = inputs(B, S, T, cpu.n_tokens, 1000 * S + T)
    pose = pose * (1 + 8 * torch.arange(T, dtype=torch.float32) / T)[None, :, None, None]
    y = model_for((4, 4), precision).forward_fused(tok.to(cuda_device), pose.to(cuda_device), **OFF)
    err = err_of(y, check(tok, pose))
    print(f"ramped (2, 40, 300) {precision}: max|y - y64| = {err:.3e}")
    assert err <= BAR


@pytest.mark.parametrize("precision", PRECISIONS)
def test_more_work_than_workgroups(cuda_device, precision):
    """300 sequences x 4 heads x 2 query blocks; batch independence and determinism bit for bit."""
    shape = (300, 17, 129)
    tok, pose, ref = reference((1, 1), shape)
    model = model_for((1, 1), precision)
    tok, pose = tok.to(cuda_device), pose.to(cuda_device)
    y = model.forward_fused(tok, pose, **OFF)
    err = err_of(y, ref)
    print(f"{shape} {precision}: max|y - y64| = {err:.3e}")
    assert err <= BAR
    assert torch.equal(model.forward_fused(tok[7:8], pose[7:8], **OFF)[0], y[7])      # alone == inside the batch
    assert torch.equal(model.forward_fused(tok, pose, **OFF), y)                      # run to run
    side = torch.cuda.Stream(cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        ys = model.forward_fused(tok, pose, **OFF)
    side.synchronize()
    assert torch.equal(ys, y)                                                         # on a second stream


def _abi(model):
    lib, _ = model._ensure_handle()
    return lib, model._handle


def _ws_bytes(model, B, S, T):
    lib, h = _abi(model)
    return lib.b2h_tpt_workspace_bytes(h, B, S, T)


def _call(model, B, S, T, nbytes, flags=0, factor=1.0):
    from hand_pose_sl_amd.transformer_enc import TENC_KERNELS
    lib, h = _abi(model)
    assert lib.b2h_tpt_set_kernel(h, TENC_KERNELS[model.precision]) == 0
    return lambda p: lib.b2h_tpt_forward_fused(h, p["tokens"], p["x"], p["y"], B, S, T, flags, factor, None, p["ws"], nbytes,
                                               None)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_poisoned_output_and_workspace(cuda_device, precision):
    shape = (3, 40, 200)
    B, S, T = shape
    cpu, check = cpu_model(4, 4)
    model = model_for((4, 4), precision)
    tok, pose = inputs(B, S, T, cpu.n_tokens, 13)
    nbytes = _ws_bytes(model, B, S, T)
    out = poison.launch(_call(model, B, S, T, nbytes), {"tokens": tok, "x": pose}, {"y": (B, T, 21, 2)}, cuda_device,
                        scratch={"ws": nbytes})
    assert err_of(out["y"], check(tok, pose)) <= BAR
    assert torch.equal(out["y"].cpu(), model.forward_fused(tok, pose, **OFF).cpu())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dirty_workspace_of_a_larger_call(cuda_device, precision):
    """A workspace left behind by a (4, 128, 512) call: a smaller call reads no word it has not written."""
    cpu, check = cpu_model(4, 4)
    model = model_for((4, 4), precision)
    big = _ws_bytes(model, 4, 128, 512)
    dirty = poison.Guarded(big, poison.POISON, poison.POISON, cuda_device)
    tok, pose = inputs(4, 128, 512, cpu.n_tokens, 15)
    gi = {"tokens": poison.guarded_input(tok, True, cuda_device), "x": poison.guarded_input(pose, True, cuda_device)}
    gy = poison.guarded_output(4 * 4 * 512 * 42, True, cuda_device)
    rc = _call(model, 4, 128, 512, big)({"tokens": gi["tokens"].ptr, "x": gi["x"].ptr, "y": gy.ptr, "ws": dirty.ptr})
    torch.cuda.synchronize(cuda_device)
    assert rc == 0 and dirty.guards_intact() and gy.guards_intact()
    assert int((gy.body == poison._i32(poison.POISON)).sum()) == 0
    B, S, T = 2, 40, 200
    tok, pose, ref = reference((4, 4), (B, S, T))
    out = poison.launch(_call(model, B, S, T, big), {"tokens": tok, "x": pose}, {"y": (B, T, 21, 2)}, cuda_device,
                        scratch={"ws": dirty})
    assert err_of(out["y"], ref) <= BAR


@pytest.mark.parametrize("precision", PRECISIONS)
def test_out_of_range_ids_on_the_device(cuda_device, precision):
    cpu, _ = cpu_model(1, 1)
    model = model_for((1, 1), precision)
    B, S, T = 3, 9, 200
    tok, pose = inputs(B, S, T, cpu.n_tokens, 19)
    bad = tok.clone()
    bad[1, 2], bad[1, 7] = cpu.n_tokens, -1
    nbytes = _ws_bytes(model, B, S, T)
    ys = []
    for t in (tok, bad):
        gt, gx = poison.guarded_input(t, True, cuda_device), poison.guarded_input(pose, True, cuda_device)
        gy = poison.guarded_output(4 * B * T * 42, True, cuda_device)
        gw = poison.guarded_output(nbytes, True, cuda_device)
        rc = _call(model, B, S, T, nbytes)({"tokens": gt.ptr, "x": gx.ptr, "y": gy.ptr, "ws": gw.ptr})
        torch.cuda.synchronize(cuda_device)
        assert rc == 0
        assert all(g.guards_intact() for g in (gt, gx, gy, gw))
        ys.append(gy.view(torch.float32, (B, T, 21, 2)).clone())
    clean, got = ys
    assert bool(torch.isfinite(clean).all())
    assert bool(torch.isnan(got[1]).all())
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


def test_limits_and_errors(cuda_device):
    from hand_pose_sl_amd import _lib
    model = model_for((1, 1), "fp32")
    lib, h = _abi(model)
    B = 2
    ws = torch.empty(_ws_bytes(model, B, 128, 1024), dtype=torch.uint8, device=cuda_device)
    tok = torch.zeros((B, 129), dtype=torch.int64, device=cuda_device)
    x = torch.zeros((B, 1025, 12, 2), device=cuda_device)
    y = torch.empty((B, 1025, 21, 2), device=cuda_device)
    p = [ctypes.c_void_p(t.data_ptr()) for t in (tok, x, y)]
    w = ctypes.c_void_p(ws.data_ptr())

    def call(S, T, nbytes=ws.numel()):
        return lib.b2h_tpt_forward_fused(h, *p, B, S, T, 0, 1.0, None, w, nbytes, None)
    assert call(40, 1025) == _lib.ERR_SHAPE
    assert call(129, 200) == _lib.ERR_SHAPE
    assert call(40, 0) == _lib.ERR_SHAPE
    assert call(40, 200, _ws_bytes(model, B, 40, 200) - 16) == _lib.ERR_INVALID
    assert call(40, 200, _ws_bytes(model, B, 40, 200)) == _lib.OK
    assert lib.b2h_tpt_forward_fused(h, *p, B, 40, 200, _lib.POST_MASK_TAIL, 1.0, None, w, ws.numel(), None) == _lib.ERR_INVALID
    torch.cuda.synchronize(cuda_device)
    with pytest.raises(RuntimeError, match="1024"):
        model.forward_fused(tok[:, :5], x, **OFF)                            # T = 1025 through _lib.check
    with pytest.raises(RuntimeError, match="128"):
        model(tok[:, :5], x[:, :129])                                        # the plain forward keeps its limit
    with pytest.raises(RuntimeError):
        model.forward_fused(tok[:, :5], x[:, :200], torch.tensor([1, 2, 3]), mask_tail=True)    # n_frames shape


def _write_utterance(tmp_path):
    rec = load_golden("openpose_long_n30_m20")
    frames = json.loads(str(rec["frames_json"]))
    src = tmp_path / "utt"
    src.mkdir()
    for i, fr in enumerate(frames):
        (src / f"utt_{i:012d}_keypoints.json").write_text(json.dumps(fr))
    return src, frames


def test_cli_end_to_end(tmp_path, cuda_device):
    """`--model TextPoseTransformer` at the default --max-frames 200: 30 frames padded to 200 by repeating frame 0."""
    from hand_pose_sl_amd import infer, openpose
    src, frames = _write_utterance(tmp_path)
    cpu, check = cpu_model(4, 4)
    ckpt = tmp_path / "best_model.pth"
    torch.save(cpu.state_dict(), ckpt)
    ids = [5, 17, 999, 3, 42, 7, 1]
    tokens = tmp_path / "tokens.json"
    tokens.write_text(json.dumps({"utt": ids}))
    item = openpose.load_utterance(frames, 200)
    assert item["n_frames"] == 30 and item["body_kp"].shape == (200, 12, 2)
    want = check(torch.tensor([infer.pad_tokens(ids)]), torch.from_numpy(item["body_kp"][None]).double() / FACTOR)[0] * FACTOR
    for precision in PRECISIONS:
        out = tmp_path / ("out_" + precision)
        infer.main(["--data", str(src), "--model", "TextPoseTransformer", "--model-checkpoint", str(ckpt),
                    "--output-folder", str(out), "--tokens", str(tokens), "--precision", precision])
        files = sorted(os.listdir(out))
        assert len(files) == 30
        worst = 0.0
        for i, f in enumerate(files):
            got = np.array(json.load(open(out / f))["people"][0]["hand_right_keypoints_2d"]).reshape(21, 3)
            worst = max(worst, float(np.abs(got[:, :2] - want[i].numpy()).max()))
            assert (got[:, 2] == 1.0).all()
        print(f"CLI {precision}: max|y - y64| = {worst:.3e} px")
        assert worst <= BAR * FACTOR


@pytest.mark.parametrize("precision", PRECISIONS)
def test_validate(cuda_device, precision):
    import hand_pose_sl_amd as hps
    B, S, T = 3, 40, 200
    cpu, check = cpu_model(4, 4)
    model = model_for((4, 4), precision)
    batches, want = [], {"L1": [], "confL1": []}
    for i in range(2):
        g = torch.Generator().manual_seed(700 + i)
        tok, pose = inputs(B, S, T, cpu.n_tokens, 800 + i)
        target = torch.rand((B, T, 21, 2), generator=g) - 0.5
        conf = torch.rand((B, T, 21), generator=g)
        n_frames = torch.tensor([T, 129, 64 + i])
        batches.append({"text_tokens": tok, "input_kp": pose, "target_kp": target, "n_frames": n_frames, "target_conf": conf})
        pred = check(tok, pose)
        l1 = conf_l1 = 0.0
        for b, n in enumerate(n_frames.tolist()):
            d = pred[b, :n] - target[b, :n].double()
            l1 += float(d.abs().mean())
            conf_l1 += float((d * conf[b, :n].double().unsqueeze(2)).abs().mean())
        want["L1"].append(l1 / B)
        want["confL1"].append(conf_l1)
    for lname, crit, tol in (("L1", hps.maskedPoseL1(), BAR), ("confL1", hps.poderatedPoseL1(), B * BAR)):
        expect = float(np.mean(want[lname]))
        got = hps.validate(model, batches, loss=lname)
        got2 = hps.validate(model, batches, crit, torch.device("cuda"), SimpleNamespace(model="TextPoseTransformer", loss=lname))
        print(f"validate {lname} {precision}: {got:.9f} vs {expect:.9f}")
        assert abs(got - expect) <= tol and abs(got2 - expect) <= tol
    with pytest.raises(ValueError):
        hps.validate(model, batches, None, None, SimpleNamespace(model="Conv", loss="L1"))
