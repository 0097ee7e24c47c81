"""Key-padding masks on the MI355X: text_lengths / frame_lengths through every training attention
route and the fp32 inference kernels, b2h_token_lengths, and the masked entry points of the C ABI.

Oracle: torch's nn.Transformer on the CPU in float64 with the three key-padding masks (tests/padding_ref.py), for the
cases with dropout its masked port with the keep-masks the kernels used.  Bars, the project's own: y within 2e-5 of
float64 at the valid frames, gradients within train_ref.bar (4 * max|g32_ref - g64| + 1e-6 * max|g64|) per tensor.
Everything that the feature promises bit for bit is compared with torch.equal on runs of the C ABI under
tests/poison.py, whose buffers -- outputs, gradients, saved activations and scratch -- start as a NaN pattern no kernel
writes: an unwritten dK / dV row shows."""
import ctypes

import pytest
import torch

import hand_pose_sl_amd as hps
import padding_ref as ref
from hand_pose_sl_amd import _lib
from hand_pose_sl_amd.transformer_enc import TENC_KERNELS
from poison import launch as poisoned_launch
from test_padding_masks_cpu import TOKEN_ROWS
from tpt_train_ref import assert_within_bar, cpu_masks, param_keys, train_model

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
ROUTES = {"default": {}, "whole_mfma": dict(whole="mfma"), "blocked_mfma": dict(kernels="mfma"),
          "all_mfma": dict(whole="mfma", kernels="mfma", linear="mfma")}
# the attention kernels a route must resolve to: (encoder, decoder at T <= 128, decoder beyond)
NAMES = {"default": ("b2h_tt_sdpa", "b2h_tt_sdpa", "b2h_lt_sdpa"), "whole_mfma": ("b2h_mw_sdpa", "b2h_mw_sdpa", "b2h_lt_sdpa"),
         "blocked_mfma": ("b2h_tt_sdpa", "b2h_tt_sdpa", "b2h_mt_sdpa"), "all_mfma": ("b2h_mw_sdpa", "b2h_mw_sdpa", "b2h_mt_sdpa")}
PARITY = [(c, r) for c in ("whole", "blocked", "deep") for r in ("default", "whole_mfma", "blocked_mfma")] + [("blocked", "all_mfma")]


def _model(name, route, p, dev):
    """A training model of the case's geometry on `route`, the handle switched too (for the calls of the C ABI)."""
    kw = ROUTES[route]
    m = train_model(ref.case_state(name), p, dev)
    m.set_train_whole(kw.get("whole", "valu")).set_train_kernels(kw.get("kernels", "valu")).set_train_linear(kw.get("linear", "valu"))
    lib, _ = m._ensure_created()
    for setter, value in m._train_route():
        assert getattr(lib, setter)(m._handle, value) == _lib.OK
    enc, dec, far = (lib.b2h_tpt_train_enc_attn_name(m._handle).decode(), lib.b2h_tpt_train_attn_name(m._handle, 128).decode(),
                     lib.b2h_tpt_train_attn_name(m._handle, 129).decode())
    assert (enc, dec, far) == NAMES[route]
    assert lib.b2h_tpt_train_linear_name(m._handle).decode() == ("b2h_ml_linear" if kw.get("linear") == "mfma" else "b2h_tt_linear")
    return m


def _abi_step(m, tok, x, dy, masks, p, tl, fl, dev, masked=True):
    """forward + backward through the C ABI under poison (module doc): {"y", "dx", "g<i>"}.  masks: CPU dict or {};
    tl / fl: lists or None; masked=False calls the parents (tl and fl must be None)."""
    lib, _ = m._ensure_created()
    B, S, T = tok.shape[0], tok.shape[1], x.shape[1]
    tensors = [t.detach().cpu() for t in m._tensors()]
    inputs = dict(tok=tok, x=x, dy=dy)
    inputs.update({f"p{i}": t for i, t in enumerate(tensors)})
    inputs.update({f"m{i}": t for i, t in enumerate(masks.values())})
    if tl is not None:
        inputs["tl"] = torch.tensor(tl, dtype=torch.int64)
    if fl is not None:
        inputs["fl"] = torch.tensor(fl, dtype=torch.int64)
    outs = {f"g{i}": tuple(t.shape) for i, t in enumerate(tensors)}
    outs.update(dx=(B, T, 12, 2), y=(B, T, 21, 2))
    nsaved, nws = lib.b2h_tpt_train_bytes(m._handle, B, S, T, 0), lib.b2h_tpt_train_bytes(m._handle, B, S, T, 1)

    def call(q):
        pa = (vp * len(tensors))(*[q[f"p{i}"] for i in range(len(tensors))])
        ma = (vp * len(masks))(*[q[f"m{i}"] for i in range(len(masks))]) if masks else None
        ga = (vp * len(tensors))(*[q[f"g{i}"] for i in range(len(tensors))])
        if not masked:
            rc = lib.b2h_tpt_train_forward(m._handle, pa, q["tok"], q["x"], ma, p, q["y"], q["saved"], nsaved, B, S, T, None)
            return rc or lib.b2h_tpt_backward(m._handle, pa, q["tok"], ma, p, q["dy"], q["saved"], nsaved, q["dx"], ga, q["ws"],
                                              nws, B, S, T, None)
        rc = lib.b2h_tpt_train_forward_masked(m._handle, pa, q["tok"], q["x"], ma, p, q["y"], q["saved"], nsaved, B, S, T,
                                              q.get("tl"), q.get("fl"), None)
        return rc or lib.b2h_tpt_backward_masked(m._handle, pa, q["tok"], ma, p, q["dy"], q["saved"], nsaved, q["dx"], ga,
                                                 q["ws"], nws, B, S, T, q.get("tl"), q.get("fl"), None)

    return poisoned_launch(call, inputs, outs, dev, scratch={"saved": nsaved, "ws": nws})


def _assert_equal_runs(a, b, keys, valid, what):
    """y at the valid frames, every parameter gradient and dx: the same bits."""
    assert torch.equal(a["y"][valid], b["y"][valid]), f"{what}: y differs at valid frames"
    assert torch.isfinite(a["y"]).all() and torch.isfinite(b["y"]).all()
    for i, k in enumerate(keys):
        assert torch.equal(a[f"g{i}"], b[f"g{i}"]), f"{what}: {k} differs by {float((a[f'g{i}'] - b[f'g{i}']).abs().max()):.3e}"
    assert torch.equal(a["dx"], b["dx"]), f"{what}: dx differs"


# ---- 1. token_lengths -------------------------------------------------------------------------------------------
def test_token_lengths(cuda_device):
    tok = torch.from_numpy(TOKEN_ROWS).to(cuda_device)
    for pad in (0, 7, -1):
        got = hps.token_lengths(tok, pad_id=pad)
        assert got.dtype == torch.int64 and got.device == tok.device and got.shape == (5,)
        assert got.cpu().tolist() == ref.token_lengths_ref(TOKEN_ROWS, pad).tolist()
    assert hps.token_lengths(tok).cpu().tolist() == [9, 1, 3, 2, 9]
    # more rows than one workgroup holds, rows longer than a wave, a row slice that is not its storage's start
    g = torch.Generator().manual_seed(1)
    big = torch.randint(0, 3, (11, 130), generator=g)
    big[3, 70:] = 0
    big[5] = 0
    big[6, 129] = 2
    assert hps.token_lengths(big.to(cuda_device)).cpu().tolist() == ref.token_lengths_ref(big.numpy()).tolist()
    assert hps.token_lengths(big.to(cuda_device)[1:]).cpu().tolist() == ref.token_lengths_ref(big.numpy()[1:]).tolist()
    assert hps.token_lengths(torch.zeros((0, 4), dtype=torch.int64, device=cuda_device)).shape == (0,)


def test_token_lengths_under_poison(cuda_device):
    lib = _lib.load()
    res = poisoned_launch(lambda q: lib.b2h_token_lengths(q["tok"], 5, 9, 0, q["len"], None), dict(tok=torch.from_numpy(TOKEN_ROWS)),
                          dict(len=(5, 2)), cuda_device)
    assert res["len"].view(torch.int64).reshape(-1).cpu().tolist() == [9, 1, 3, 2, 9]


# ---- 2. training parity against the float64 oracle ------------------------------------------------------------
def _check_against(got_y, got_g, got_dx, reference, keys, valid, what):
    y64, g64, dx64, err32, err32_dx = reference
    err = float((got_y.cpu().double() - y64)[valid].abs().max())
    print(f"\n{what}: max|y - y64| at valid frames {err:.3e}")
    assert torch.isfinite(got_y).all(), f"{what}: a padded row is not finite"
    assert err <= ref.BAR_Y, f"{what}: y {err:.3e}"
    for k, g, a, e in zip(keys, got_g, g64, err32):
        assert_within_bar(g.cpu().double().numpy(), a.numpy(), e, f"{what} {k}")
    assert_within_bar(got_dx.cpu().double().numpy(), dx64.numpy(), err32_dx, f"{what} dx")
    assert not got_dx.cpu()[~valid].any(), f"{what}: dx of a padded frame is not 0"


@pytest.mark.parametrize("name,route", PARITY, ids=lambda v: v)
def test_training_parity_p0(name, route, cuda_device):
    tok, x, dy, tl, fl = ref.case_data(name)
    m = _model(name, route, 0.0, cuda_device)
    xd = x.to(cuda_device).requires_grad_(True)
    y = m(tok.to(cuda_device), xd, text_lengths=torch.tensor(tl), frame_lengths=fl)     # a tensor and a sequence
    y.backward(dy.to(cuda_device))
    keys = param_keys(*ref.CASES[name][3])
    _check_against(y.detach(), [t.grad for t in m._tensors()], xd.grad, ref.case_reference(name), keys,
                   ref.valid_frames(fl, x.shape[1]), f"{name} {route} p=0")


@pytest.mark.parametrize("name,route", [("whole", "default"), ("whole", "whole_mfma"), ("blocked", "blocked_mfma"),
                                        ("blocked", "default"), ("deep", "all_mfma")], ids=lambda v: v)
def test_training_parity_with_dropout(name, route, cuda_device):
    p = 0.1
    tok, x, dy, tl, fl = ref.case_data(name)
    (B, S, T), _, _, (ne, nd) = ref.CASES[name]
    masks = cpu_masks(B, S, T, ne, nd, p, 9300)
    m = _model(name, route, p, cuda_device)
    xd = x.to(cuda_device).requires_grad_(True)
    y = m._forward_train(tok.to(cuda_device), xd, {k: v.to(cuda_device) for k, v in masks.items()}, tl, fl)
    y.backward(dy.to(cuda_device))
    _check_against(y.detach(), [t.grad for t in m._tensors()], xd.grad, ref.port_reference(name, masks, p), param_keys(ne, nd),
                   ref.valid_frames(fl, T), f"{name} {route} p={p}")


# ---- 3. the padding does not matter ------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", ["whole", "blocked", "deep"])
def test_padding_content_does_not_matter(name, route, cuda_device):
    p = 0.1 if name != "blocked" else 0.0
    tok, x, dy, tl, fl = ref.case_data(name)
    tok2, x2 = ref.repadded(name)
    (B, S, T), _, _, (ne, nd) = ref.CASES[name]
    masks = cpu_masks(B, S, T, ne, nd, p, 9301)
    m = _model(name, route, p, cuda_device)
    a = _abi_step(m, tok, x, dy, masks, p, tl, fl, cuda_device)
    b = _abi_step(m, tok2, x2, dy, masks, p, tl, fl, cuda_device)
    valid = ref.valid_frames(fl, T).to(cuda_device)
    _assert_equal_runs(a, b, param_keys(ne, nd), valid, f"{name} {route}")
    for r in (a, b):
        assert r["dx"][~valid].view(torch.int32).eq(0).all(), "dx of a padded frame: +0 bits, over the poison"
    # and it does matter without the lengths: the test's padding reaches the valid frames of the unmasked model
    c = _abi_step(m, tok2, x2, dy, masks, p, None, None, cuda_device)
    assert not torch.equal(c["y"][valid], b["y"][valid])


# ---- 4. full lengths equal no lengths ----------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", ["whole", "blocked"])
def test_full_lengths_equal_no_lengths_in_training(name, route, cuda_device):
    p = 0.1 if name == "whole" else 0.0
    tok, x, dy, _, _ = ref.case_data(name)
    (B, S, T), _, _, (ne, nd) = ref.CASES[name]
    masks = cpu_masks(B, S, T, ne, nd, p, 9302)
    m = _model(name, route, p, cuda_device)
    parent = _abi_step(m, tok, x, dy, masks, p, None, None, cuda_device, masked=False)
    everything = torch.ones((B, T), dtype=torch.bool, device=cuda_device)
    keys = param_keys(ne, nd)
    for tl, fl in (([S] * B, [T] * B), (None, None), ([S] * B, None), (None, [T] * B)):
        got = _abi_step(m, tok, x, dy, masks, p, tl, fl, cuda_device)
        _assert_equal_runs(got, parent, keys, everything, f"{name} {route} lengths {tl}, {fl}")


def _infer_model(name, dev):
    m = train_model(ref.case_state(name), 0.0, dev).eval()
    return m


def _infer_calls(m, tok, x, T, tl, fl):
    """{entry point: y} for the inference entry points that take T frames."""
    kw = {} if tl is None and fl is None else dict(text_lengths=tl, frame_lengths=fl)
    out = {"forward_long": m.forward_long(tok, x, **kw),
           "forward_fused": m.forward_fused(tok, x, dif_encoding=False, normalize=False, denormalize=False, **kw)}
    if T <= 128:
        out["forward"] = m(tok, x, **kw)
    return out


@pytest.mark.parametrize("name", ["whole", "blocked"])
def test_full_lengths_equal_no_lengths_in_inference(name, cuda_device):
    tok, x, _, _, _ = ref.case_data(name)
    (B, S, T) = ref.CASES[name][0]
    m = _infer_model(name, cuda_device)
    with torch.no_grad():
        plain = _infer_calls(m, tok, x, T, None, None)
        for tl, fl in (([S] * B, [T] * B), ([S] * B, None), (None, [T] * B)):
            for k, y in _infer_calls(m, tok, x, T, tl, fl).items():
                assert torch.equal(y, plain[k]), (k, tl, fl)


# ---- 5. clamp ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", ["whole", "blocked"])
def test_lengths_are_clamped(name, route, cuda_device):
    tok, x, dy, tl, fl = ref.case_data(name)
    (B, S, T), _, _, (ne, nd) = ref.CASES[name]
    m = _model(name, route, 0.0, cuda_device)
    # a 0 (and a negative length) behaves as 1, a length above the rows as the rows
    tl_a, fl_a = [S + 3, 0] + list(tl[2:]), [T + 3, -5] + list(fl[2:])
    tl_b, fl_b = [S, 1] + list(tl[2:]), [T, 1] + list(fl[2:])
    a = _abi_step(m, tok, x, dy, {}, 0.0, tl_a, fl_a, cuda_device)
    b = _abi_step(m, tok, x, dy, {}, 0.0, tl_b, fl_b, cuda_device)
    _assert_equal_runs(a, b, param_keys(ne, nd), torch.ones((B, T), dtype=torch.bool, device=cuda_device), f"{name} {route}")
    mi = _infer_model(name, cuda_device)
    with torch.no_grad():
        ya, yb = _infer_calls(mi, tok, x, T, tl_a, fl_a), _infer_calls(mi, tok, x, T, tl_b, fl_b)
    for k in ya:
        assert torch.equal(ya[k], yb[k]) and torch.isfinite(ya[k]).all(), k


# ---- 6. fp32 inference: parity, invariance, batch independence ---------------------------------------------------
@pytest.mark.parametrize("name", ["whole", "blocked"])
def test_inference_parity_and_invariance(name, cuda_device):
    tok, x, _, tl, fl = ref.case_data(name)
    tok2, x2 = ref.repadded(name)
    (B, S, T) = ref.CASES[name][0]
    y64 = ref.case_reference(name)[0]
    valid = ref.valid_frames(fl, T)
    m = _infer_model(name, cuda_device)
    with torch.no_grad():
        got, got2 = _infer_calls(m, tok, x, T, tl, fl), _infer_calls(m, tok2, x2, T, tl, fl)
        tail = m.forward_fused(tok, x, n_frames=fl, dif_encoding=False, normalize=False, denormalize=False, mask_tail=True,
                               text_lengths=tl, frame_lengths=torch.tensor(fl, device=cuda_device))
        unmasked = m.forward_long(tok2, x2)
    assert set(got) == ({"forward", "forward_long", "forward_fused"} if T <= 128 else {"forward_long", "forward_fused"})
    for k, y in got.items():
        err = float((y.cpu().double() - y64)[valid].abs().max())
        print(f"\n{name} {k}: max|y - y64| at valid frames {err:.3e}")
        assert torch.isfinite(y).all() and err <= ref.BAR_Y, (k, err)
        assert torch.equal(y, got["forward_long"])                      # one launch list behind the three
        assert torch.equal(y.cpu()[valid], got2[k].cpu()[valid]), f"{k}: the padding's content reached a valid frame"
    assert torch.equal(tail.cpu()[valid], got["forward_long"].cpu()[valid]) and not tail.cpu()[~valid].any()
    assert not torch.equal(unmasked.cpu()[valid], got2["forward_long"].cpu()[valid])
    # a sequence alone and inside the batch: the same bits
    with torch.no_grad():
        for b in range(B):
            alone = m.forward_long(tok[b:b + 1], x[b:b + 1], text_lengths=tl[b:b + 1], frame_lengths=fl[b:b + 1])
            assert torch.equal(alone[0], got["forward_long"][b]), b


def test_f16x3_refuses_lengths_on_the_device(cuda_device):
    tok, x, _, tl, fl = ref.case_data("whole")
    m = _infer_model("whole", cuda_device).set_precision("f16x3")
    with torch.no_grad():
        plain = m.forward_long(tok, x)                                  # f16x3 without lengths is what it was
        with pytest.raises(RuntimeError, match=r"b2h_tpt_set_kernel\(fp32\)"):
            m.forward_long(tok, x, text_lengths=tl)
        assert torch.equal(m.forward_long(tok, x), plain)
    # the C ABI's own refusal
    lib, dev = m._ensure_handle()
    assert lib.b2h_tpt_set_kernel(m._handle, TENC_KERNELS["f16x3"]) == _lib.OK
    B, S, T = 3, 9, 17
    need = lib.b2h_tpt_workspace_bytes(m._handle, B, S, T)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    t, xx, y = tok.to(dev), x.to(dev), torch.empty((B, T, 21, 2), device=dev)
    ln = torch.tensor(tl, device=dev)
    args = (m._handle, vp(t.data_ptr()), vp(xx.data_ptr()), vp(y.data_ptr()), B, S, T, 0, 1.0, None)
    assert lib.b2h_tpt_forward_masked(*args, vp(ln.data_ptr()), None, vp(ws.data_ptr()), need, None) == _lib.ERR_UNSUPPORTED
    assert "b2h_tpt_set_kernel(fp32)" in _lib.last_error()
    assert lib.b2h_tpt_forward_masked(*args, None, None, vp(ws.data_ptr()), need, None) == _lib.OK
    torch.cuda.synchronize(dev)
    assert torch.equal(y, plain)


# ---- 8. the C ABI: alignment and overlap of the length arrays ---------------------------------------------------
def test_masked_entry_points_refuse_misaligned_and_overlapping_lengths(cuda_device):
    name = "whole"
    tok, x, dy, tl, fl = ref.case_data(name)
    (B, S, T), _, _, (ne, nd) = ref.CASES[name]
    m = _model(name, "default", 0.0, cuda_device)
    lib, dev = m._ensure_handle()
    tensors = list(m._tensors())
    grads = [torch.empty_like(t) for t in tensors]
    pa, ga = (vp * len(tensors))(*[t.data_ptr() for t in tensors]), (vp * len(grads))(*[t.data_ptr() for t in grads])
    t, xx, dyd = tok.to(dev), x.to(dev), dy.to(dev)
    y, dx = torch.empty((B, T, 21, 2), device=dev), torch.empty((B, T, 12, 2), device=dev)
    nsaved, nws = lib.b2h_tpt_train_bytes(m._handle, B, S, T, 0), lib.b2h_tpt_train_bytes(m._handle, B, S, T, 1)
    saved, ws = torch.empty(nsaved, dtype=torch.uint8, device=dev), torch.empty(nws, dtype=torch.uint8, device=dev)
    lens = torch.tensor([tl + [0], fl + [0]], dtype=torch.int64, device=dev)          # room for a pointer 4 bytes in
    good_t, good_f = lens[0].data_ptr(), lens[1].data_ptr()

    def fwd(a, b):
        return lib.b2h_tpt_train_forward_masked(m._handle, pa, vp(t.data_ptr()), vp(xx.data_ptr()), None, 0.0, vp(y.data_ptr()),
                                                vp(saved.data_ptr()), nsaved, B, S, T, a, b, None)

    def bwd(a, b):
        return lib.b2h_tpt_backward_masked(m._handle, pa, vp(t.data_ptr()), None, 0.0, vp(dyd.data_ptr()), vp(saved.data_ptr()),
                                           nsaved, vp(dx.data_ptr()), ga, vp(ws.data_ptr()), nws, B, S, T, a, b, None)

    inf_need = lib.b2h_tpt_workspace_bytes(m._handle, B, S, T)
    iws = torch.empty(inf_need, dtype=torch.uint8, device=dev)

    def inf(a, b):
        return lib.b2h_tpt_forward_masked(m._handle, vp(t.data_ptr()), vp(xx.data_ptr()), vp(y.data_ptr()), B, S, T, 0, 1.0, None,
                                          a, b, vp(iws.data_ptr()), inf_need, None)

    for call in (fwd, bwd, inf):
        for a, b in ((vp(good_t + 4), vp(good_f)), (vp(good_t), vp(good_f + 4)), (None, vp(good_f + 4)), (vp(good_t + 4), None)):
            assert call(a, b) == _lib.ERR_INVALID and "8-byte aligned" in _lib.last_error(), call.__name__
    # a length array inside an output
    for call, out in ((fwd, y), (fwd, saved), (bwd, dx), (bwd, ws), (bwd, grads[0]), (inf, y), (inf, iws)):
        inside = vp(out.data_ptr() + 8)
        for a, b in ((inside, vp(good_f)), (vp(good_t), inside)):
            assert call(a, b) == _lib.ERR_INVALID and "overlap" in _lib.last_error(), (call.__name__, _lib.last_error())
    # well-formed calls, masked and not, still run
    assert fwd(vp(good_t), vp(good_f)) == _lib.OK and bwd(vp(good_t), vp(good_f)) == _lib.OK
    assert inf(vp(good_t), vp(good_f)) == _lib.OK
    assert lib.b2h_tpt_train_forward(m._handle, pa, vp(t.data_ptr()), vp(xx.data_ptr()), None, 0.0, vp(y.data_ptr()),
                                     vp(saved.data_ptr()), nsaved, B, S, T, None) == _lib.OK
    assert lib.b2h_tpt_backward(m._handle, pa, vp(t.data_ptr()), None, 0.0, vp(dyd.data_ptr()), vp(saved.data_ptr()), nsaved,
                                vp(dx.data_ptr()), ga, vp(ws.data_ptr()), nws, B, S, T, None) == _lib.OK
    assert lib.b2h_tpt_forward_fused(m._handle, vp(t.data_ptr()), vp(xx.data_ptr()), vp(y.data_ptr()), B, S, T, 0, 1.0, None,
                                     vp(iws.data_ptr()), inf_need, None) == _lib.OK
    torch.cuda.synchronize(dev)
