"""The native dropout masks on the MI355X: b2h_dropout_masks (kernel_dropout_masks.h) bit for bit against the numpy
restatement of its generator (philox_ref.py), between guard bytes and over poison; `set_dropout_source("native")` on
both transformers -- order, shapes, one allocation, steps, torch's generator untouched, keep rates; gradients with the
kernel's own masks against float64 autograd of the ports at the bars of test_tpt_train_long_gpu.py and
test_tenc_train_gpu.py; reproducibility from (seed, step); a captured step that draws new masks on every replay."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
import philox_ref
import tenc_train_ref
import test_tpt_train_long_gpu as long_gpu
from hand_pose_sl_amd import _lib
from tpt_train_ref import assert_within_bar, mask_shapes, param_keys, recipe_state, train_model

pytestmark = pytest.mark.gpu
N_TOKENS = 50
GUARD = 32
# kDmThreads * kDmMaxBlocks of kernel_dropout_masks.h: a call with more 16-byte chunks than this strides over them
GRID_THREADS = 256 * 1024
SIZES = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 392, 4099, 2 ** 20 + 5]


def _draw(dev, sizes, p, seed, step, first=0, step_word=None):
    """One b2h_dropout_masks call into buffers pre-filled with 0xFF between 32 guard bytes of 0xA5 on either side; checks
    that every guard byte survived and every mask byte is 0 or 1, and returns the masks (numpy, uint8)."""
    offsets, total = [], 0
    for n in sizes:
        offsets.append(total + GUARD)                       # GUARD and every start are multiples of 16
        total += (GUARD + n + GUARD + 15) // 16 * 16
    host = np.full(max(total, 16), 0xA5, np.uint8)
    for o, n in zip(offsets, sizes):
        host[o:o + n] = 0xFF
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    word = None if step_word is None else torch.tensor([step_word], dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.load().b2h_dropout_masks((ctypes.c_void_p * len(sizes))(*[buf.data_ptr() + o for o in offsets]),
                                             (ctypes.c_int64 * len(sizes))(*sizes), len(sizes), first, p, seed, step,
                                             None if word is None else ctypes.c_void_p(word.data_ptr()), ctypes.c_void_p(st)))
    got = buf.cpu().numpy()
    if word is not None:
        assert int(word.item()) == step_word                # read, never written
    out, keep = [], np.ones(got.shape, bool)
    for o, n in zip(offsets, sizes):
        out.append(got[o:o + n].copy())
        keep[o:o + n] = False
    assert (got[keep] == 0xA5).all(), "a guard byte was written"
    for i, m in enumerate(out):
        assert m.size == 0 or int(m.max()) <= 1, f"mask {i}: a byte is neither 0 nor 1 (0xFF = never written)"
    return out


@functools.lru_cache(maxsize=None)
def _words(seed, step):
    """The restatement's words for SIZES, masks numbered from 0 (shared: leave unchanged)."""
    return [philox_ref.words(n, i, step, seed) for i, n in enumerate(SIZES)]


# ---- 1. bits against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0, 2 ** 32 - 1])
@pytest.mark.parametrize("seed", [3, 2 ** 40 + 5])
@pytest.mark.parametrize("p", [0.1, 0.5, 1 / 3, 2.0 ** -30], ids=["0.1", "0.5", "third", "2^-30"])
def test_bits_equal_the_restatement(p, seed, step, cuda_device):
    thr = np.uint64(philox_ref.threshold(p))
    got = _draw(cuda_device, SIZES, p, seed, step)
    for i, (g, w) in enumerate(zip(got, _words(seed, step))):
        assert np.array_equal(g, (w >= thr).astype(np.uint8)), f"mask {i} of {SIZES[i]} elements"


def test_pinned_vectors_on_the_device(cuda_device):
    assert _draw(cuda_device, [20], 0.5, 3, 5, first=2)[0].tolist() == [1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0]
    assert _draw(cuda_device, [20], 0.1, 3, 5, first=2)[0].tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1]


def test_step_word_first_index_and_more_than_64_masks(cuda_device):
    sizes = SIZES[:12]
    ref = _draw(cuda_device, sizes, 0.5, 3, 5)
    for a, b in zip(ref, philox_ref.masks(sizes, 5, 3, 0.5)):
        assert np.array_equal(a, b)
    for step, word in ((2, 3), (0, 5), (2 ** 32 + 5, 0), (2 ** 32 - 1, 6)):        # s = (step + word) mod 2^32
        for a, b in zip(ref, _draw(cuda_device, sizes, 0.5, 3, step, step_word=word)):
            assert np.array_equal(a, b), (step, word)
    assert not np.array_equal(ref[11], _draw(cuda_device, sizes, 0.5, 3, 2, step_word=4)[11])
    for a, b in zip(ref[7:], _draw(cuda_device, sizes[7:], 0.5, 3, 5, first=7)):    # mask i has number first_index + i
        assert np.array_equal(a, b)
    # one mask alone, and behind others of other sizes: an element depends on its own (number, index) only
    assert np.array_equal(_draw(cuda_device, [4099], 0.5, 3, 5, first=11)[0], ref[11])
    assert np.array_equal(_draw(cuda_device, [2 ** 20 + 5, 0, 77, 4099], 0.5, 3, 5, first=8)[3], ref[11])
    # 70 masks: two launches (64 + 6); empty masks among them
    many = [(37 * i) % 53 for i in range(70)]
    assert many.count(0) == 2 and many[0] == 0
    for i, (a, b) in enumerate(zip(_draw(cuda_device, many, 1 / 3, 2 ** 40 + 5, 9), philox_ref.masks(many, 9, 2 ** 40 + 5, 1 / 3))):
        assert np.array_equal(a, b), i
    for i, (a, b) in enumerate(zip(_draw(cuda_device, many[60:], 1 / 3, 2 ** 40 + 5, 9, first=60),
                                   philox_ref.masks(many, 9, 2 ** 40 + 5, 1 / 3)[60:])):
        assert np.array_equal(a, b), i


def test_more_chunks_than_the_grid_has_threads(cuda_device):
    """The issue's 2^20 + 5 bytes are 65 537 chunks, fewer than this kernel's largest grid (262 144 threads), so this
    case adds a call of 2.5 grids of chunks: every thread walks its stride, the last pass is partial, and a mask
    boundary falls inside a pass."""
    sizes = [16 * GRID_THREADS + 21, 5, 16 * GRID_THREADS * 3 // 2 - 7]
    for a, b in zip(_draw(cuda_device, sizes, 0.5, 3, 1), philox_ref.masks(sizes, 1, 3, 0.5)):
        assert np.array_equal(a, b)


# ---- 2. poison and guards (every _draw checks them) --------------------------------------------------------------
def test_p1_drops_everything_and_p0_keeps_everything(cuda_device):
    for m in _draw(cuda_device, SIZES, 1.0, 3, 0):
        assert not m.any()
    for m in _draw(cuda_device, SIZES, 0.0, 3, 0):
        assert m.all()
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))       # thr = 2^32 - 256: 6e-8 of the words survive
    for m, w in zip(_draw(cuda_device, SIZES, below_one, 3, 0), _words(3, 0)):
        assert np.array_equal(m, (w >= np.uint64(2 ** 32 - 256)).astype(np.uint8))


# ---- 3. TextPoseTransformer: order, shapes, one allocation, steps, keep rates -----------------------------------
def _numel_tpt(m, B, S, T, capacity=64):
    m._ensure_created()
    out = (ctypes.c_int64 * max(capacity, 1))(*[-1] * max(capacity, 1))
    n = _lib.load().b2h_tpt_mask_numel(m._handle, B, S, T, out, capacity)
    return n, list(out)[:capacity]


def _check_views(masks, order, seed, step, p):
    assert [(k, tuple(v.shape)) for k, v in masks.items()] == order
    storages = {v.untyped_storage().data_ptr() for v in masks.values()}
    assert len(storages) == 1                               # one allocation
    for i, (k, v) in enumerate(masks.items()):
        assert v.dtype == torch.uint8 and v.is_contiguous() and v.data_ptr() % 16 == 0 and v.device.type == "cuda", k
        assert np.array_equal(v.cpu().numpy().reshape(-1), philox_ref.mask(v.numel(), i, step, seed, p)), (k, step)
        if v.numel() >= 300:                                # the bound of test_mask_keep_rates
            sigma = (p * (1 - p) / v.numel()) ** 0.5
            assert abs(float(v.float().mean()) - (1 - p)) <= 5 * sigma, (k, step)


@pytest.mark.parametrize("shape", [(2, 7, 15), (3, 9, 21), (1, 17, 129)], ids=lambda s: "b%d_s%d_t%d" % s)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("layers", [(1, 1), (2, 3)], ids=lambda l: "e%d_d%d" % l)
def test_text_pose_transformer_draws(layers, p, shape, cuda_device):
    m = train_model(recipe_state(40, N_TOKENS, *layers), p, cuda_device)
    assert m.dropout_source == "torch"
    assert m.set_dropout_source("native", seed=3) is m
    order = mask_shapes(*shape, *layers)
    torch.manual_seed(77)
    before = torch.cuda.get_rng_state(cuda_device)
    first = m._draw_dropout_masks(*shape)
    second = m._draw_dropout_masks(*shape)
    assert torch.equal(torch.cuda.get_rng_state(cuda_device), before) and torch.initial_seed() == 77
    _check_views(first, order, 3, 0, p)
    _check_views(second, order, 3, 1, p)
    assert m._drop_step.dtype == torch.int64 and m._drop_step.device.type == "cuda" and m._drop_step.tolist() == [2]
    m.set_dropout_source("native", seed=3)                  # again: the count restarts
    _check_views(m._draw_dropout_masks(*shape), order, 3, 0, p)
    count, numel = _numel_tpt(m, *shape)
    assert count == len(order) == 4 * layers[0] + 6 * layers[1] and numel[:count] == [math.prod(s) for _, s in order]
    assert numel[count:] == [-1] * (64 - count)
    assert _numel_tpt(m, *shape, capacity=3) == (count, numel[:3])     # min(count, capacity) written, the count returned
    assert _numel_tpt(m, shape[0], 129, shape[2])[0] == 0 and _numel_tpt(m, shape[0], shape[1], 1025)[0] == 0
    assert _numel_tpt(m, -1, shape[1], shape[2])[0] == 0 and _numel_tpt(m, shape[0], 0, shape[2])[0] == 0
    p0 = train_model(recipe_state(40, N_TOKENS, *layers), 0.0, cuda_device).set_dropout_source("native", seed=3)
    assert p0._draw_dropout_masks(*shape) == {}             # p == 0: no masks, as under "torch"


# ---- 4. gradients against float64 autograd of the port, with the masks the kernel drew ---------------------------
# The data seeds were chosen on the CPU alone: the masks are those of the restatement (mask seed 3, step 0), and the
# first seed of the rule of test_tpt_train_long_gpu._check_case (7000 + T) keeps its ReLU margin in both cases:
#   (2, 3) layers, p 0.1, (2, 7, 15):   nearest ReLU input 1.15e-4, fp32 rounding 2.6e-6
#   (1, 1) layers, p 0.5, (1, 17, 129): nearest ReLU input 1.14e-4, fp32 rounding 2.1e-6
GRAD_CASES = [((2, 3), 0.1, (2, 7, 15), "valu"), ((1, 1), 0.5, (1, 17, 129), "valu"), ((1, 1), 0.5, (1, 17, 129), "mfma")]


@pytest.mark.parametrize("layers,p,shape,route", GRAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gradients_with_native_masks_against_float64_autograd(layers, p, shape, route, cuda_device):
    dev = cuda_device
    state = recipe_state(100 + 10 * layers[0] + layers[1], N_TOKENS, *layers)
    m = train_model(state, p, dev).set_train_kernels(route).set_dropout_source("native", seed=3)
    tok, x, dy = long_gpu._data(*shape, N_TOKENS, 7000 + shape[2], 1.0)
    masks = m._draw_dropout_masks(*shape)
    cm = {k: v.cpu() for k, v in masks.items()}             # read back: the masks the kernel drew
    for i, (k, s) in enumerate(mask_shapes(*shape, *layers)):
        assert np.array_equal(cm[k].numpy().reshape(-1), philox_ref.mask(math.prod(s), i, 0, 3, p)), k
    (y64, g64, dx64), pre64 = long_gpu._port_grads_and_relu_inputs(tok, x, state, cm, p, dy, torch.float64)
    (y32, g32, dx32), pre32 = long_gpu._port_grads_and_relu_inputs(tok, x, state, cm, p, dy, torch.float32)
    nearest, rounding = float(pre64.abs().min()), float((pre32 - pre64).abs().max())
    assert nearest >= long_gpu.RELU_MARGIN * rounding, (nearest, rounding)      # holds on the CPU ports, see above
    xd = x.to(dev).requires_grad_(True)
    y = m._forward_train(tok.to(dev), xd, masks)
    y.backward(dy.to(dev))
    what = f"L={layers} p={p} shape={shape} {route}"
    err_y, tol_y = float((y.detach().cpu().double() - y64).abs().max()), long_gpu._tol_y(y64)
    print(f"\n{what}: y error {err_y:.3e} (bar {tol_y:.3e})")
    assert err_y <= tol_y, what
    got = [q.grad.detach().cpu().double().numpy() for q in m._tensors()] + [xd.grad.cpu().double().numpy()]
    worst = (0.0, "")
    for k, g, a, b in zip(param_keys(*layers) + ["dx"], got, g64 + [dx64], g32 + [dx32]):
        err32 = float((b.double() - a).abs().max())
        if err32 > 0:
            worst = max(worst, (float(np.abs(g - a.numpy()).max() / err32), k))
    print(f"{what}: worst ratio {worst[0]:.3f} ({worst[1]})")
    for k, g, a, b in zip(param_keys(*layers) + ["dx"], got, g64 + [dx64], g32 + [dx32]):
        assert_within_bar(g, a.numpy(), float((b.double() - a).abs().max()), f"{what} {k}")


# ---- 5. reproducibility ------------------------------------------------------------------------------------------
def _two_steps(seed, dev, tok, x, dy):
    m = train_model(recipe_state(40, N_TOKENS, 2, 2), 0.1, dev).set_dropout_source("native", seed=seed)
    return [long_gpu._step(m, tok, x, dy) for _ in range(2)]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(g, h) for g, h in zip(a[1], b[1]))


def test_reproducible_from_seed_and_step(cuda_device):
    B, S, T = 3, 11, 37
    tok, x, dy = (t.to(cuda_device) for t in long_gpu._data(B, S, T, N_TOKENS, 41))
    torch.manual_seed(1)
    a = _two_steps(11, cuda_device, tok, x, dy)
    torch.manual_seed(2)                                    # torch's seed plays no part
    b = _two_steps(11, cuda_device, tok, x, dy)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    assert not torch.equal(a[0][0], a[1][0]) and not torch.equal(a[0][2], a[1][2])      # step 2 differs from step 1
    c = _two_steps(12, cuda_device, tok, x, dy)
    assert not torch.equal(a[0][0], c[0][0]) and not torch.equal(a[1][0], c[1][0])      # another seed differs
    # no seed given: torch.initial_seed()
    torch.manual_seed(11)
    m = train_model(recipe_state(40, N_TOKENS, 2, 2), 0.1, cuda_device).set_dropout_source("native")
    assert _same(long_gpu._step(m, tok, x, dy), a[0])


def test_default_source_is_torch_and_unchanged(cuda_device):
    B, S, T, p = 2, 7, 15, 0.1
    m = train_model(recipe_state(40, N_TOKENS, 1, 1), p, cuda_device)
    assert m.dropout_source == "torch" and m._drop_step is None
    torch.manual_seed(7)
    masks = m._draw_dropout_masks(B, S, T)
    torch.manual_seed(7)
    for (k, shape), (key, v) in zip(mask_shapes(B, S, T, 1, 1), masks.items()):
        assert k == key and torch.equal(v, (torch.rand(shape, device=cuda_device) >= p).to(torch.uint8))
    back = train_model(recipe_state(40, N_TOKENS, 1, 1), p, cuda_device).set_dropout_source("native", seed=3)
    torch.manual_seed(7)
    again = back.set_dropout_source("torch")._draw_dropout_masks(B, S, T)               # switched back: torch's draw
    assert all(torch.equal(masks[k], again[k]) for k in masks)


# ---- 6. a captured step draws new masks on every replay ----------------------------------------------------------
def test_captured_step_redraws_on_every_replay(cuda_device):
    B, S, T = 2, 7, 15
    state = recipe_state(90, N_TOKENS, 2, 2)
    m = train_model(state, 0.1, cuda_device).set_dropout_source("native", seed=5)
    tok, x, dy = (t.to(cuda_device) for t in long_gpu._data(B, S, T, N_TOKENS, 91))
    xs = x.clone().requires_grad_(True)
    s = torch.cuda.Stream(cuda_device)                      # warm-up on a side stream, as torch's docs do: draw 0
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        m(tok, xs).backward(dy)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    assert m._drop_step.tolist() == [1]
    graph = torch.cuda.CUDAGraph()
    for q in m.parameters():
        q.grad = None
    xs.grad = None
    with torch.cuda.graph(graph):                           # one stream: no parallel branches; the draw is inside
        m(tok, xs).backward(dy)
    assert m._drop_step.tolist() == [1]                     # capturing ran nothing
    replays = []
    for _ in range(2):
        for q in m.parameters():
            q.grad.fill_(float("nan"))
        xs.grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        replays.append(([q.grad.clone() for q in m._tensors()], xs.grad.clone()))
    assert m._drop_step.tolist() == [3]                     # one warm-up draw and two replays
    twin = train_model(state, 0.1, cuda_device).set_dropout_source("native", seed=5)
    twin._draw_dropout_masks(B, S, T)                       # the warm-up's step 0
    for grads, dx in replays:                               # steps 1 and 2
        _, eager_g, eager_dx = long_gpu._step(twin, tok, x, dy)
        assert torch.equal(eager_dx, dx) and all(torch.equal(a, b) for a, b in zip(eager_g, grads))
    assert twin._drop_step.tolist() == [3]
    assert not torch.equal(replays[0][1], replays[1][1])
    assert any(not torch.equal(a, b) for a, b in zip(replays[0][0], replays[1][0]))


# ---- 7. TransformerEnc -------------------------------------------------------------------------------------------
def test_transformer_enc_draws_and_gradients(cuda_device):
    dev, B, T, nlayers, p = cuda_device, 2, 9, 2, 0.1
    state = tenc_train_ref.seeded_state(nlayers, 31)
    m = hps.TransformerEnc(24, 4, 128, 42, nlayers, dropout=p)
    m.load_state_dict(state)
    m = m.to(dev).train()
    assert m.dropout_source == "torch" and m.set_dropout_source("native", seed=2 ** 40 + 5) is m
    order = [("pos", (B, T, 24))]
    for l in range(nlayers):
        order += [((l, n), (B, 4, T, T) if n == "attn" else (B, T, 128)) for n in tenc_train_ref.NAMES]
    before = torch.cuda.get_rng_state(dev)
    masks = m._draw_dropout_masks(B, T)
    _check_views(masks, order, 2 ** 40 + 5, 0, p)
    _check_views(m._draw_dropout_masks(B, T), order, 2 ** 40 + 5, 1, p)
    assert torch.equal(torch.cuda.get_rng_state(dev), before) and m._drop_step.tolist() == [2]
    m._ensure_created()
    out = (ctypes.c_int64 * 16)(*[-1] * 16)
    lib = _lib.load()
    assert lib.b2h_tenc_mask_numel(m._handle, B, T, out, 16) == 1 + 4 * nlayers == len(order)
    assert list(out) == [math.prod(s) for _, s in order] + [-1] * (16 - len(order))
    assert lib.b2h_tenc_mask_numel(m._handle, B, T, out, 2) == len(order)
    assert lib.b2h_tenc_mask_numel(m._handle, B, 101, out, 16) == 0 and lib.b2h_tenc_mask_numel(m._handle, B, 0, out, 16) == 0
    # one float64 parity case, as test_tenc_train_gpu._check_case, with the masks of the first draw
    g = torch.Generator().manual_seed(3100)
    x, dy = torch.randn((B, T, 12, 2), generator=g), torch.randn((B, T, 21, 2), generator=g)
    xd = x.to(dev).requires_grad_(True)
    y = m._forward_train(xd, masks)
    y.backward(dy.to(dev))
    cm = {k: v.cpu() for k, v in masks.items()}
    y64, g64, dx64 = tenc_train_ref.port_grads(x, state, cm, p, dy, torch.float64)
    _, g32, dx32 = tenc_train_ref.port_grads(x, state, cm, p, dy, torch.float32)
    assert float((y.detach().cpu().double() - y64).abs().max()) <= 2e-5 * max(1.0, float(y64.abs().max()))
    got = [q.grad.detach().cpu().double().numpy() for q in m._tensors()[1:]] + [xd.grad.cpu().double().numpy()]
    for k, gg, a, b in zip(tenc_train_ref.param_keys(nlayers) + ["dx"], got, g64 + [dx64], g32 + [dx32]):
        assert_within_bar(gg, a.numpy(), float((b.double() - a).abs().max()), f"tenc {k}")
    # the whole step through model(x): two models, one seed, the same bits; the next step differs
    a, b = (hps.TransformerEnc(24, 4, 128, 42, nlayers, dropout=p) for _ in range(2))
    ys = []
    for mm in (a, b):
        mm.load_state_dict(state)
        mm.to(dev).train().set_dropout_source("native", seed=11)
        ys.append([mm(x.to(dev)).detach().clone() for _ in range(2)])
    assert torch.equal(ys[0][0], ys[1][0]) and torch.equal(ys[0][1], ys[1][1]) and not torch.equal(ys[0][0], ys[0][1])
