"""Every entry point of the C ABI at the weakest pointer alignment include/b2h.h promises for each argument (the
table in DESIGN.md, "Pointer alignment"), and the Python surface on parameters and inputs that start off the 16-byte
grid.

Criterion: the same call twice through tests/poison.py -- once with every operand on the 16-byte grid, once with every
weakly promised pointer at its weakest alignment (tensor i of a pointer array 4 * (1 + i % 3) bytes past the grid where
the promise is 4 bytes, 8 bytes where it is 8) -- must give the same bits in every output.  That needs no tolerance: in
none of these kernels does the order of a sum depend on an address; alignment only selects how words reach LDS or
registers.  poison.launch adds quiet NaNs right before and after every shifted operand, intact guards, every output word
written and inputs unmodified.  The aligned side is not its own witness: it is held to the float64 ports with the bars
the other test files use (train_ref.assert_within_bar: 4 * max|g32 - g64| + 1e-6 * max|g64|; 2e-5 on y; tpt_ref.BAR)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import batch_ref
import hand_pose_sl_amd as hps
import oracle
import poison
import tenc_train_ref as TE
import tpt_geom_ref as G
import train_ref
from hand_pose_sl_amd import _lib
from test_tpt_geom_gpu import _numpy_item, _ws_bytes, combo_models
from tpt_train_ref import cpu_masks, tokens_with_padding
from tpt_train_ref import param_keys as tpt_param_keys
from train_ref import assert_within_bar

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
TOL_Y = 2e-5                                  # the fp32 bar on y of test_tenc_train_gpu.py / test_train_gpu.py
FACTOR = 1280.0
POST = _lib.POST_DENORMALIZE | _lib.POST_MASK_TAIL
ALL_FLAGS = _lib.PRE_CHEST_DIFF | _lib.PRE_NORMALIZE | POST


# ---- the two runs ------------------------------------------------------------------------------------------------
def weak4(names, start=0):
    """Tensor i of a pointer array promised 4-byte aligned: 4, 8, 12, 4, ... bytes past the 16-byte grid."""
    return {n: 4 * (1 + (start + i) % 3) for i, n in enumerate(names)}


def bits(t):
    return t.contiguous().view(torch.int32)


def both(call, inputs, outputs, dev, shift_sets, scratch=None):
    """The call on the grid and once per {name: bytes} of `shift_sets`; every output bit-equal; the aligned outputs.
    Also checks that the harness put every pointer where it was asked to."""
    def placed(shifts):
        def run(p):
            for k in list(inputs) + list(outputs):
                assert p[k].value % 16 == shifts.get(k, 0), (k, p[k].value % 16)
            return call(p)
        return run
    aligned = poison.launch(placed({}), inputs, outputs, dev, scratch=scratch)
    for shifts in shift_sets:
        assert shifts and any(shifts.values())
        moved = poison.launch(placed(shifts), inputs, outputs, dev, scratch=scratch, shifts=shifts)
        for k in outputs:
            assert torch.equal(bits(aligned[k]), bits(moved[k])), (k, shifts.get(k, 0))
    return aligned


def all_residues(shifts, names):
    return {shifts[n] for n in names} == {4, 8, 12}


def test_harness_shifts_the_operand_not_the_bands(cuda_device):
    for shift in (0, 4, 8, 12):
        g = poison.Guarded(40, poison.QNAN, 0, cuda_device, shift)
        assert g.words.data_ptr() % 256 == 0 and g.ptr.value == g.words.data_ptr() + poison.GUARD + shift
        assert g.body.numel() == 10 and not g.body.any() and g.guards_intact()
        assert g.words.numel() == (2 * poison.GUARD + shift + 40) // 4
        g.words[g.lo - 1] = 0                      # the word right before the operand belongs to the lower band
        assert not g.guards_intact()
        g.words[g.lo - 1] = g.fill
        g.words[g.hi] = 0                          # the word right after its last word to the upper band
        assert not g.guards_intact()
    with pytest.raises(AssertionError):
        poison.Guarded(40, 0, 0, cuda_device, 2)
    t = torch.arange(42, dtype=torch.float32).view(1, 1, 21, 2)
    got, lib = {}, _lib.load()

    def call(p):                                   # b2h_target_transform without flags: hand_out = hand
        got.update({k: p[k].value % 16 for k in ("a", "body", "y")})
        return lib.b2h_target_transform(p["body"], p["a"], p["y"], 1, 1, 0, 1.0, None)
    ins = {"a": t, "body": torch.zeros((1, 1, 12, 2))}
    out = poison.launch(call, ins, {"y": (1, 1, 21, 2)}, cuda_device, shifts={"a": 4, "y": 12})
    assert got == {"a": 4, "body": 0, "y": 12} and torch.equal(out["y"].cpu(), t)
    with pytest.raises(AssertionError):
        poison.launch(call, ins, {"y": (1, 1, 21, 2)}, cuda_device, shifts={"b": 4})


# ---- TransformerEnc training ---------------------------------------------------------------------------------------
def _noisy(state, seed, skip=()):
    """`state` with seeded noise on every tensor, so that LayerNorm gains and biases and the attention biases are not
    their defaults (a kernel that dropped one would pass on gamma = 1, beta = 0)."""
    g = torch.Generator().manual_seed(seed)
    return {k: (v.clone() if k in skip else v + 0.05 * torch.randn(v.shape, generator=g)) for k, v in state.items()}


@pytest.mark.parametrize("route", ["valu", "mfma"])
@pytest.mark.parametrize("B,T", [(3, 17), (2, 100)])
def test_tenc_training_params_and_grads_off_the_grid(B, T, route, cuda_device):
    """b2h_tenc_train_forward + b2h_tenc_backward, 2 layers, p = 0.1: pe, every weight, bias, gamma and beta and all 28
    gradients at +4 / +8 / +12.  On the mfma route every ml_stage_w call takes its dword path (K = 24 and 128)."""
    L, p = 2, 0.1
    state = _noisy(TE.seeded_state(L, 60), 61, skip=("pos_encoder.pe",))
    m = hps.TransformerEnc(24, 4, 128, 42, L, dropout=p)
    m.load_state_dict(state)
    m = m.to(cuda_device).train()
    lib, _ = m._ensure_created()
    assert lib.b2h_tenc_set_train_kernel(m._handle, _lib.TRAIN_KERNELS[route]) == _lib.OK
    assert lib.b2h_tenc_set_train_linear(m._handle, _lib.TRAIN_KERNELS[route]) == _lib.OK
    assert lib.b2h_tenc_train_linear_name(m._handle).decode() == {"valu": "b2h_tt_linear", "mfma": "b2h_ml_linear"}[route]
    assert lib.b2h_tenc_train_attn_name(m._handle, T).decode() == {"valu": "b2h_tt_sdpa", "mfma": "b2h_mw_sdpa"}[route]
    g = torch.Generator().manual_seed(62)
    x = torch.randn((B, T, 12, 2), generator=g)
    dy = torch.randn((B, T, 21, 2), generator=g)
    masks = {"pos": (torch.rand((B, T, 24), generator=g) >= p).to(torch.uint8)}
    for l in range(L):
        masks[(l, "attn")] = (torch.rand((B, 4, T, T), generator=g) >= p).to(torch.uint8)
        for n in TE.NAMES[1:]:
            masks[(l, n)] = (torch.rand((B, T, 128), generator=g) >= p).to(torch.uint8)
    tensors = [t.detach().cpu() for t in m._tensors()]
    np_, ng = len(tensors), len(tensors) - 1
    assert ng == 28
    inputs = dict(x=x, dy=dy)
    inputs.update({f"p{i}": t for i, t in enumerate(tensors)})
    inputs.update({f"m{i}": t for i, t in enumerate(masks.values())})
    outs = {f"g{i}": tuple(t.shape) for i, t in enumerate(tensors[1:])}
    outs["dx"], outs["y"] = (B, T, 12, 2), (B, T, 21, 2)
    shifts = weak4([f"p{i}" for i in range(np_)])
    shifts.update(weak4([f"g{i}" for i in range(ng)], start=1))
    assert shifts["p0"] == 4                                                     # pe
    assert all_residues(shifts, [f"p{i}" for i, t in enumerate(tensors) if i and t.dim() == 2])      # weights
    assert all_residues(shifts, [f"p{i}" for i, t in enumerate(tensors) if t.dim() == 1])            # biases, gamma, beta
    assert all_residues(shifts, [f"g{i}" for i in range(ng)])
    nsaved, nws = lib.b2h_tenc_train_bytes(m._handle, B, T, 0), lib.b2h_tenc_train_bytes(m._handle, B, T, 1)

    def call(q):
        pa = (vp * np_)(*[q[f"p{i}"] for i in range(np_)])
        ma = (vp * len(masks))(*[q[f"m{i}"] for i in range(len(masks))])
        ga = (vp * ng)(*[q[f"g{i}"] for i in range(ng)])
        rc = lib.b2h_tenc_train_forward(m._handle, pa, q["x"], ma, p, q["y"], q["saved"], nsaved, B, T, None)
        return rc or lib.b2h_tenc_backward(m._handle, pa, ma, p, q["dy"], q["saved"], nsaved, q["dx"], ga, q["ws"], nws, B, T,
                                           None)
    res = both(call, inputs, outs, cuda_device, [shifts], scratch={"saved": nsaved, "ws": nws})
    if (B, T) == (3, 17):                                  # the aligned side against the float64 port
        y64, g64, dx64 = TE.port_grads(x, state, masks, p, dy, torch.float64)
        _, g32, dx32 = TE.port_grads(x, state, masks, p, dy, torch.float32)
        assert float((res["y"].cpu().double() - y64).abs().max()) <= TOL_Y * max(1.0, float(y64.abs().max()))
        for i, (a, b) in enumerate(zip(g64, g32)):
            assert_within_bar(res[f"g{i}"].cpu().double().numpy(), a.numpy(), (b.double() - a).abs().max(), f"g{i}")
        assert_within_bar(res["dx"].cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "dx")


# ---- TextPoseTransformer training ---------------------------------------------------------------------------------
TPT_TRAIN = [((12, 42), 17, "valu"), ((12, 42), 17, "mfma"), ((29, 8), 17, "valu"), ((29, 8), 17, "mfma"),
             ((12, 42), 130, "valu")]


@pytest.mark.parametrize("combo,T,route", TPT_TRAIN, ids=lambda v: "j%d_o%d" % v if isinstance(v, tuple) else str(v))
def test_tpt_training_params_grads_and_tokens_off_the_grid(combo, T, route, cuda_device):
    """b2h_tpt_train_forward + b2h_tpt_backward, (1 enc, 1 dec), (B, S) = (3, 9): every parameter (the embedding table
    among them: b2h_embed_dwords) and gradient at +4 / +8 / +12, the token ids at +8.  (29, 8): K = 58 (K & 3 != 0) and
    M = 8 (M & 3 == 0) with a shifted W.  T = 130: the blocked attention."""
    B, S, p = 3, 9, 0.1
    state = G.recipe_state(60 + combo[0], 50, *combo, 1, 1)
    m = G.train_model(state, p, cuda_device)
    lib, _ = m._ensure_created()
    assert lib.b2h_tpt_set_train_kernel(m._handle, _lib.TRAIN_KERNELS[route]) == _lib.OK
    assert lib.b2h_tpt_set_train_linear(m._handle, _lib.TRAIN_KERNELS[route]) == _lib.OK
    assert lib.b2h_tpt_train_linear_name(m._handle).decode() == {"valu": "b2h_tt_linear", "mfma": "b2h_ml_linear"}[route]
    assert lib.b2h_tpt_train_attn_name(m._handle, T).decode() == ("b2h_tt_sdpa" if T <= 128 else "b2h_lt_sdpa")
    g = torch.Generator().manual_seed(310 + T)
    tok = tokens_with_padding(B, S, 50, g)
    x = torch.randn((B, T, combo[0], 2), generator=g)
    dy = torch.randn((B, T, combo[1] // 2, 2), generator=g)
    masks = cpu_masks(B, S, T, 1, 1, p, 311)
    tensors = [t.detach().cpu() for t in m._tensors()]
    keys = tpt_param_keys(1, 1)
    n = len(tensors)
    inputs = dict(tok=tok, x=x, dy=dy)
    inputs.update({f"p{i}": t for i, t in enumerate(tensors)})
    inputs.update({f"m{i}": t for i, t in enumerate(masks.values())})
    outs = {f"g{i}": tuple(t.shape) for i, t in enumerate(tensors)}
    outs["dx"], outs["y"] = tuple(x.shape), tuple(dy.shape)
    shifts = weak4([f"p{i}" for i in range(n)])
    shifts.update(weak4([f"g{i}" for i in range(n)], start=1))
    shifts["tok"] = 8
    assert shifts[f"p{keys.index('token_embedding.weight')}"] in (4, 8, 12)
    assert all_residues(shifts, [f"p{i}" for i, t in enumerate(tensors) if t.dim() == 2])
    assert all_residues(shifts, [f"p{i}" for i, t in enumerate(tensors) if t.dim() == 1])
    nsaved, nws = lib.b2h_tpt_train_bytes(m._handle, B, S, T, 0), lib.b2h_tpt_train_bytes(m._handle, B, S, T, 1)

    def call(q):
        pa = (vp * n)(*[q[f"p{i}"] for i in range(n)])
        ma = (vp * len(masks))(*[q[f"m{i}"] for i in range(len(masks))])
        ga = (vp * n)(*[q[f"g{i}"] for i in range(n)])
        rc = lib.b2h_tpt_train_forward(m._handle, pa, q["tok"], q["x"], ma, p, q["y"], q["saved"], nsaved, B, S, T, None)
        return rc or lib.b2h_tpt_backward(m._handle, pa, q["tok"], ma, p, q["dy"], q["saved"], nsaved, q["dx"], ga, q["ws"],
                                          nws, B, S, T, None)
    res = both(call, inputs, outs, cuda_device, [shifts], scratch={"saved": nsaved, "ws": nws})
    y64, g64, dx64 = G.port_grads(tok, x, state, masks, p, dy, torch.float64)
    _, g32, dx32 = G.port_grads(tok, x, state, masks, p, dy, torch.float32)
    assert float((res["y"].cpu().double() - y64).abs().max()) <= G.tol(y64)
    for i, (a, b) in enumerate(zip(g64, g32)):
        assert_within_bar(res[f"g{i}"].cpu().double().numpy(), a.numpy(), (b.double() - a).abs().max(), keys[i])
    assert_within_bar(res["dx"].cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "dx")


# ---- ConvModel training ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_emb", [False, True])
@pytest.mark.parametrize("C", [30, 65])
def test_conv_training_params_and_grads_off_the_grid(C, pos_emb, cuda_device):
    """b2h_train_forward + b2h_backward, B = 3; T = 9, or the 100 frames a pos_emb model requires (B2H_ERR_SHAPE else)."""
    B, T = 3, 100 if pos_emb else 9
    torch.manual_seed(21 + C)
    m = hps.ConvModel(C, "ReLU", pos_emb).to(cuda_device).train()
    state = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    lib, _ = m._ensure_created()
    g = torch.Generator().manual_seed(22)
    x = torch.randn((B, T, 12, 2), generator=g)
    dy = torch.randn((B, T, 21, 2), generator=g)
    params = {f"p{i}": q.detach().cpu() for i, q in enumerate(m._params())}
    outs = {f"g{i}": tuple(q.shape) for i, q in enumerate(m._params())}
    outs["dx"], outs["y"] = (B, T, 12, 2), (B, T, 21, 2)
    shifts = weak4(list(params))
    shifts.update(weak4([f"g{i}" for i in range(8)], start=1))
    assert all_residues(shifts, list(params)) and all_residues(shifts, [f"g{i}" for i in range(8)])
    nbytes = lib.b2h_backward_workspace_bytes(m._handle, B, T)

    def call(q):
        pa = (vp * 8)(*[q[f"p{i}"] for i in range(8)])
        ga = (vp * 8)(*[q[f"g{i}"] for i in range(8)])
        rc = lib.b2h_train_forward(m._handle, pa, q["x"], q["y"], B, T, None)
        return rc or lib.b2h_backward(m._handle, pa, q["x"], q["dy"], q["dx"], ga, B, T, q["ws"], nbytes, None)
    res = both(call, dict(x=x, dy=dy, **params), outs, cuda_device, [shifts], scratch={"ws": nbytes})
    y64, g64, dx64 = train_ref.port_grads(x, state, dy, pos_emb, torch.float64)
    _, g32, dx32 = train_ref.port_grads(x, state, dy, pos_emb, torch.float32)
    assert float((res["y"].cpu().double() - y64).abs().max()) <= TOL_Y * max(1.0, float(y64.abs().max()))
    for i, (a, b) in enumerate(zip(g64, g32)):
        assert_within_bar(res[f"g{i}"].cpu().double().numpy(), a.numpy(), (b.double() - a).abs().max(), f"g{i}")
    assert_within_bar(res["dx"].cpu().double().numpy(), dx64.numpy(), (dx32.double() - dx64).abs().max(), "dx")


# ---- the eight loss entry points -------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [4, 12, 21])
@pytest.mark.parametrize("weighted", [False, True], ids=["masked", "weighted"])
def test_loss_entry_points_off_the_grid(weighted, J, cuda_device):
    """Forward: pred, target, scores, per_seq and loss are promised fp32 alignment only, n_frames its int64's 8 bytes.
    Backward: pred, target and dpred are checked for 16 bytes; scores, dloss and n_frames are not.  J = 21 runs the
    fixed-width entry points, 4 and 12 the *_joints ones.  Bits, not values: the empty sequence's NaN is legitimate."""
    B, T, lengths = 3, 5, [5, 0, 2]
    lib = _lib.load()
    g = torch.Generator().manual_seed(40 + J)
    P, Tg, S = torch.randn((B, T, J, 2), generator=g), torch.randn((B, T, J, 2), generator=g), torch.rand((B, T, J), generator=g)
    P[0, 1, 2, 1] = Tg[0, 1, 2, 1] = 0.25                                       # a tie: sign(0) = 0
    inputs = {"p": P, "t": Tg, "nf": torch.tensor(lengths, dtype=torch.int64)}
    if weighted:
        inputs["s"] = S

    def fwd(q):
        if J == 21:
            if weighted:
                return lib.b2h_weighted_l1(q["p"], q["t"], q["s"], q["nf"], B, T, q["per"], q["loss"], None)
            return lib.b2h_masked_l1(q["p"], q["t"], q["nf"], B, T, q["per"], q["loss"], None)
        if weighted:
            return lib.b2h_weighted_l1_joints(q["p"], q["t"], q["s"], q["nf"], B, T, J, q["per"], q["loss"], None)
        return lib.b2h_masked_l1_joints(q["p"], q["t"], q["nf"], B, T, J, q["per"], q["loss"], None)
    sets = [{"p": a, "t": b, "s": c, "nf": 8, "per": d, "loss": e} for a, b, c, d, e in
            ((4, 8, 12, 4, 8), (8, 12, 4, 12, 4), (12, 4, 8, 8, 12))]
    sets = [{k: v for k, v in s.items() if k in inputs or k in ("per", "loss")} for s in sets]
    out = both(fwd, inputs, {"per": (B,), "loss": (1,)}, cuda_device, sets)
    kind = "confL1" if weighted else "L1"
    want = [train_ref.reference_loss(P[i:i + 1].double().clone(), Tg[i:i + 1].double(), lengths[i:i + 1], S[i:i + 1].double(), kind)
            for i in range(B)]
    np.testing.assert_allclose(out["per"].cpu().numpy(), np.array([float(w) for w in want]), rtol=5e-6)   # NaN where it is NaN
    assert np.isnan(float(out["loss"][0])) and np.isnan(float(want[1]))

    inputs["g"] = torch.tensor([3.0])

    def bwd(q):
        if J == 21:
            if weighted:
                return lib.b2h_weighted_l1_backward(q["p"], q["t"], q["s"], q["nf"], B, T, q["g"], q["d"], None)
            return lib.b2h_masked_l1_backward(q["p"], q["t"], q["nf"], B, T, q["g"], q["d"], None)
        if weighted:
            return lib.b2h_weighted_l1_joints_backward(q["p"], q["t"], q["s"], q["nf"], B, T, J, q["g"], q["d"], None)
        return lib.b2h_masked_l1_joints_backward(q["p"], q["t"], q["nf"], B, T, J, q["g"], q["d"], None)
    sets = [{k: v for k, v in s.items() if k in inputs} for s in
            ({"s": 4, "nf": 8, "g": 8}, {"s": 8, "nf": 8, "g": 12}, {"s": 12, "nf": 8, "g": 4})]
    got = both(bwd, inputs, {"d": (B, T, J, 2)}, cuda_device, sets)["d"].cpu().double()
    ref = {}
    for dt in (torch.float64, torch.float32):
        pp = P.to(dt).clone().requires_grad_(True)
        (train_ref.reference_loss(pp.clone(), Tg.to(dt), lengths, S.to(dt), kind) * 3.0).backward()
        ref[dt] = pp.grad.double()
    assert not got[1].any() and not got[2, 2:].any() and got[0, 1, 2, 1] == 0
    assert_within_bar(got.numpy(), ref[torch.float64].numpy(), (ref[torch.float32] - ref[torch.float64]).abs().max(), kind)


# ---- inference: TransformerEnc ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_tenc_inference_y_off_the_grid(precision, cuda_device):
    """b2h_tenc_forward and b2h_tenc_forward_fused with every flag: y at +4, +8 and +12 (its stores are raw buffer
    stores: dword aligned by construction), n_frames at +8; (B, T) = (3, 17)."""
    B, T = 3, 17
    torch.manual_seed(3)
    m = hps.TransformerEnc(24, 4, 128, 42, 2, precision=precision).to(cuda_device).eval()
    state = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    lib = m._ensure_handle()
    assert lib.b2h_tenc_set_kernel(m._handle, hps.transformer_enc.TENC_KERNELS[precision]) == _lib.OK
    nws = lib.b2h_tenc_workspace_bytes(m._handle, B, T)
    g = torch.Generator().manual_seed(4)
    x = torch.rand((B, T, 12, 2), generator=g) - 0.5
    body = torch.rand((B, T, 12, 2), generator=g) * torch.tensor([1280.0, 720.0])
    nf = np.array([17, 5, 0])
    y = both(lambda q: lib.b2h_tenc_forward(m._handle, q["x"], q["y"], B, T, q["ws"], nws, None), {"x": x}, {"y": (B, T, 21, 2)},
             cuda_device, [{"y": s} for s in (4, 8, 12)], scratch={"ws": nws})["y"].cpu().numpy()
    assert np.abs(y - oracle.transformer_forward(x.numpy(), state)).max() <= TOL_Y
    yf = both(lambda q: lib.b2h_tenc_forward_fused(m._handle, q["x"], q["y"], B, T, ALL_FLAGS, FACTOR, q["nf"], q["ws"], nws, None),
              {"x": body, "nf": torch.from_numpy(nf)}, {"y": (B, T, 21, 2)}, cuda_device,
              [{"y": s, "nf": 8} for s in (4, 8, 12)], scratch={"ws": nws})["y"].cpu().numpy()
    inp, _ = oracle.preprocess(body.numpy(), None)
    ref = oracle.postprocess(oracle.transformer_forward(inp, state), FACTOR, nf)
    assert np.abs(yf - ref).max() <= 2 * TOL_Y * FACTOR                         # test_poisoned_buffers.py's fused bar
    assert not yf[1, 5:].any() and not yf[2].any()


# ---- inference: TextPoseTransformer ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("T", [17, 130])
@pytest.mark.parametrize("combo", [(12, 42), (21, 24), (29, 8)], ids=lambda c: "j%d_o%d" % c)
def test_tpt_inference_y_and_tokens_at_8_bytes(combo, T, precision, cuda_device):
    """b2h_tpt_forward (T <= 128) and b2h_tpt_forward_fused (T = 130: the long path) with y, the token ids and n_frames at
    +8, the weakest the header allows; nout 42, 24 and 8."""
    cpu, check, model = combo_models(*combo)
    model.set_precision(precision)
    lib, _ = model._ensure_handle()
    h = model._handle
    assert lib.b2h_tpt_set_kernel(h, hps.transformer_enc.TENC_KERNELS[precision]) == _lib.OK
    B, S = 3, 9
    tok, pose = G.inputs(B, S, T, cpu.n_tokens, combo[0], 200 + T)
    n_frames = torch.tensor([T, 5, 0], dtype=torch.int64)
    nws = _ws_bytes(model, B, S, T)
    shape = (B, T, combo[1] // 2, 2)
    want = check(tok, pose)
    if T <= 128:
        y = both(lambda q: lib.b2h_tpt_forward(h, q["tokens"], q["x"], q["y"], B, S, T, q["ws"], nws, None),
                 {"tokens": tok, "x": pose}, {"y": shape}, cuda_device, [{"tokens": 8, "y": 8}], scratch={"ws": nws})["y"]
        assert float((y.cpu().double() - want).abs().max()) <= G.tol(want)
    yf = both(lambda q: lib.b2h_tpt_forward_fused(h, q["tokens"], q["x"], q["y"], B, S, T, POST, FACTOR, q["nf"], q["ws"], nws, None),
              {"tokens": tok, "x": pose, "nf": n_frames}, {"y": shape}, cuda_device, [{"tokens": 8, "y": 8, "nf": 8}],
              scratch={"ws": nws})["y"]
    want = want * FACTOR
    want[1, 5:] = 0
    want[2] = 0
    assert float((yf.cpu().double() - want).abs().max()) <= G.tol(want / FACTOR) * FACTOR
    assert not yf[1, 5:].any() and not yf[2].any()


@pytest.mark.parametrize("predict,n_joints", [("right_index", 29), ("right_3fingers", 21)])
def test_item_kernel_with_all_three_pointers_at_8_bytes(predict, n_joints, cuda_device):
    B, T = 3, 17
    g = torch.Generator().manual_seed(11)
    body = torch.rand((B, T, 12, 2), generator=g) * FACTOR
    hand = torch.rand((B, T, 21, 2), generator=g) * FACTOR
    lib = _lib.load()
    flags = _lib.PRE_CHEST_DIFF | _lib.PRE_NORMALIZE
    out = both(lambda q: lib.b2h_tpt_build_item(q["body"], q["hand"], q["item"], B, T, _lib.PREDICT[predict], flags, FACTOR, None),
               {"body": body, "hand": hand}, {"item": (B, T, n_joints, 2)}, cuda_device,
               [{"body": 8, "hand": 8, "item": 8}])["item"].cpu().numpy()
    want = _numpy_item(body.numpy().reshape(B * T, 12, 2), hand.numpy().reshape(B * T, 21, 2), predict, True, True)
    assert np.array_equal(out.reshape(B * T, n_joints, 2).view(np.int32), want.view(np.int32))


def test_build_batch_with_every_pointer_at_8_bytes(cuda_device):
    """The committed h5_store fixture: the store, the batch description and all five outputs at +8."""
    rec = batch_ref.load_fixture("h5_store")
    rows, offsets, n_body, tokens = rec["store"]
    T, S = rec["T"], rec["S"]
    key = ("right_hand", 1, 1, "first", "c")
    utt, start = rec["lists"]["c"], rec["starts"][("first", "c")]
    B = utt.numel()
    ji, jt = batch_ref.joints("right_hand", n_body)
    flags = _lib.BATCH_DIF_ENCODING | _lib.BATCH_NORMALIZE
    lib = _lib.load()
    ins = {"rows": rows, "offsets": offsets, "tokens": tokens, "utt": utt, "start": start}
    outs = {"input_kp": (B, T, ji, 2), "target_kp": (B, T, jt, 2), "target_conf": (B, T, jt), "text_tokens": (B, S, 2),
            "n_frames": (B, 2)}                                       # an int64 output counts as two words
    out = both(lambda q: lib.b2h_build_batch(q["rows"], rows.shape[0], q["offsets"], offsets.numel() - 1, n_body, q["tokens"], S,
                                             q["utt"], q["start"], B, T, _lib.PREDICT["right_hand"], flags, FACTOR, q["input_kp"],
                                             q["target_kp"], q["target_conf"], q["text_tokens"], q["n_frames"], None),
               ins, outs, cuda_device, [{k: 8 for k in list(ins) + list(outs)}])
    got = {k: out[k].cpu() for k in ("input_kp", "target_kp", "target_conf")}
    got["text_tokens"] = out["text_tokens"].cpu().view(torch.int64).view(B, S)
    got["n_frames"] = out["n_frames"].cpu().view(torch.int64).view(B)
    for k, w in rec["expected"][key].items():
        assert batch_ref.same_bits(got[k], w), k


# ---- the Python surface: parameters that are views of one flat buffer ----------------------------------------------
def _reseat(tensors, dev):
    """Re-seat every tensor as a view of one flat fp32 buffer, tensor i at 4 * (1 + i % 3) bytes past the 16-byte grid."""
    total = sum((t.numel() + 3) // 4 * 4 + 4 for t in tensors)
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    o = 0
    for i, t in enumerate(tensors):
        o = (o + 3) // 4 * 4 + 1 + i % 3
        n = t.numel()
        flat[o:o + n].copy_(t.data.reshape(-1))
        t.data = flat[o:o + n].view_as(t)
        assert t.data_ptr() % 16 == 4 * (1 + i % 3) and t.is_contiguous()
        o += n
    return flat


def _surface_models(kind, dev):
    """(model, its tensors to re-seat, step(model) -> (y, dx), eval run(model) -> y) for one of the three models."""
    g = torch.Generator().manual_seed(70)
    if kind == "conv":
        torch.manual_seed(71)
        m = hps.ConvModel(30, "ReLU", False)
        x = torch.randn((3, 9, 12, 2), generator=g).to(dev)
        dy = torch.randn((3, 9, 21, 2), generator=g).to(dev)
        return m, (lambda q: list(q.parameters())), (lambda q, xd: q(xd)), (lambda q: q(x)), x, dy
    if kind == "tenc":
        state = _noisy(TE.seeded_state(2, 72), 73, skip=("pos_encoder.pe",))
        m = hps.TransformerEnc(24, 4, 128, 42, 2, dropout=0.1)
        m.load_state_dict(state)
        x = torch.randn((3, 17, 12, 2), generator=g).to(dev)
        dy = torch.randn((3, 17, 21, 2), generator=g).to(dev)
        masks = {}

        def fwd(q, xd):
            if not masks:
                torch.manual_seed(74)
                masks.update(q._draw_dropout_masks(3, 17))
            return q._forward_train(xd, masks)
        return m, (lambda q: q._tensors()), fwd, (lambda q: q(x)), x, dy
    m = G.train_model(G.recipe_state(75, 50, 29, 8, 1, 1), 0.1)
    tok = tokens_with_padding(3, 9, 50, g).to(dev)
    x = torch.randn((3, 17, 29, 2), generator=g).to(dev)
    dy = torch.randn((3, 17, 4, 2), generator=g).to(dev)
    masks = {}

    def fwd(q, xd):
        if not masks:
            torch.manual_seed(76)
            masks.update(q._draw_dropout_masks(3, 9, 17))
        return q._forward_train(tok, xd, masks)
    return m, (lambda q: q._tensors()), fwd, (lambda q: q(tok, x)), x, dy


@pytest.mark.parametrize("kind", ["conv", "tenc", "tpt"])
def test_parameters_viewed_from_one_flat_buffer(kind, cuda_device):
    """A gradient-bucket / flattened-parameter layout: `p.data = flat[o:o+n].view_as(p)` at mixed residues.  One autograd
    step, two steps of the native Adam and eval-mode inference (the packer reads the shifted pointers) give the bits of
    a twin model with ordinary parameters."""
    cpu, tensors_of, fwd, infer, x, dy = _surface_models(kind, cuda_device)
    twin = copy.deepcopy(cpu).to(cuda_device).train()
    flat_model = copy.deepcopy(cpu).to(cuda_device).train()
    flat = _reseat(tensors_of(flat_model), cuda_device)
    assert {t.data_ptr() % 16 for t in tensors_of(flat_model)} == {4, 8, 12}
    assert all(t.data_ptr() % 16 == 0 for t in tensors_of(twin))
    results = []
    for m in (twin, flat_model):
        opt = hps.Adam(m.parameters(), lr=1e-3)
        xd = x.clone().requires_grad_(True)
        fwd(m, xd).backward(dy)
        first = ([p.grad.clone() for p in m.parameters()], xd.grad.clone())
        opt.step()
        opt.zero_grad()
        fwd(m, x.clone().requires_grad_(True)).backward(dy)
        opt.step()
        after = [p.detach().clone() for p in m.parameters()]
        m.eval()
        with torch.no_grad():
            y = infer(m)
        results.append((first, after, y))
    (g0, dx0), p0, y0 = results[0]
    (g1, dx1), p1, y1 = results[1]
    assert torch.equal(bits(dx0), bits(dx1)) and torch.equal(bits(y0), bits(y1))
    assert len(g0) == len(g1) and all(torch.equal(bits(a), bits(b)) for a, b in zip(g0, g1))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(p0, p1))
    assert all(t.data_ptr() >= flat.data_ptr() and t.data_ptr() < flat.data_ptr() + 4 * flat.numel()
               for t in tensors_of(flat_model))                                    # still the views: updated in place
    assert not any(torch.equal(a, b.detach()) for a, b in zip(p0, copy.deepcopy(cpu).to(cuda_device).parameters()))


# ---- inputs that start off the grid ---------------------------------------------------------------------------------
def _off_grid(t, dev, shift):
    """A contiguous view holding `t`, `shift` bytes past the 16-byte grid of a flat buffer."""
    flat = torch.zeros(t.numel() + 4, dtype=t.dtype, device=dev)
    assert flat.data_ptr() % 16 == 0 and shift % t.element_size() == 0
    o = shift // t.element_size()
    v = flat[o:o + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == shift and v.is_contiguous()
    return v


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_tpt_inference_on_a_plain_batch_slice(precision, cuda_device):
    """ninp = 42: pose rows are 168 bytes, so with T = 17 pose[1:] is contiguous and starts 8 bytes off the grid."""
    cpu, _, model = combo_models(21, 24)
    model.set_precision(precision)
    tok, pose = G.inputs(4, 9, 17, cpu.n_tokens, 21, 90)
    tok, pose = tok.to(cuda_device), pose.to(cuda_device)
    sl_tok, sl_pose = tok[1:], pose[1:]
    assert sl_pose.data_ptr() % 16 == 8 and sl_pose.is_contiguous()
    for run in (model, model.forward_long):
        assert torch.equal(bits(run(sl_tok, sl_pose)), bits(run(sl_tok.clone(), sl_pose.clone())))
    g = torch.Generator().manual_seed(91)
    body = torch.rand((3, 17, 12, 2), generator=g) * FACTOR
    hand = torch.rand((3, 17, 21, 2), generator=g) * FACTOR
    nf = torch.tensor([17, 5, 0])
    want = model.forward_fused(sl_tok.clone(), body.to(cuda_device), nf, mask_tail=True, right_hand=hand.to(cuda_device))
    got = model.forward_fused(sl_tok, _off_grid(body, cuda_device, 4), nf, mask_tail=True, right_hand=_off_grid(hand, cuda_device, 12))
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("kind", ["conv", "tenc"])
def test_conv_and_tenc_inference_on_a_view_into_a_flat_buffer(kind, cuda_device):
    torch.manual_seed(92)
    m = (hps.ConvModel(30, "ReLU", False) if kind == "conv" else hps.TransformerEnc(24, 4, 128, 42, 2)).to(cuda_device).eval()
    g = torch.Generator().manual_seed(93)
    x = torch.rand((3, 17, 12, 2), generator=g) - 0.5
    body = torch.rand((3, 17, 12, 2), generator=g) * FACTOR
    target = (torch.rand((3, 17, 21, 2), generator=g) - 0.5) * 0.2
    nf = [17, 5, 1]
    xv, bv, tv = (_off_grid(t, cuda_device, 4) for t in (x, body, target))
    with torch.no_grad():
        assert torch.equal(bits(m(xv)), bits(m(xv.clone())))
        assert torch.equal(bits(m.forward_fused(bv, nf, mask_tail=True)), bits(m.forward_fused(bv.clone(), nf, mask_tail=True)))
    for loss in ("L1", "confL1"):
        conf = torch.rand((3, 17, 21), generator=g)
        off = [{"body_kp": xv, "target_kp": tv, "n_frames": nf, "target_conf": _off_grid(conf, cuda_device, 8)}]
        on = [{"body_kp": xv.clone(), "target_kp": tv.clone(), "n_frames": nf, "target_conf": conf.to(cuda_device)}]
        a, b = hps.validate(m, off, loss=loss), hps.validate(m, on, loss=loss)
        assert a == b and np.isfinite(a)


def test_forward_into_names_the_16_byte_rule(cuda_device):
    """forward_into takes caller-owned buffers and cannot clone: a Python error that names the rule, for x and for y."""
    torch.manual_seed(94)
    m = hps.ConvModel(30, "ReLU", False).to(cuda_device).eval()
    x = torch.rand((2, 9, 12, 2), device=cuda_device) - 0.5
    y = torch.empty((2, 9, 21, 2), device=cuda_device)
    want = m.forward_into(x, y).clone()
    for xs, ys in ((_off_grid(x, cuda_device, 4), y), (x, _off_grid(y, cuda_device, 8))):
        before = ys.clone()
        with pytest.raises(RuntimeError, match=r"forward_into needs x and y to start on a 16-byte boundary \(data_ptr\(\) % 16 == 0\)"):
            m.forward_into(xs, ys)
        assert torch.equal(ys, before)                                      # nothing launched
    assert torch.equal(m.forward_into(x, y), want)
