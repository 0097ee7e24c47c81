"""TextPoseTransformer with trained-like weights on the MI355X: heads locked onto one or two keys, logits that carry
row-constant offsets of +-100 from the K bias, stack LayerNorms whose rows have a variance below or near eps
(tests/tpt_stress_ref.py; the CPU side, the fixture and the proofs that the cases see what they are for are in
tests/test_tpt_stress_cpu.py).  Which kernels a case runs:

  inference, T <= 128, "fp32":   b2h_attn_f32 (self- and cross-attention), b2h_tpt_layernorm
  inference, T <= 128, "f16x3":  b2h_attn_qkv_h3 / b2h_attn_cross_h3, b2h_tpt_layernorm
  inference, T > 128:            the blocked attention of kernel_attn_long.h in the selected precision for the decoder
                                 (the encoder keeps the short kernels: S <= 128), through forward_fused(..., **OFF)
  training, T <= 128:            b2h_tt_sdpa and its backward, b2h_tt_layernorm and its backward
  training, T > 128, "valu":     b2h_lt_* (kernel_train_attn_long.h) for the decoder's attentions
  training, T > 128, "mfma":     b2h_mt_* (kernel_train_attn_mfma.h); the resolved name is checked

Bars (the project's own): y by the rule of tests/test_tenc_params.py, max|y - y64| <= max(2e-5 * max(1, max|y64|),
k * max|y32 - y64|) with k = 4 for fp32 arithmetic and 16 for f16x3 (the near-eps LayerNorm case: k * max|y32 - y64|
alone), y64 / y32 the float64 / float32 CPU port; gradients by train_ref.assert_within_bar unchanged.  One bar rests
on an emulation: for the `offset` training cases a tensor's err32 is the larger of the plain float32 port's error and
that of tpt_stress_ref.port_grads_like_kernels, the training kernels' arithmetic (bias-first fma chains in the linear
layers, one accumulator per attention sum, P recomputed from a saved log-sum-exp) run in float32 on the CPU; DESIGN.md
section 18 has the measurements behind it.  Every case meets the conditions (a)-(c) of tpt_stress_ref on the CPU ports
before a kernel runs.  The training cases of `peaked` / `offset` use 1 + 1 layers and one sequence from 128 frames on,
which is what the ReLU-margin rule allows under these weights (tpt_stress_ref.TRAIN_LAYERS).
Run with -s for the worst err / bar per route."""
import functools

import pytest
import torch

import test_tpt_train_long_gpu as long_gpu
import tpt_ref
import tpt_stress_ref as sr
from tpt_train_ref import train_model

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "f16x3"]
OFF = dict(dif_encoding=False, normalize=False, denormalize=False, mask_tail=False)
WORST = {}                                               # route -> worst max|y - y64| / bar
WORST_TRAIN = {}                                         # route -> _check_case's record (gradient ratio to err32, y / bar)


@functools.lru_cache(maxsize=None)
def _model(recipe):
    model = tpt_ref.build(sr.N_TOKENS, *sr.LAYERS)
    model.load_state_dict(sr.stressed_state(recipe))
    return model.to("cuda:0").eval()


_REFERENCE = {}


def _checked_reference(recipe, kind, tokens, pose, name):
    """(y64, y32) of the CPU ports for input `name`: computed once, shared and left unchanged; conditions (a) and (b)
    are asserted on a new input before any kernel runs on it."""
    if name not in _REFERENCE:
        y64, y32, _ = sr.ports(tokens, pose, sr.stressed_state(recipe))
        sr.check_inputs(recipe, kind, tokens, pose, y64, y32)
        _REFERENCE[name] = (y64, y32)
    return _REFERENCE[name]


def _run(model, precision, tokens, pose):
    model.set_precision(precision)
    with torch.no_grad():
        if pose.shape[1] <= sr.KB:
            return model(tokens.to("cuda:0"), pose.to("cuda:0")).cpu()
        return model.forward_fused(tokens.to("cuda:0"), pose.to("cuda:0"), **OFF).cpu()


def _check(y, y64, y32, recipe, precision, what):
    bar = sr.y_bar(y64, y32, sr.K[precision], floor=recipe != "lnvar")
    err = float((y.double() - y64).abs().max())
    route = f"inference {'short' if y.shape[1] <= sr.KB else 'long'} {precision}"
    WORST[route] = max(WORST.get(route, 0.0), err / bar)
    print(f"\n{what} {precision}: max|y - y64| = {err:.3e}, bar {bar:.3e} (float32 port: {float((y32.double() - y64).abs().max()):.3e}); "
          f"ERR/BAR {route}: {WORST[route]:.3f}")
    assert bool(torch.isfinite(y).all()) and err <= bar, f"{what} {precision}: max|y - y64| = {err:.3e} > bar {bar:.3e}"
    return bar


# ---- 1. inference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", sr.INFER_CASES, ids=sr.case_id)
def test_inference_matches_float64(case, precision, cuda_device):
    recipe, shape, kind = case
    tokens, pose = sr.case_inputs(recipe, shape, kind)
    y64, y32 = _checked_reference(recipe, kind, tokens, pose, sr.case_id(case))
    y = _run(_model(recipe), precision, tokens, pose)
    assert y.shape == y64.shape and y.dtype == torch.float32
    _check(y, y64, y32, recipe, precision, sr.case_id(case))


# ---- 2. the padded-key trap --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_padded_keys_stay_masked_below_the_negative_offset(precision, cuda_device):
    """S = 17 leaves 15 padded keys in the memory's second tile; HEAD_NEG's real keys all score <= -20 there, so a
    padded key that reads as zeros would take the row and one that holds the K bias would share it (CPU test).  The
    same sequences with 15 more REAL tokens fill that tile: the two outputs must differ, and each must meet its own
    reference."""
    B, S, T = sr.SHAPES[0]
    tokens, pose = sr.case_inputs("offset", (B, S, T), "plain")
    more = torch.randint(1, sr.N_TOKENS - 1, (B, 32 - S), generator=torch.Generator().manual_seed(17))
    filled = torch.cat([tokens, more], 1)
    out, bars, refs = [], [], []
    for name, tok in (("S = 17", tokens), ("S = 32", filled)):
        y64, y32 = _checked_reference("offset", "plain", tok, pose, "trap " + name)
        y = _run(_model("offset"), precision, tok, pose)
        bars.append(_check(y, y64, y32, "offset", precision, "padded-key trap " + name))
        out.append(y)
        refs.append(y64)
    assert float((refs[0] - refs[1]).abs().max()) > 10 * sum(bars)     # the two differ by far more than both bars ...
    assert float((out[0] - out[1]).abs().max()) > 8 * sum(bars)        # ... so the outputs must, too


# ---- 3. batch independence ---------------------------------------------------------------------------------------
def _neighbours(tokens, pose):
    """A benign sequence (one token id, zero pose) and a NaN one to put next to (tokens, pose)."""
    return {"benign": (torch.ones_like(tokens), torch.zeros_like(pose)),
            "NaN": (tokens.clone(), torch.full_like(pose, float("nan")))}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape,kind", [((1, 17, 33), "plain"), ((1, 9, 300), "ramp")], ids=["t33", "t300_ramp"])
def test_stressed_sequence_in_a_batch_equals_itself_alone(shape, kind, precision, cuda_device):
    tokens, pose = sr.case_inputs("offset", shape, kind)
    model = _model("offset")
    alone = _run(model, precision, tokens, pose)
    assert bool(torch.isfinite(alone).all())
    for name, (tok, x) in _neighbours(tokens, pose).items():
        y = _run(model, precision, torch.cat([tokens, tok]), torch.cat([pose, x]))
        assert torch.equal(y[0], alone[0]), name
        assert bool(torch.isfinite(y[1]).all()) == (name == "benign")
        y = _run(model, precision, torch.cat([tok, tokens]), torch.cat([x, pose]))       # and as the second sequence
        assert torch.equal(y[1], alone[0]), name


@pytest.mark.parametrize("route", ["valu", "mfma"])
def test_stressed_sequence_trains_in_a_batch_as_it_does_alone(route, cuda_device):
    """y and dx of the stressed sequence, with its own dropout masks, next to a benign and next to a NaN sequence."""
    shape, p = (1, 17, 130), 0.1
    state = sr.train_state("offset")
    tokens, x = sr.case_inputs("offset", shape, "plain", state=state)
    dy = torch.randn((1, shape[2], 21, 2), generator=torch.Generator().manual_seed(23))
    m = train_model(state, p, cuda_device).set_train_kernels(route)
    torch.manual_seed(24)
    masks = m._draw_dropout_masks(2, shape[1], shape[2])
    first = {k: v[:1].contiguous() for k, v in masks.items()}
    dev = lambda *ts: [t.to(cuda_device) for t in ts]   # noqa: E731
    y0, _, dx0 = long_gpu._step(m, *dev(tokens, x, dy), first)
    assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(dx0).all())
    for name, (tok, xx) in _neighbours(tokens, x).items():
        y, _, dx = long_gpu._step(m, *dev(torch.cat([tokens, tok]), torch.cat([x, xx]), torch.cat([dy, dy])), masks)
        assert torch.equal(y[0], y0[0]) and torch.equal(dx[0], dx0[0]), name


# ---- 4. training -------------------------------------------------------------------------------------------------
def _attn_name(m, T):
    lib, _ = m._ensure_created()
    return lib.b2h_tpt_train_attn_name(m._handle, T).decode()


@pytest.mark.parametrize("case", sr.TRAIN_CASES, ids=sr.case_id)
def test_training_matches_float64_autograd(case, monkeypatch, cuda_device):
    """_check_case of test_tpt_train_long_gpu.py (the kernels' own dropout masks, the ReLU-margin rule) on the stressed
    state: the draws are tpt_stress_ref.case_inputs, admitted by conditions (a) and (b) on the CPU ports; y is held to
    the relative rule, every gradient to assert_within_bar."""
    recipe, shape, kind, route, p = case
    state = sr.train_state(recipe)
    built = []

    def made(st, pp, dev=None):
        built.append(train_model(st, pp, dev).set_train_kernels(route))
        return built[-1]
    worst = WORST_TRAIN.setdefault(f"training {'short' if shape[2] <= sr.KB else route}", {"ratio": 0.0, "what": "", "y": 0.0})
    monkeypatch.setattr(long_gpu, "train_model", made)
    monkeypatch.setattr(long_gpu, "WORST", worst)
    long_gpu._check_case(state, p, *shape, 1.0, 8000 + shape[2], cuda_device,
                         inputs=lambda attempt: sr.case_inputs(recipe, shape, kind, attempt, state),
                         admit=sr.admit(recipe, kind), y_bar=sr.train_y_bar,
                         also32=sr.port_grads_like_kernels if recipe == "offset" else None)
    want = "b2h_tt_sdpa" if shape[2] <= sr.KB else {"valu": "b2h_lt_sdpa", "mfma": "b2h_mt_sdpa"}[route]
    assert len(built) == 1 and built[0].train_kernels == route and _attn_name(built[0], shape[2]) == want


# ---- 5. the record -----------------------------------------------------------------------------------------------
def test_report_worst_ratios():
    """Prints what DESIGN.md section 18 quotes (pytest -s, after the tests above)."""
    print()
    for route, r in sorted(WORST.items()):
        print(f"ERR/BAR {route}: {r:.3f}")
    for route, w in sorted(WORST_TRAIN.items()):
        print(f"{route}: worst max|g - g64| / max|g32 - g64| = {w['ratio']:.3f} ({w['what']}); worst y err / bar = {w.get('y_ratio', 0.0):.3f}")
