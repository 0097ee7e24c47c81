"""Every refusal of the four transformer training entry points (b2h_tenc_train_forward / b2h_tenc_backward /
b2h_tpt_train_forward / b2h_tpt_backward), pinned as the exact (status, b2h_last_error()) pair: one defect per call on
an otherwise valid call, plus doubly-invalid calls that pin which check fires first.  Nothing is launched: every call
is refused on the host, except B = 0 in the forwards, which returns B2H_OK before any launch.

Shapes: TransformerEnc with 1 layer at (B, T) = (1, 2); TextPoseTransformer with (1 enc, 1 dec) at (B, S, T) = (1, 2, 3).
The inputs and outputs are a few hundred bytes; the saved buffer and the scratch have the sizes b2h_*_train_bytes
asks for (the scratch holds one 198 KB slab at any shape), so that a valid call stays valid but for its one defect.
The overlap cases pass an address inside another operand: the range that the library assumes behind it may run past
the end of that tensor (y laid over a 256-byte mask, the scratch over the saved buffer).  That is safe only because
the call is refused before anything is launched, which is what these cases assert.
"""
import ctypes
import warnings

import pytest
import torch

import hand_pose_sl_amd as hps
from hand_pose_sl_amd import _lib

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
OK, INVALID, SHAPE = _lib.OK, _lib.ERR_INVALID, _lib.ERR_SHAPE
NAN = float("nan")


class _Ptrs:
    """A pointer array argument: the good pointers, with single entries or the whole array replaced."""

    def __init__(self, tensors):
        self.p = [t.data_ptr() for t in tensors]

    def with_(self, i, value):
        new = _Ptrs([])
        new.p = list(self.p)
        new.p[i] = value
        return new

    def arg(self):
        return (vp * len(self.p))(*self.p)


def _arg(v):
    if isinstance(v, _Ptrs):
        return v.arg()
    if isinstance(v, torch.Tensor):
        return vp(v.data_ptr())
    return v


class _Harness:
    """A model handle, a valid argument set for each of its two entry points, and `call` to run one with defects."""

    def __init__(self, kind, dev):
        self.kind = kind
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            if kind == "tenc":
                self.model = hps.TransformerEnc(24, 4, 128, 42, 1, dropout=0.0).to(dev).train()
                self.dims = {"B": 1, "T": 2}
                tensors = [t.detach() for t in self.model._tensors()]          # pe, then the 16 parameters
                grads = [torch.zeros_like(t) for t in tensors[1:]]
                mask_numel = [1 * 2 * 24, 1 * 4 * 2 * 2, 256, 256, 256]
            else:
                self.model = hps.TextPoseTransformer(7, 12, 2, 4, 128, 42, 1, 1, dropout=0.0).to(dev).train()
                self.dims = {"B": 1, "S": 2, "T": 3}
                tensors = [t.detach() for t in self.model._tensors()]
                grads = [torch.zeros_like(t) for t in tensors]
                mask_numel = [16, 256, 256, 256, 36, 384, 24, 384, 384, 384]
        self.lib, _ = self.model._ensure_created()
        self.h = self.model._handle
        dims = tuple(self.dims.values())
        bytes_fn = getattr(self.lib, f"b2h_{kind}_train_bytes")
        self.nsaved, self.nscratch = bytes_fn(self.h, *dims, 0), bytes_fn(self.h, *dims, 1)
        f32 = dict(dtype=torch.float32, device=dev)
        B, T = self.dims["B"], self.dims["T"]
        self.good = dict(
            params=_Ptrs(tensors), masks=None, p=0.0,
            x=torch.zeros((B, T, 12, 2), **f32), y=torch.zeros((B, T, 21, 2), **f32),
            dy=torch.zeros((B, T, 21, 2), **f32), dx=torch.zeros((B, T, 12, 2), **f32),
            saved=torch.zeros(self.nsaved, dtype=torch.uint8, device=dev), saved_bytes=self.nsaved,
            scratch=torch.zeros(self.nscratch, dtype=torch.uint8, device=dev), scratch_bytes=self.nscratch,
            grads=_Ptrs(grads), **self.dims)
        if kind == "tpt":
            self.good["tokens"] = torch.zeros((B, self.dims["S"]), dtype=torch.int64, device=dev)
        self.mask_tensors = [torch.ones(n, dtype=torch.uint8, device=dev) for n in mask_numel]
        self.with_masks = dict(p=0.5, masks=_Ptrs(self.mask_tensors))
        self.keep = (tensors, grads)
        self.big_param = max(tensors[1:], key=lambda t: t.numel())     # in_proj_weight: larger than the saved buffer
        torch.cuda.synchronize(dev)

    def call(self, entry, **defects):
        a = dict(self.good, **defects)
        model = a.pop("model", self.h)
        tok = ("tokens",) if self.kind == "tpt" else ()
        dims = tuple(self.dims)
        if entry == "forward":
            names = ("params",) + tok + ("x", "masks", "p", "y", "saved", "saved_bytes") + dims
            fn = getattr(self.lib, f"b2h_{self.kind}_train_forward")
        else:
            names = ("params",) + tok + ("masks", "p", "dy", "saved", "saved_bytes", "dx", "grads", "scratch",
                                         "scratch_bytes") + dims
            fn = getattr(self.lib, f"b2h_{self.kind}_backward")
        rc = fn(model, *[_arg(a[n]) for n in names], None)
        return rc, self.lib.b2h_last_error().decode()

    def off(self, name, by):
        """The address of a good buffer, moved by `by` bytes."""
        return vp(self.good[name].data_ptr() + by)


@pytest.fixture(scope="module")
def harness(cuda_device):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _Harness(kind, cuda_device)
        return made[kind]
    return get


TENC_SHAPE = "expected B >= 0 and T >= 1"
TENC_LEN = "TransformerEnc: T exceeds the positional encoding's max_len (src + pe[:T], HandPoseModels.py:101,167)"
TPT_SHAPE = "expected B >= 0, S >= 1 and T >= 1"
TPT_LEN = "TextPoseTransformer training: S is limited to 128 and T to B2H_TPT_MAX_FRAMES = 1024"
P_RANGE = "dropout p must be in [0, 1]"
MASKS_P = "masks must be given exactly when p > 0"
FWD_NULL = "NULL pointer"
FWD_ALIGN = "x, y and the saved buffer must be 16-byte aligned"
BWD_NULL = "dy / saved / scratch is NULL"
BWD_ALIGN = "dy, dx, the saved buffer and the scratch must be 16-byte aligned"
TENC_B0 = "b2h_tenc_backward needs B >= 1 (the gradients of an empty batch are not defined here)"
TPT_B0 = "b2h_tpt_backward needs B >= 1 (the gradients of an empty batch are not defined here)"

# (name, defects as a function of the harness, status, message or {model: message}).  The byte counts in the messages
# are those of the shapes above: TransformerEnc saved 10464 B, scratch 205312 B; TextPoseTransformer 36848 B and 212992 B.
COMMON = [
    # checks shared by forward and backward of both models, in their order
    ("null_params", lambda h: dict(params=None), INVALID, "params is NULL"),
    ("p_above_1", lambda h: dict(p=1.5), INVALID, P_RANGE),
    ("p_negative", lambda h: dict(p=-0.25), INVALID, P_RANGE),
    ("p_nan", lambda h: dict(p=NAN), INVALID, P_RANGE),
    ("masks_at_p0", lambda h: dict(masks=h.with_masks["masks"]), INVALID, MASKS_P),
    ("no_masks_at_p", lambda h: dict(p=0.5), INVALID, MASKS_P),
    ("null_param_0", lambda h: dict(params=h.good["params"].with_(0, None)), INVALID, "params[0] is NULL"),
    ("null_param_5", lambda h: dict(params=h.good["params"].with_(5, None)), INVALID, "params[5] is NULL"),
    ("misaligned_param", lambda h: dict(params=h.good["params"].with_(2, h.good["params"].p[2] + 2)), INVALID,
     "params must be 4-byte aligned fp32 tensors"),
    ("null_mask_0", lambda h: dict(h.with_masks, masks=h.with_masks["masks"].with_(0, None)), INVALID, "masks[0] is NULL"),
    ("null_mask_4", lambda h: dict(h.with_masks, masks=h.with_masks["masks"].with_(4, None)), INVALID, "masks[4] is NULL"),
    # doubly invalid: the earlier check fires
    ("null_params_and_bad_p", lambda h: dict(params=None, p=2.0), INVALID, "params is NULL"),
    ("bad_p_and_masks", lambda h: dict(p=NAN, masks=h.with_masks["masks"]), INVALID, P_RANGE),
    ("null_param_and_null_mask", lambda h: dict(h.with_masks, params=h.good["params"].with_(1, None),
                                                masks=h.with_masks["masks"].with_(0, None)), INVALID, "params[1] is NULL"),
]
FORWARD = [
    ("b_zero_ok", lambda h: dict(B=0), OK, None),
    ("b_zero_with_null_x_ok", lambda h: dict(B=0, x=None, y=None, saved=None, saved_bytes=0), OK, None),
    ("null_x", lambda h: dict(x=None), INVALID, FWD_NULL),
    ("null_y", lambda h: dict(y=None), INVALID, FWD_NULL),
    ("null_saved", lambda h: dict(saved=None), INVALID, FWD_NULL),
    ("misaligned_x", lambda h: dict(x=h.off("x", 4)), INVALID, FWD_ALIGN),
    ("misaligned_y", lambda h: dict(y=h.off("y", 8)), INVALID, FWD_ALIGN),
    ("misaligned_saved", lambda h: dict(saved=h.off("saved", 4)), INVALID, FWD_ALIGN),
    ("y_over_x", lambda h: dict(y=h.good["x"]), INVALID, "an output overlaps an input"),
    ("saved_over_param", lambda h: dict(saved=h.big_param), INVALID, "an output overlaps a parameter"),
    ("y_over_mask", lambda h: dict(h.with_masks, y=h.mask_tensors[3]), INVALID, "an output overlaps a mask"),
    ("y_over_saved", lambda h: dict(y=h.good["saved"]), INVALID, "two outputs overlap"),
    ("null_x_and_short_saved", lambda h: dict(x=None, saved_bytes=16), INVALID, FWD_NULL),
    ("misaligned_y_and_short_saved", lambda h: dict(y=h.off("y", 4), saved_bytes=16), INVALID, FWD_ALIGN),
]
BACKWARD = [
    ("null_dy", lambda h: dict(dy=None), INVALID, BWD_NULL),
    ("null_saved", lambda h: dict(saved=None), INVALID, BWD_NULL),
    ("null_scratch", lambda h: dict(scratch=None), INVALID, BWD_NULL),
    ("null_grads", lambda h: dict(grads=None), INVALID, "grads is NULL"),
    ("misaligned_dy", lambda h: dict(dy=h.off("dy", 4)), INVALID, BWD_ALIGN),
    ("misaligned_saved", lambda h: dict(saved=h.off("saved", 8)), INVALID, BWD_ALIGN),
    ("misaligned_scratch", lambda h: dict(scratch=h.off("scratch", 4)), INVALID, BWD_ALIGN),
    ("misaligned_dx", lambda h: dict(dx=h.off("dx", 4)), INVALID, BWD_ALIGN),
    ("short_saved", lambda h: dict(saved_bytes=h.nsaved - 1), INVALID, {
        "tenc": "saved buffer smaller than b2h_tenc_train_bytes", "tpt": "saved buffer smaller than b2h_tpt_train_bytes"}),
    ("short_scratch", lambda h: dict(scratch_bytes=h.nscratch - 1), INVALID, {
        "tenc": "scratch smaller than b2h_tenc_train_bytes (205312 B)",
        "tpt": "scratch smaller than b2h_tpt_train_bytes (212992 B)"}),
    ("null_grad_0", lambda h: dict(grads=h.good["grads"].with_(0, None)), INVALID, "grads[0] is NULL"),
    ("null_grad_last", lambda h: dict(grads=h.good["grads"].with_(-1, None)), INVALID,
     {"tenc": "grads[15] is NULL", "tpt": "grads[38] is NULL"}),
    ("misaligned_grad", lambda h: dict(grads=h.good["grads"].with_(3, h.good["grads"].p[3] + 2)), INVALID,
     "grads must be 4-byte aligned"),
    ("b_zero", lambda h: dict(B=0), SHAPE, {"tenc": TENC_B0, "tpt": TPT_B0}),
    ("dx_over_dy", lambda h: dict(dx=h.good["dy"]), INVALID, "an output overlaps an input"),
    ("scratch_over_saved", lambda h: dict(scratch=h.good["saved"], scratch_bytes=h.nscratch), INVALID,
     "an output overlaps an input"),
    ("grad_over_param", lambda h: dict(grads=h.good["grads"].with_(3, h.good["params"].p[4])), INVALID,
     "an output overlaps a parameter"),
    ("dx_over_mask", lambda h: dict(h.with_masks, dx=h.mask_tensors[2]), INVALID, "an output overlaps a mask"),
    ("dx_over_scratch", lambda h: dict(dx=h.good["scratch"]), INVALID, "two outputs overlap"),
    ("grad_over_grad", lambda h: dict(grads=h.good["grads"].with_(1, h.good["grads"].p[2])), INVALID, "two outputs overlap"),
    # doubly invalid: the earlier check fires
    ("b_zero_and_null_dy", lambda h: dict(B=0, dy=None), SHAPE, {"tenc": TENC_B0, "tpt": TPT_B0}),
    ("null_dy_and_null_grads", lambda h: dict(dy=None, grads=None), INVALID, BWD_NULL),
    ("null_grads_and_misaligned_dy", lambda h: dict(grads=None, dy=h.off("dy", 4)), INVALID, "grads is NULL"),
    ("misaligned_dy_and_short_saved", lambda h: dict(dy=h.off("dy", 4), saved_bytes=16), INVALID, BWD_ALIGN),
    ("short_saved_and_short_scratch", lambda h: dict(saved_bytes=16, scratch_bytes=16), INVALID, {
        "tenc": "saved buffer smaller than b2h_tenc_train_bytes", "tpt": "saved buffer smaller than b2h_tpt_train_bytes"}),
    ("short_scratch_and_null_grad", lambda h: dict(scratch_bytes=16, grads=h.good["grads"].with_(0, None)), INVALID, {
        "tenc": "scratch smaller than b2h_tenc_train_bytes (205312 B)",
        "tpt": "scratch smaller than b2h_tpt_train_bytes (212992 B)"}),
    ("null_grad_and_overlap", lambda h: dict(grads=h.good["grads"].with_(2, None), dx=h.good["scratch"]), INVALID,
     "grads[2] is NULL"),
    ("misaligned_grad_1_and_null_grad_2", lambda h: dict(grads=h.good["grads"].with_(1, h.good["grads"].p[1] + 1)
                                                         .with_(2, None)), INVALID, "grads must be 4-byte aligned"),
]
TENC_ONLY = [
    ("t_zero", lambda h: dict(T=0), SHAPE, TENC_SHAPE),
    ("b_negative", lambda h: dict(B=-1), SHAPE, TENC_SHAPE),
    ("t_above_max_len", lambda h: dict(T=101), SHAPE, TENC_LEN),        # pos_encoder's max_len is 100
    ("t_above_128", lambda h: dict(T=129), SHAPE, TENC_LEN),
    ("t_zero_and_null_param", lambda h: dict(T=0, params=h.good["params"].with_(0, None)), SHAPE, TENC_SHAPE),
    ("masks_at_p0_and_t_zero", lambda h: dict(masks=h.with_masks["masks"], T=0), INVALID, MASKS_P),
]
TPT_ONLY = [
    ("t_zero", lambda h: dict(T=0), SHAPE, TPT_SHAPE),
    ("s_zero", lambda h: dict(S=0), SHAPE, TPT_SHAPE),
    ("s_above_128", lambda h: dict(S=129), SHAPE, TPT_LEN),
    ("t_above_1024", lambda h: dict(T=1025), SHAPE, TPT_LEN),
    ("null_tokens", lambda h: dict(tokens=None), INVALID, "tokens is NULL"),
    ("misaligned_tokens", lambda h: dict(tokens=h.off("tokens", 4)), INVALID, "tokens must be 8-byte aligned"),
    ("t_zero_and_null_tokens", lambda h: dict(T=0, tokens=None), SHAPE, TPT_SHAPE),
    ("null_mask_and_null_tokens", lambda h: dict(h.with_masks, masks=h.with_masks["masks"].with_(9, None), tokens=None),
     INVALID, "masks[9] is NULL"),
    ("null_tokens_and_b_zero", lambda h: dict(tokens=None, B=0), None, None),   # status by entry point, below
]
FORWARD_ONLY_SIZES = [
    ("short_saved", lambda h: dict(saved_bytes=h.nsaved - 1), INVALID, {
        "tenc": "saved buffer smaller than b2h_tenc_train_bytes (10464 B)",
        "tpt": "saved buffer smaller than b2h_tpt_train_bytes (36848 B)"}),
]


def _cases():
    out = []
    for kind, only in (("tenc", TENC_ONLY), ("tpt", TPT_ONLY)):
        for entry, own in (("forward", FORWARD + FORWARD_ONLY_SIZES), ("backward", BACKWARD)):
            for name, defects, status, message in COMMON + only + own:
                if name == "null_tokens_and_b_zero":    # tokens may be NULL at B = 0: the forward returns, the backward refuses B
                    status, message = (OK, None) if entry == "forward" else (SHAPE, TPT_B0)
                if isinstance(message, dict):
                    message = message[kind]
                out.append(pytest.param(kind, entry, defects, status, message, id=f"{kind}-{entry}-{name}"))
    return out


def test_byte_counts_of_the_messages(harness):
    assert (harness("tenc").nsaved, harness("tenc").nscratch) == (10464, 205312)
    assert (harness("tpt").nsaved, harness("tpt").nscratch) == (36848, 212992)


@pytest.mark.parametrize("kind, entry, defects, status, message", _cases())
def test_refusal(harness, kind, entry, defects, status, message):
    h = harness(kind)
    rc, err = h.call(entry, **defects(h))
    assert rc == status
    if status != OK:
        assert err == message


@pytest.mark.parametrize("kind", ["tenc", "tpt"])
@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_null_model(harness, kind, entry):
    assert harness(kind).call(entry, model=None) == (INVALID, "model is NULL")
    assert harness(kind).call(entry, model=None, params=None, p=NAN) == (INVALID, "model is NULL")
