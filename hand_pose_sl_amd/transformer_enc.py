"""Drop-in mirror of the reference's `TransformerEnc` (body2hand/src/models/HandPoseModels.py:
118-178), the second text-free body->hand model, on libb2h's gfx950 kernels.

Same constructor `TransformerEnc(ninp, nhead, nhid, nout, nlayers, dropout=0.5)` and the same
`state_dict` (the torch.nn containers are built in the reference's order, so a seeded default
init is identical and its checkpoints load as they are); `model(src)` with src float32
(B, T, 12, 2) -> float32 (B, T, 21, 2).  The torch containers only hold parameters: the forward
runs through the C ABI (`b2h_tenc_forward`).  Only the geometry the reference's CLIs construct
(ninp=24, nhead=4, nhid=128, nout=42; infer_utterance.py:99-101) is implemented.

Training: in training mode with autograd enabled and a parameter or the input requiring a gradient,
`model(src)` runs `_native.TrainFn` -- an exact-fp32 HIP forward and backward (b2h_tenc_train_forward /
b2h_tenc_backward, kernel_tenc_train.h) that read the parameters' own storage -- so the reference's loop
body (steps/traintest.py:87-121) runs unchanged with any torch optimizer.  The dropout keep-masks are
drawn by torch on the model's device (`_draw_dropout_masks`; they follow torch.manual_seed) and handed
to the kernels; after `model.set_dropout_source("native", seed)` libb2h draws them itself, all of a step in one
launch (b2h_dropout_masks, kernel_dropout_masks.h).  Every other call (eval mode or no_grad) runs the inference kernels selected by
`precision`.  No path ever falls back to PyTorch ops.
"""
import ctypes
import math
import warnings

import torch
import torch.nn as nn

from . import _lib
from ._native import NativeDropout, NativeModule, TrainFn, TrainRoutes, _aligned, _ptrs


class PositionalEncoding(nn.Module):
    """Sinusoidal table added to the (T, B, d_model) input; registered as buffer `pe` of shape
    (max_len, 1, d_model) so that it is part of the state_dict like the reference's
    (HandPoseModels.py:86-103).  pe[p, 2i] = sin(p w_i), pe[p, 2i+1] = cos(p w_i),
    w_i = 10000^(-2i/d_model)."""

    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        freq = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        angle = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1) * freq
        table = torch.zeros(max_len, d_model)
        table[:, 0::2] = torch.sin(angle)
        table[:, 1::2] = torch.cos(angle)
        self.register_buffer("pe", table.unsqueeze(0).transpose(0, 1))


TENC_KERNELS = {"fp32": 0, "f16x3": 1}   # b2h_tenc_kernel (include/b2h.h)


class TransformerEnc(NativeDropout, TrainRoutes, NativeModule, nn.Module):
    """`precision` (not in the reference; keyword only): "fp32" = fp32 operands on the matrix cores
    (default); "f16x3" = every Linear operand split into f16 hi + lo, three f16 MFMAs per product
    with fp32 accumulation: fp32-grade error at 3/16 of the matrix cycles, for activations and
    weights inside the f16 range (|x| < 65504).

    Training (model.train(), autograd on, a parameter or the input requires grad): always exact fp32, whatever
    `precision` says, with dropout probability `pos_encoder.dropout.p` everywhere as in the reference; gradients as
    accurate as the reference's own fp32 CPU training (tests/test_tenc_train_gpu.py).  By default every kernel of a
    step runs on the vector ALU; `set_train_kernels("mfma")` (attribute `train_kernels`, default "valu") moves the
    self-attention of every layer, forward and backward, to fp32 MFMA kernels, and `set_train_linear("mfma")`
    (attribute `train_linear`, default "valu") every Linear layer."""

    def __init__(self, ninp, nhead, nhid, nout, nlayers, dropout=0.5, *, precision="fp32"):
        super().__init__()
        if precision not in TENC_KERNELS:
            raise ValueError(f"precision must be one of {sorted(TENC_KERNELS)}, got {precision!r}")
        self.precision = precision
        self.train_kernels = "valu"
        self.train_linear = "valu"
        self.model_type = "Transformer"
        self.src_mask = None
        self.pos_encoder = PositionalEncoding(ninp, dropout, max_len=100)
        encoder_layers = nn.TransformerEncoderLayer(nhid, nhead, nhid, dropout)
        with warnings.catch_warnings():  # torch notes that seq-first layers skip its nested-tensor path
            warnings.simplefilter("ignore", UserWarning)
            self.transformer_encoder = nn.TransformerEncoder(encoder_layers, nlayers)
        self.ninp = ninp
        self.hidden2pose_projection = nn.Linear(nhid, nout)
        self.pose2hidden_projection = nn.Linear(ninp, nhid)
        self._geom = (int(ninp), int(nhead), int(nhid), int(nout), int(nlayers))

    def set_train_kernels(self, name):
        """Select the attention kernels of later training forwards, "valu" (the default) or "mfma"; returns self.
        "mfma" runs every layer's self-attention, forward and backward, on v_mfma_f32_16x16x4_f32
        (kernel_train_attn_whole_mfma.h): exact fp32 and as deterministic as the default; the forward is bitwise equal
        to the default's, the backward sums one row term in another order.  A backward runs the route its forward ran,
        whatever the model says by then.  Measurements: DESIGN.md section 25."""
        return self._choose_train_route("train_kernels", "train kernels", name)

    def set_train_linear(self, name):
        """Select the Linear kernels of later training forwards, "valu" (the default) or "mfma"; returns self.  "mfma"
        runs every Linear layer of the step, forward and backward, on v_mfma_f32_16x16x4_f32
        (kernel_train_linear_mfma.h): bitwise equal to the default.  Independent of `set_train_kernels`; LayerNorm,
        the positional encoding and inference are untouched.  A backward runs the Linears its forward ran."""
        return self._choose_train_route("train_linear", "train linear", name)

    _NAME, _CREATE, _LOAD, _DESTROY = "TransformerEnc", "b2h_tenc_create", "b2h_tenc_load_weights", "b2h_tenc_destroy"

    def _tensors(self):
        # through the module dictionaries (53 tensors; nn.Module.__getattr__ would cost ~50 us per forward)
        M = self._modules
        p2h = M["pose2hidden_projection"]._parameters
        t = [M["pos_encoder"]._buffers["pe"], p2h["weight"], p2h["bias"]]
        for layer in M["transformer_encoder"]._modules["layers"]._modules.values():
            lm = layer._modules
            sa = lm["self_attn"]
            for owner, names in ((sa._parameters, ("in_proj_weight", "in_proj_bias")),
                                 (sa._modules["out_proj"]._parameters, ("weight", "bias")),
                                 (lm["linear1"]._parameters, ("weight", "bias")), (lm["linear2"]._parameters, ("weight", "bias")),
                                 (lm["norm1"]._parameters, ("weight", "bias")), (lm["norm2"]._parameters, ("weight", "bias"))):
                t.append(owner[names[0]])
                t.append(owner[names[1]])
        h2p = M["hidden2pose_projection"]._parameters
        t.append(h2p["weight"])
        t.append(h2p["bias"])
        return t

    def _device(self):
        return self._modules["pose2hidden_projection"]._parameters["weight"].device

    def _handle_key(self, dev):
        # the handle is made for one device and one max_len (b2h_tenc_load_weights reads max_len rows of pe)
        return dev.index, int(self._modules["pos_encoder"]._buffers["pe"].shape[0])

    def _create_args(self):
        return self._geom + (int(self._modules["pos_encoder"]._buffers["pe"].shape[0]),)

    def _wants_grad(self, src):
        """The training path's condition: training mode, autograd on, a parameter or the input needs a gradient."""
        return (self.training and torch.is_grad_enabled() and
                (src.requires_grad or any(p.requires_grad for p in self._tensors()[1:])))

    def _check_input(self, src):
        if src.dim() != 4 or src.shape[2] * src.shape[3] != self.ninp:
            raise RuntimeError(f"expected input of shape (B, T, {self.ninp // 2}, 2), got {tuple(src.shape)}")
        return src.to(device=self._device(), dtype=torch.float32, non_blocking=True).contiguous()

    def _mask_order(self, B, T):
        """(key, shape) of every keep-mask in the order of b2h_tenc_train_forward (include/b2h.h)."""
        order = [("pos", (B, T, self.ninp))]
        for l in range(self._geom[4]):
            order.append(((l, "attn"), (B, self._geom[1], T, T)))
            order += [((l, name), (B, T, self._geom[2])) for name in ("drop1", "ff", "drop2")]
        return order

    def _draw_dropout_masks(self, B, T):
        """The keep-masks of one training forward: uint8, 1 = keep with probability 1 - p, drawn on the model's
        device with torch's generator (so they follow torch.manual_seed), or under `dropout_source` "native" by
        b2h_dropout_masks as views of one allocation (mask number = position; `set_dropout_source`), in either
        case in this fixed order: `pos` (B, T, 24);
        then layer by layer `attn` (B, 4, T, T), `drop1`, `ff`, `drop2` (B, T, 128 each), keyed (layer, name).
        An empty dict at p = 0."""
        return self._drawn_masks(float(self._modules["pos_encoder"]._modules["dropout"].p), B, T)

    def _forward_train(self, src, masks):
        """The differentiable forward (`_native.TrainFn`) with the given keep-masks (`_draw_dropout_masks`)."""
        x = self._check_input(src)
        p = float(self._modules["pos_encoder"]._modules["dropout"].p)
        tensors = self._tensors()
        return TrainFn.apply(self, p, self._checked_masks(masks, p, x.device, x.shape[0], x.shape[1]), tensors[0], x,
                             *tensors[1:])

    # what TrainFn asks of the model: pe travels as params[0] of the entry points and has no gradient; the two routes
    # travel to the backward
    _TRAIN_FNS = ("b2h_tenc_train_bytes", "b2h_tenc_train_forward", "b2h_tenc_backward")
    _TRAIN_LEAD_IS_PARAM = True

    def _train_shapes(self, pe, x):
        B, T = x.shape[0], x.shape[1]
        return (B, T), (B, T, 21, 2), (B, T, 12, 2)

    def _train_head(self, pe, params):
        return (_ptrs((pe, *params)),)

    def _train_route(self):
        return (("b2h_tenc_set_train_kernel", _lib.TRAIN_KERNELS[self.train_kernels]),
                ("b2h_tenc_set_train_linear", _lib.TRAIN_KERNELS[self.train_linear]))

    def _run(self, src, flags, factor, n_frames):
        lib = self._ensure_handle()
        if src.dim() != 4 or src.shape[2] * src.shape[3] != self.ninp:
            raise RuntimeError(f"expected input of shape (B, T, {self.ninp // 2}, 2), got {tuple(src.shape)}")
        dev = self._modules["pose2hidden_projection"]._parameters["weight"].device
        x = _aligned(src.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous())
        B, T = x.shape[0], x.shape[1]
        nf = None
        if flags & _lib.POST_MASK_TAIL:
            if n_frames is None:
                raise ValueError("mask_tail needs n_frames")
            nf = torch.as_tensor(n_frames).to(device=dev, dtype=torch.int64).contiguous()
            if nf.shape != (B,):
                raise RuntimeError(f"n_frames must have shape ({B},)")
        y = torch.empty((B, T, 21, 2), dtype=torch.float32, device=dev)
        need = lib.b2h_tenc_workspace_bytes(self._handle, B, T)
        ws = self._grown_workspace(need, dev)
        with _lib.on_device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.b2h_tenc_set_kernel(self._handle, TENC_KERNELS[self.precision]))
            if flags == 0:
                _lib.check(lib.b2h_tenc_forward(self._handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                                B, T, ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(st)))
            else:
                _lib.check(lib.b2h_tenc_forward_fused(self._handle, ctypes.c_void_p(x.data_ptr()),
                                                      ctypes.c_void_p(y.data_ptr()), B, T, flags, float(factor),
                                                      ctypes.c_void_p(nf.data_ptr()) if nf is not None else None,
                                                      ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(st)))
        return y

    def forward(self, src):
        if self._wants_grad(src):
            x = self._check_input(src)
            return self._forward_train(x, self._draw_dropout_masks(x.shape[0], x.shape[1]))
        return self._run(src, 0, 1.0, None)

    def forward_fused(self, body, n_frames=None, dif_encoding=True, normalize=True, denormalize=True,
                      mask_tail=False, factor=1280.0):
        """Raw-pixel body keypoints in, pixel-space hand keypoints out, with the item transforms inside
        the model's own first and last kernel: ChestDifference + /factor (steps/utils.py:180-210) on the
        rows as they enter (before the positional encoding, HandPoseModels.py:167) -> the encoder ->
        x factor (traintest.py:270-271) and the optional tail mask (utils.py:309-312) in the store of
        hidden2pose_projection's output.  Same flags as ConvModel.forward_fused.  Inference only."""
        if self._wants_grad(body):
            raise RuntimeError("TransformerEnc.forward_fused is inference-only (no gradient): call model.eval() or wrap "
                               "the call in torch.no_grad(); train through model(x), which is differentiable")
        flags = ((_lib.PRE_CHEST_DIFF if dif_encoding else 0) | (_lib.PRE_NORMALIZE if normalize else 0) |
                 (_lib.POST_DENORMALIZE if denormalize else 0) | (_lib.POST_MASK_TAIL if mask_tail else 0))
        return self._run(body, flags, factor, n_frames)


_TencTrainFn = TrainFn   # the name earlier documents and tests' docstrings use
