"""Drop-in mirror of the reference's `TextPoseTransformer` (body2hand/src/models/HandPoseModels.py:181-230),
the text-conditioned body->hand model and the default of the reference's CLIs (run.py:32-36,148-151;
infer_utterance.py:27-28,102-103), on libb2h's gfx950 kernels.

Same constructor `TextPoseTransformer(n_tokens, n_joints, joints_dim, nhead, nhid, nout, n_enc_layers,
n_dec_layers, dropout=0.5)` and the same `state_dict`: the torch.nn containers are built in the reference's order,
so a seeded default init is identical and its checkpoints load as they are.  `model(input_tokens, input_pose)`
with int64 token ids (B, S) and float32 pose (B, T, n_joints, 2) -> float32 (B, T, nout / 2, 2); tokenisation stays
with the caller, as in the reference (traintest.py:105-107).  The geometries are the four the reference's CLIs build:
(n_joints, nout) = (12, 42) (infer_utterance.py:79-80), (8, 42) (run.py:100-101, the trainer's default), (29, 8)
(`--predict right_index`, run.py:92-93) and (21, 24) (`right_3fingers`, :96-97), and any other pairing of those
values (n_joints * joints_dim in {16, 24, 42, 58}, nout in {8, 24, 42}).  The torch containers only hold parameters: the forward runs
through the C ABI (`b2h_tpt_forward`).  Like the reference, the model by default passes no mask (padded token id 0 is
attended like any other id) and never applies its two positional encodings, which exist only as `pe` buffers.

Key-padding masks (not in the reference): `text_lengths` and `frame_lengths`, keywords of
`forward`, `forward_long`, `forward_fused` and `_forward_train`, each a tensor or sequence of shape (B,) or None.  Padding
is a suffix, so torch's src / memory key-padding masks are `text_lengths` (`token_lengths(tokens)`) and its tgt
key-padding mask is `frame_lengths` (the loader's `n_frames`): key j of sequence b is attended iff
j < clamp(length[b], 1, rows).  A length of 0 counts as 1, where torch returns NaN.  Exact fp32 only: with
`set_precision("f16x3")` a length is refused.  A model trained with masks must be run with masks.

Training: in training mode with autograd enabled and a parameter or `input_pose` requiring a gradient,
`model(input_tokens, input_pose)` runs `_native.TrainFn` -- an exact-fp32 HIP forward and backward
(b2h_tpt_train_forward / b2h_tpt_backward, kernel_tpt_train.h) that read the parameters' own storage -- so the
reference's loop body (steps/traintest.py:105-121) runs unchanged with any torch optimizer, at S <= 128 tokens and
T <= 1024 frames (the trainer pads to `--max-frames 200`, run.py:28; beyond 128 frames the decoder's two attentions
run blocked, kernel_train_attn_long.h, or after `model.set_train_kernels("mfma")` on the matrix cores in exact fp32,
kernel_train_attn_mfma.h; after `model.set_train_whole("mfma")` the encoder's self-attention at every T and the
decoder's two attentions up to 128 frames run the whole-matrix fp32 MFMA pair b2h_mw_sdpa / _bwd,
kernel_train_attn_whole_mfma.h).  The dropout keep-masks
are drawn by torch on the model's device (`_draw_dropout_masks`; they follow torch.manual_seed) and handed to the
kernels; after `model.set_dropout_source("native", seed)` libb2h draws them itself, all of a step in one launch
(b2h_dropout_masks, kernel_dropout_masks.h).  Every other call (eval mode or no_grad) runs the inference kernels.

Inference is exact fp32 by default; `model.set_precision("f16x3")` selects the f16 hi + lo split path (three
v_mfma_f32_16x16x32_f16 per product, Q, K, V projected inside the attention kernels), valid while every weight and
activation is below 65504 in magnitude.  S <= 128; in inference `model(tokens, pose)` takes T <= 128, `forward_fused`
and `forward_long` T <= 1024 (the reference's CLIs default to 200 frames), the former with the item transforms.  No path ever falls back to PyTorch ops.
"""
import ctypes
import warnings

import torch
import torch.nn as nn

from . import _lib
from ._native import NativeDropout, NativeModule, TrainFn, TrainRoutes, _aligned, _ptrs
from .transformer_enc import TENC_KERNELS, PositionalEncoding


class TextPoseTransformer(NativeDropout, TrainRoutes, NativeModule, nn.Module):
    """`precision` (not in the reference; keyword only): the constructor accepts only "fp32" = fp32 operands on the
    matrix cores, the default.  `set_precision("f16x3")` switches the inference forward to the f16 hi + lo split
    (fp32-grade results, the same 2e-5 parity bar; needs |weights| and |activations| < 65504, else the forward
    raises) and `set_precision("fp32")` switches back; no reload of the weights.  The constructor itself keeps
    refusing "f16x3" because tests/test_tpt_cpu.py::test_python_side_errors pins that refusal; a later change that
    may touch that test lifts it.  Training is exact fp32 whatever the precision, and takes T <= 1024 frames;
    `set_train_kernels("mfma")` (attribute `train_kernels`, default "valu") moves the decoder's attentions beyond 128
    frames to fp32 MFMA kernels, and `set_train_linear("mfma")` (attribute `train_linear`, default "valu") moves every
    Linear layer of a training step, forward and backward at every length, to fp32 MFMA kernels, and
    `set_train_whole("mfma")` (attribute `train_whole`, default "valu") moves every attention of at most 128 x 128 (the
    encoder's, and up to 128 frames the decoder's two) to the whole-matrix fp32 MFMA pair.  The
    inference route of `model(tokens, pose)` stops at 128 (`forward_long` / `forward_fused` go to 1024)."""

    def __init__(self, n_tokens, n_joints, joints_dim, nhead, nhid, nout, n_enc_layers, n_dec_layers, dropout=0.5, *,
                 precision="fp32"):
        super().__init__()
        if precision != "fp32":
            raise ValueError(f"precision must be 'fp32', got {precision!r}")
        self.precision = precision
        self.train_kernels = "valu"
        self.train_linear = "valu"
        self.train_whole = "valu"
        self.model_type = "Transformer"
        self.src_mask = None
        self.token_pos_encoder = PositionalEncoding(nhid, dropout, max_len=40)
        self.pose_pos_encoder = PositionalEncoding(nhid, dropout, max_len=100)
        with warnings.catch_warnings():  # torch notes that seq-first layers skip its nested-tensor path
            warnings.simplefilter("ignore", UserWarning)
            self.transformer = nn.Transformer(nhid, nhead, n_enc_layers, n_dec_layers, nhid, dropout=dropout)
        self.token_embedding = nn.Embedding(n_tokens, nhid)
        self.hidden2pose_projection = nn.Linear(nhid, nout)
        self.pose2hidden_projection = nn.Linear(n_joints * joints_dim, nhid)
        self.n_tokens = int(n_tokens)
        self.ninp = int(n_joints * joints_dim)
        self.nout = int(nout)
        self._dropout_p = float(dropout)
        self._geom = (self.n_tokens, self.ninp, int(nhead), int(nhid), int(nout), int(n_enc_layers), int(n_dec_layers))

    def set_precision(self, name):
        """Select the inference arithmetic, "fp32" or "f16x3", for later forwards (`forward_fused` included);
        returns self.  Measured at 200 frames: f16x3 is 1.72x fp32 at (4096, 40, 200) and
        1.94x at (64, 40, 200)."""
        if name not in TENC_KERNELS:
            raise ValueError(f"precision must be one of {sorted(TENC_KERNELS)}, got {name!r}")
        self.precision = name
        return self

    def set_train_kernels(self, name):
        """Select the kernels of later training forwards, "valu" (the default) or "mfma"; returns self.  "mfma" runs
        the decoder's two attentions beyond 128 frames, forward and backward, on v_mfma_f32_16x16x4_f32
        (kernel_train_attn_mfma.h): exact fp32 like the default and as deterministic, in another summation order.  Up
        to 128 frames and in the encoder it changes nothing.  A backward runs the route its forward ran, whatever the
        model says by then.  Measurements: DESIGN.md section 17."""
        return self._choose_train_route("train_kernels", "train kernels", name)

    def set_train_linear(self, name):
        """Select the Linear kernels of later training forwards, "valu" (the default) or "mfma"; returns self.  "mfma"
        runs every Linear layer of the step -- Y = X W^T + b, dX = dY W and the slab partials of dW, db, in the encoder
        and the decoder at every length -- on v_mfma_f32_16x16x4_f32 (kernel_train_linear_mfma.h): exact fp32, the
        default's summation order per element, as deterministic.  Independent of `set_train_kernels`; LayerNorm, the
        embedding, the attentions and inference are untouched.  A backward runs the Linears its forward ran, whatever
        the model says by then.  Measurements: DESIGN.md section 19."""
        return self._choose_train_route("train_linear", "train linear", name)

    def set_train_whole(self, name):
        """Select the whole-matrix attention kernels of later training forwards, "valu" (the default) or "mfma";
        returns self.  "mfma" runs every attention of at most 128 x 128 -- the encoder's self-attention (S x S) at
        every T, and up to 128 frames the decoder's self-attention (T x T) and cross-attention (T x S) -- forward and
        backward on v_mfma_f32_16x16x4_f32 (b2h_mw_sdpa / _bwd, kernel_train_attn_whole_mfma.h): exact fp32, y bitwise
        equal to the default's, the gradients in another fixed summation order.  Independent of `set_train_kernels`
        (which keeps the decoder beyond 128 frames) and `set_train_linear`.  A backward runs the kernels its forward
        ran, whatever the model says by then.  Measurements: DESIGN.md section 30."""
        return self._choose_train_route("train_whole", "train whole", name)

    _NAME, _CREATE, _LOAD, _DESTROY = "TextPoseTransformer", "b2h_tpt_create", "b2h_tpt_load_weights", "b2h_tpt_destroy"

    def _tensors(self):
        """The parameters in state_dict order, i.e. the order of b2h_tpt_load_weights (the two pe buffers, which the
        forward never uses, are not among them)."""
        return list(self.parameters())

    def _device(self):
        return self._modules["pose2hidden_projection"]._parameters["weight"].device

    def _create_args(self):
        return self._geom

    def _ensure_handle(self):
        """(library, device): this model's callers have always unpacked the pair."""
        return super()._ensure_handle(), self._device()

    def _wants_grad(self, input_tokens, input_pose):
        """The training path's condition: training mode, autograd on, a parameter or the pose needs a gradient."""
        return (self.training and torch.is_grad_enabled() and
                (input_pose.requires_grad or any(p.requires_grad for p in self._tensors())))

    def _mask_order(self, B, S, T):
        """(key, shape) of every keep-mask in the order of b2h_tpt_train_forward (include/b2h.h)."""
        nhead, nhid, n_enc, n_dec = self._geom[2], self._geom[3], self._geom[5], self._geom[6]
        order = []
        for l in range(n_enc):
            order.append((("enc", l, "attn"), (B, nhead, S, S)))
            order += [(("enc", l, name), (B, S, nhid)) for name in ("drop1", "ff", "drop2")]
        for l in range(n_dec):
            order += [(("dec", l, "self_attn"), (B, nhead, T, T)), (("dec", l, "drop1"), (B, T, nhid)),
                      (("dec", l, "cross_attn"), (B, nhead, T, S)), (("dec", l, "drop2"), (B, T, nhid)),
                      (("dec", l, "ff"), (B, T, nhid)), (("dec", l, "drop3"), (B, T, nhid))]
        return order

    def _draw_dropout_masks(self, B, S, T):
        """The keep-masks of one training forward: uint8, 1 = keep with probability 1 - p, drawn on the model's
        device with torch's generator (so they follow torch.manual_seed), or under `dropout_source` "native" by
        b2h_dropout_masks as views of one allocation (mask number = position; `set_dropout_source`), in either
        case in this fixed order, which is that of
        torch's layers: per encoder layer ("enc", l, name) with name = `attn` (B, 4, S, S), `drop1`, `ff`, `drop2`
        (B, S, 128 each); then per decoder layer ("dec", l, name) with name = `self_attn` (B, 4, T, T), `drop1`
        (B, T, 128), `cross_attn` (B, 4, T, S), `drop2`, `ff`, `drop3` (B, T, 128 each).  An empty dict at p = 0."""
        return self._drawn_masks(self._dropout_p, B, S, T)

    def _check_inputs(self, input_tokens, input_pose):
        if input_pose.dim() != 4 or input_pose.shape[2] * input_pose.shape[3] != self.ninp:
            raise RuntimeError(f"expected input_pose of shape (B, T, {self.ninp // 2}, 2), got {tuple(input_pose.shape)}")
        if input_tokens.dim() != 2:
            raise RuntimeError(f"expected input_tokens of shape (B, S), got {tuple(input_tokens.shape)}")
        if input_tokens.shape[0] != input_pose.shape[0]:
            raise RuntimeError(f"input_tokens has batch size {input_tokens.shape[0]}, input_pose {input_pose.shape[0]}")
        if input_tokens.dtype not in (torch.int64, torch.int32):
            raise RuntimeError(f"expected integer token ids (int64, like nn.Embedding), got {input_tokens.dtype}")
        if input_tokens.device.type == "cpu" and input_tokens.numel():
            # where the ids are host memory the range check costs no synchronisation; ids already on the device
            # are checked by the kernel, which turns their sequence's output into NaN (include/b2h.h)
            lo, hi = int(input_tokens.min()), int(input_tokens.max())
            if lo < 0 or hi >= self.n_tokens:
                raise IndexError("index out of range in self")  # nn.Embedding's message

    def _key_lengths(self, lengths, name, B, dev):
        """A key-length argument as the int64 (B,) tensor on `dev` the entry points read, or None."""
        if lengths is None:
            return None
        t = torch.as_tensor(lengths).detach().to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
        if t.shape != (B,):
            raise RuntimeError(f"expected {name} of shape ({B},), got {tuple(t.shape)}")
        return t

    @staticmethod
    def _check_lengths(B, text_lengths, frame_lengths):
        """The shape refusal of `_key_lengths`, where nothing has been moved to a device yet."""
        for lengths, name in ((text_lengths, "text_lengths"), (frame_lengths, "frame_lengths")):
            if lengths is not None and tuple(torch.as_tensor(lengths).shape) != (B,):
                raise RuntimeError(f"expected {name} of shape ({B},), got {tuple(torch.as_tensor(lengths).shape)}")

    def _forward_train(self, input_tokens, input_pose, masks, text_lengths=None, frame_lengths=None):
        """The differentiable forward (`_native.TrainFn`) with the given keep-masks (`_draw_dropout_masks`) and key
        lengths, which travel to the backward next to the token ids."""
        self._check_inputs(input_tokens, input_pose)
        dev = self._device()
        tok = input_tokens.to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
        x = input_pose.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
        p = self._dropout_p
        masks = self._checked_masks(masks, p, x.device, tok.shape[0], tok.shape[1], x.shape[1])
        tl = self._key_lengths(text_lengths, "text_lengths", tok.shape[0], dev)
        fl = self._key_lengths(frame_lengths, "frame_lengths", tok.shape[0], dev)
        lead = tok if tl is None and fl is None else (tok, tl, fl)
        return TrainFn.apply(self, p, masks, lead, x, *self._tensors())

    # what TrainFn asks of the model: the token ids are an argument of their own; the two routes travel to the backward
    _TRAIN_FNS = ("b2h_tpt_train_bytes", "b2h_tpt_train_forward", "b2h_tpt_backward")
    _TRAIN_FNS_MASKED = ("b2h_tpt_train_bytes", "b2h_tpt_train_forward_masked", "b2h_tpt_backward_masked")
    _TRAIN_LEAD_IS_PARAM = False

    def _train_shapes(self, tok, x):
        B, S, T = tok.shape[0], tok.shape[1], x.shape[1]
        return (B, S, T), (B, T, self.nout // 2, 2), (B, T, self.ninp // 2, 2)

    def _train_head(self, tok, params):
        return _ptrs(params), ctypes.c_void_p(tok.data_ptr())

    def _train_route(self):
        return (("b2h_tpt_set_train_kernel", _lib.TRAIN_KERNELS[self.train_kernels]),
                ("b2h_tpt_set_train_linear", _lib.TRAIN_KERNELS[self.train_linear]),
                ("b2h_tpt_set_train_whole", _lib.TRAIN_KERNELS[self.train_whole]))

    def forward(self, input_tokens, input_pose, text_lengths=None, frame_lengths=None):
        train = self._wants_grad(input_tokens, input_pose) and self._device().type == "cuda"
        if not train and self.training and self._dropout_p > 0.0:
            raise RuntimeError("hand_pose_sl_amd.TextPoseTransformer: this call runs the inference kernels (autograd is "
                               "off, nothing requires a gradient, or the parameters are not on a GPU), which are "
                               f"inference-only: in training mode the reference applies dropout (p = {self._dropout_p}) "
                               "and this path has none; call model.eval()")
        self._check_inputs(input_tokens, input_pose)
        if train:
            # the lengths are validated before the masks are drawn, so a refusal does not advance a generator
            self._check_lengths(input_tokens.shape[0], text_lengths, frame_lengths)
            return self._forward_train(input_tokens, input_pose, self._draw_dropout_masks(
                input_tokens.shape[0], input_tokens.shape[1], input_pose.shape[1]), text_lengths, frame_lengths)
        if text_lengths is None and frame_lengths is None:
            return self._run(input_tokens, input_pose, None)
        return self._run(input_tokens, input_pose, (0, 1.0, None), text_lengths, frame_lengths, max_frames=128)

    def _run(self, input_tokens, input_pose, fused, text_lengths=None, frame_lengths=None, max_frames=None):
        """The inference kernels: b2h_tpt_forward, or b2h_tpt_forward_fused with fused = (flags, factor, n_frames), or
        with a key length b2h_tpt_forward_masked (`max_frames`: the limit of `forward`, which that entry point does not
        have)."""
        masked = text_lengths is not None or frame_lengths is not None
        if masked:
            self._check_lengths(input_tokens.shape[0], text_lengths, frame_lengths)
            if self.precision == "f16x3":
                # b2h_tpt_forward_masked's own refusal (B2H_ERR_UNSUPPORTED), raised here before any launch
                raise RuntimeError("libb2h: B2H_TENC_F16X3 takes no key lengths (text_lengths / frame_lengths): its attention "
                                   "kernels attend to every row; select exact fp32 with b2h_tpt_set_kernel(fp32), i.e. "
                                   "model.set_precision(\"fp32\") (status -6)")
            if max_frames is not None and input_pose.dim() == 4 and input_pose.shape[1] > max_frames:
                raise RuntimeError("libb2h: TextPoseTransformer: S and T are limited to 128 in model(tokens, pose); "
                                   "forward_long and forward_fused take T <= 1024 (status -2)")
        lib, dev = self._ensure_handle()
        tok = input_tokens.to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
        # a composite model's rows are 168 or 232 bytes: pose[1:] of an odd T starts 8 bytes off the 16-byte grid
        x = _aligned(input_pose.detach().to(device=dev, dtype=torch.float32, non_blocking=True).contiguous())
        B, S, T = tok.shape[0], tok.shape[1], x.shape[1]
        nf = None
        if fused is not None and fused[2] is not None:
            nf = torch.as_tensor(fused[2]).to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
            if nf.shape != (B,):
                raise RuntimeError(f"expected n_frames of shape ({B},), got {tuple(nf.shape)}")
        y = torch.empty((B, T, self.nout // 2, 2), dtype=torch.float32, device=dev)
        need = lib.b2h_tpt_workspace_bytes(self._handle, B, S, T)
        ws = self._grown_workspace(need, dev)
        args = (ctypes.c_void_p(ws.data_ptr()), ws.numel())
        with _lib.on_device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.b2h_tpt_set_kernel(self._handle, TENC_KERNELS[self.precision]))
            head = (self._handle, ctypes.c_void_p(tok.data_ptr()), ctypes.c_void_p(x.data_ptr()),
                    ctypes.c_void_p(y.data_ptr()), B, S, T)
            if fused is None:
                _lib.check(lib.b2h_tpt_forward(*head, *args, ctypes.c_void_p(st)))
            elif masked:
                tl = self._key_lengths(text_lengths, "text_lengths", B, dev)
                fl = self._key_lengths(frame_lengths, "frame_lengths", B, dev)
                _lib.check(lib.b2h_tpt_forward_masked(*head, fused[0], fused[1],
                                                      ctypes.c_void_p(nf.data_ptr()) if nf is not None else None,
                                                      ctypes.c_void_p(tl.data_ptr()) if tl is not None else None,
                                                      ctypes.c_void_p(fl.data_ptr()) if fl is not None else None, *args,
                                                      ctypes.c_void_p(st)))
            else:
                _lib.check(lib.b2h_tpt_forward_fused(*head, fused[0], fused[1],
                                                     ctypes.c_void_p(nf.data_ptr()) if nf is not None else None, *args,
                                                     ctypes.c_void_p(st)))
        return y

    def forward_long(self, input_tokens, input_pose, text_lengths=None, frame_lengths=None):
        """`model(input_tokens, input_pose)` in inference for 1 <= T <= 1024 frames, in any geometry: the long path on
        rows that are already the model's input (for a composite model the (B, T, 21 | 29, 2) rows of `build_item` or of
        the reference's dataset), no transform on either side.  Equal to `model(tokens, pose)` bit for bit at T <= 128."""
        if self._wants_grad(input_tokens, input_pose) or (self.training and self._dropout_p > 0.0):
            raise RuntimeError("TextPoseTransformer.forward_long is inference-only (no gradient, no dropout): call "
                               "model.eval() or wrap the call in torch.no_grad(); train through model(tokens, pose)")
        self._check_inputs(input_tokens, input_pose)
        return self._run(input_tokens, input_pose, (0, 1.0, None), text_lengths, frame_lengths)

    def build_item(self, body, right_hand, dif_encoding=True, normalize=True, factor=1280.0):
        """The (B, T, n_joints, 2) input rows of a composite model (`--predict right_index`: 29 joints, `right_3fingers`:
        21) from raw body (B, T, 12, 2) and right-hand (B, T, 21, 2) keypoints: WristDifference, ChestDifference,
        / factor and the Build*Item concatenation of steps/utils.py:194-259 in run.py:85-104's order, one HIP kernel
        (b2h_tpt_build_item).  The predict mode follows from the model's input width."""
        predict = _lib.PREDICT_NINP.get(self.ninp)
        if predict is None:
            raise ValueError(f"build_item is for the composite inputs (n_joints 21 or 29); this model takes {self.ninp // 2} "
                             "body joints")
        if body.dim() != 4 or tuple(body.shape[2:]) != (12, 2):
            raise RuntimeError(f"expected body of shape (B, T, 12, 2), got {tuple(body.shape)}")
        if right_hand.dim() != 4 or tuple(right_hand.shape) != tuple(body.shape[:2]) + (21, 2):
            raise RuntimeError(f"expected right_hand of shape {tuple(body.shape[:2]) + (21, 2)}, got {tuple(right_hand.shape)}")
        lib, dev = self._ensure_handle()
        b = _aligned(body.detach().to(device=dev, dtype=torch.float32, non_blocking=True).contiguous())
        h = _aligned(right_hand.detach().to(device=dev, dtype=torch.float32, non_blocking=True).contiguous())
        B, T = b.shape[0], b.shape[1]
        item = torch.empty((B, T, self.ninp // 2, 2), dtype=torch.float32, device=dev)
        flags = (_lib.PRE_CHEST_DIFF if dif_encoding else 0) | (_lib.PRE_NORMALIZE if normalize else 0)
        with _lib.on_device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.b2h_tpt_build_item(ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(h.data_ptr()),
                                              ctypes.c_void_p(item.data_ptr()), B, T, _lib.PREDICT[predict], flags,
                                              float(factor), ctypes.c_void_p(st)))
        return item

    def forward_fused(self, input_tokens, body, n_frames=None, dif_encoding=True, normalize=True, denormalize=True,
                      mask_tail=False, factor=1280.0, right_hand=None, text_lengths=None, frame_lengths=None):
        """Token ids and raw-pixel body keypoints in, pixel-space hand keypoints out, with the item transforms inside
        the model's own kernels (b2h_tpt_forward_fused): ChestDifference + /factor (steps/utils.py:180-210) on the pose
        rows as they enter pose2hidden_projection -> the model -> x factor (traintest.py:270-271) and the optional
        tail mask (utils.py:309-312) in the store of hidden2pose_projection's output.  Same keywords and defaults as
        TransformerEnc.forward_fused; honours set_precision.  Inference only.

        This is also the long path: 1 <= T <= 1024 frames (S <= 128 tokens), which is what the reference's own CLIs
        feed at their default `--max-frames 200`.  Beyond 128 frames the decoder's attention walks the keys in blocks
        with an online softmax.  With every transform off and T <= 128 the result equals `model(tokens, pose)` bit for
        bit.  `model(tokens, pose)` itself keeps refusing T > 128 because
        tests/test_tpt_gpu.py::test_errors_and_weight_replacement pins that refusal; a later change that may touch
        that test should route `forward` to this path.

        `right_hand` (B, T, 21, 2), raw pixels: required exactly when the model takes a composite input (n_joints 21 or
        29, `--predict right_3fingers` / `right_index`).  `body` is then the 12 body joints, the input rows are made by
        `build_item` (where `dif_encoding` and `normalize` then apply) and the model runs with its own pre-transforms
        off; the output side is as for the body-only models.

        `text_lengths`, `frame_lengths`: the key-padding masks (module docstring), through b2h_tpt_forward_masked;
        `n_frames` stays the tail mask's own argument, usually the same tensor as `frame_lengths`."""
        composite = self.ninp in _lib.PREDICT_NINP
        if composite != (right_hand is not None):
            raise ValueError(f"right_hand must be given exactly when the model takes a composite input (n_joints 21 or 29); "
                             f"this model takes {self.ninp // 2} joints")
        if self._wants_grad(input_tokens, body):
            raise RuntimeError("TextPoseTransformer.forward_fused is inference-only (no gradient): call model.eval() or "
                               "wrap the call in torch.no_grad(); train through model(tokens, pose)")
        if self.training and self._dropout_p > 0.0:
            raise RuntimeError("hand_pose_sl_amd.TextPoseTransformer.forward_fused is inference-only: in training mode "
                               f"the reference applies dropout (p = {self._dropout_p}) and this path has none; call "
                               "model.eval()")
        if mask_tail and n_frames is None:
            raise ValueError("mask_tail=True needs n_frames")
        if composite:
            body = self.build_item(body, right_hand, dif_encoding, normalize, factor)
            dif_encoding = normalize = False
        self._check_inputs(input_tokens, body)
        flags = ((_lib.PRE_CHEST_DIFF if dif_encoding else 0) | (_lib.PRE_NORMALIZE if normalize else 0) |
                 (_lib.POST_DENORMALIZE if denormalize else 0) | (_lib.POST_MASK_TAIL if mask_tail else 0))
        return self._run(input_tokens, body, (flags, float(factor), n_frames if mask_tail else None), text_lengths,
                         frame_lengths)


_TptTrainFn = TrainFn   # the name earlier documents and tests' docstrings use
