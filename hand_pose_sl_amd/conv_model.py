"""Drop-in mirror of the reference's `ConvModel` (body2hand/src/models/
HandPoseModels.py:17-64) whose forward runs on libb2h's gfx950 kernels.

Same constructor `ConvModel(conv_channels, activation, pos_emb)`, same
`state_dict` keys `conv{1..4}.{weight,bias}` (so `load_state_dict(torch.load(p))`
from infer_utterance.py:109 works), same call `model(x)` with x float32
(B, T, 12, 2) -> float32 (B, T, 21, 2).  The `nn.Conv1d` children are parameter
containers only -- constructing them in the reference's order also makes a
seeded default init identical to the reference's -- their forward is never
called: the four layers run fused in one HIP kernel through the C ABI.

Training: in training mode with autograd enabled and a parameter or the input requiring
a gradient, `model(x)` runs `_ConvTrainFn` -- an exact-fp32 HIP forward and a HIP backward
(b2h_train_forward / b2h_backward) that read the parameters' own storage -- so the reference's
loop body (steps/traintest.py:87-121) runs unchanged with any torch optimizer.  Every other call
(eval mode or no_grad) runs the inference kernels selected by `precision`.  No path ever falls
back to PyTorch ops.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._native import NativeModule, _aligned, _ptrs


class LinearPositionalEmbedding(nn.Module):
    """Marker for `pos_emb=True` (HandPoseModels.py:66-84): channel t/100, T == 100.
    The embedding itself is generated inside the kernel."""

    def __init__(self, max_len=100):
        super().__init__()
        self.max_len = max_len


PRECISION_NOTES = """precision (which hand-written kernel computes the four layers; max-abs error vs the reference's
fp32 CPU forward, measured in tests/test_gpu_parity.py::test_error_vs_input_scale and tools/conv_precision_error.py):
  "fp32"   exact fp32 on the matrix cores, <= 1.2e-7                  2.8 G frames/s   (default: the reference's arithmetic)
  "f16x3"  fp32-grade: f16 hi+lo split operands, <= 1.2e-7            8.5 G frames/s   (needs |weights| < 65504)
  "f16"    f16 operands, fp32 accumulate: 5e-5 on normalised keypoints, 1.2e-4 at N(0,1), 6e-4 at N(0,4^2);
           meets north_star's <= 1e-3 gate up to |x| ~ 20          18 G frames/s
  "bf16"   bf16 operands, fp32 accumulate: 3.7-5.0e-4 on normalised keypoints (|x| <~ 1), 1.05e-3 at N(0,1) --
           i.e. it meets the <= 1e-3 gate only on inputs scaled like keypoints / 1280; `f16` runs at the SAME
           speed and holds the gate on any such input, so prefer it unless bf16's exponent range is needed
           (activations beyond 65504)                               18 G frames/s
training (model.train(), autograd on, a parameter or the input requires grad): always exact fp32 on the
vector ALU (b2h_train_forward / b2h_backward), whatever `precision` says; gradients as accurate as the
reference's own fp32 CPU training (tests/test_train_gpu.py)."""


class ConvModel(NativeModule, nn.Module):
    __doc__ = """ConvModel(conv_channels, activation, pos_emb, precision="fp32") -- the reference's constructor
    (HandPoseModels.py:18-37) plus the kernel choice.\n\n""" + PRECISION_NOTES

    def __init__(self, conv_channels, activation, pos_emb, precision="fp32"):
        super().__init__()
        if pos_emb:
            self.pos_emb = LinearPositionalEmbedding(max_len=100)
            self.conv1 = nn.Conv1d(12 * 2 + 1, conv_channels, kernel_size=5, padding=2)
        else:
            self.pos_emb = None
            self.conv1 = nn.Conv1d(12 * 2, conv_channels, kernel_size=5, padding=2)
        self.conv2 = nn.Conv1d(conv_channels, conv_channels, kernel_size=5, padding=2)
        self.conv3 = nn.Conv1d(conv_channels, conv_channels, kernel_size=5, padding=2)
        self.conv4 = nn.Conv1d(conv_channels, 2 * 21, kernel_size=5, padding=2)
        if activation != "ReLU":
            raise ValueError()  # HandPoseModels.py:34-37
        self.activation = nn.ReLU()
        self.conv_channels = int(conv_channels)
        self.precision = precision
        if precision not in _lib.KERNELS:
            raise ValueError(f"precision must be one of {sorted(_lib.KERNELS)}")
    # ---- native handle (NativeModule) -----------------------------------------------------
    _NAME, _CREATE, _LOAD, _DESTROY = "ConvModel", "b2h_create", "b2h_load_weights", "b2h_destroy"

    def _params(self):
        # through the module dictionaries: nn.Module.__getattr__ costs ~0.4 us per hop, and this
        # runs on every forward (weight-replacement check) -- 8 us of a 15 us small-batch call
        mods = self._modules
        out = []
        for name in ("conv1", "conv2", "conv3", "conv4"):
            p = mods[name]._parameters
            out.append(p["weight"])
            out.append(p["bias"])
        return out

    _tensors = _params

    def _device(self):
        return self._modules["conv1"]._parameters["weight"].device

    def _create_args(self):
        return self.conv_channels, b"ReLU", int(self.pos_emb is not None)

    def _load_args(self, ps):
        return [ctypes.c_void_p(p.data_ptr()) for p in ps] + [1]

    # ---- forward -------------------------------------------------------------
    def kernel_name(self, precision=None):
        lib = self._ensure_handle()
        return lib.b2h_kernel_name(self._handle, _lib.KERNELS[precision or self.precision]).decode()

    def _wants_grad(self, inp):
        """The training path's condition: training mode, autograd on, a parameter or the input needs a gradient."""
        return (self.training and torch.is_grad_enabled() and
                (inp.requires_grad or any(p.requires_grad for p in self._params())))

    def _check_input(self, inp):
        if inp.dim() != 4 or inp.shape[2] != 12 or inp.shape[3] != 2:
            raise RuntimeError(f"expected input of shape (B, T, 12, 2), got {tuple(inp.shape)}")
        dev = self._device()
        # traintest.py:354-358 passes batch["body_kp"], which the loop never moved to the device
        x = inp.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
        return x

    def forward(self, inp):
        if self._wants_grad(inp):
            x = self._check_input(inp)
            return _ConvTrainFn.apply(self, x, *self._params())
        lib = self._ensure_handle()
        x = _aligned(self._check_input(inp))     # b2h_forward takes x on the 16-byte grid
        B, T = x.shape[0], x.shape[1]
        y = torch.empty((B, T, 21, 2), dtype=torch.float32, device=x.device)
        with _lib.on_device(x.device):
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(lib.b2h_forward(self._handle, ctypes.c_void_p(x.data_ptr()),
                                       ctypes.c_void_p(y.data_ptr()), B, T,
                                       _lib.KERNELS[self.precision], ctypes.c_void_p(st)))
        return y

    def forward_into(self, x, y, precision=None):
        """Launch on the current stream with caller-owned device buffers: x (B,T,12,2) -> y (B,T,21,2),
        both contiguous float32 on the model's device.  No allocation, no synchronisation: the
        building block of stream pipelines (hand_pose_sl_amd.stream.HostPipeline) and HIP graphs."""
        lib = self._ensure_handle()
        if x.dim() != 4 or x.shape[2:] != (12, 2) or y.shape != (x.shape[0], x.shape[1], 21, 2):
            raise RuntimeError(f"expected x (B,T,12,2) and y (B,T,21,2), got {tuple(x.shape)} and {tuple(y.shape)}")
        dev = self._device()
        for t in (x, y):
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("forward_into needs contiguous float32 tensors on the model's device")
            if t.data_ptr() % 16:
                # caller-owned buffers cannot be cloned here; model(x) copies such an input instead
                raise RuntimeError("forward_into needs x and y to start on a 16-byte boundary (data_ptr() % 16 == 0): the "
                                   f"kernels move 16-byte vectors; got an offset of {t.data_ptr() % 16} bytes (a "
                                   "contiguous view into a larger buffer may start anywhere)")
        with _lib.on_device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.b2h_forward(self._handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                       x.shape[0], x.shape[1], _lib.KERNELS[precision or self.precision],
                                       ctypes.c_void_p(st)))
        return y

    def forward_fused(self, body, n_frames=None, dif_encoding=True, normalize=True, denormalize=True,
                      mask_tail=False, factor=1280.0):
        """Raw-pixel body keypoints in, pixel-space hand keypoints out, in ONE kernel:
        ChestDifference + /factor (steps/utils.py:180-210) -> four conv layers ->
        x factor (traintest.py:387-388) -> optional tail mask (utils.py:309-312).  Inference only."""
        if self._wants_grad(body):
            raise RuntimeError("ConvModel.forward_fused is inference-only (no gradient): call model.eval() or wrap the "
                               "call in torch.no_grad(); train through model(x), which is differentiable")
        lib = self._ensure_handle()
        x = _aligned(self._check_input(body))
        B, T = x.shape[0], x.shape[1]
        flags = ((_lib.PRE_CHEST_DIFF if dif_encoding else 0) | (_lib.PRE_NORMALIZE if normalize else 0) |
                 (_lib.POST_DENORMALIZE if denormalize else 0) | (_lib.POST_MASK_TAIL if mask_tail else 0))
        nf = None
        if mask_tail:
            if n_frames is None:
                raise ValueError("mask_tail needs n_frames")
            nf = torch.as_tensor(n_frames).to(device=x.device, dtype=torch.int64).contiguous()
            if nf.shape != (B,):
                raise RuntimeError(f"n_frames must have shape ({B},)")
        y = torch.empty((B, T, 21, 2), dtype=torch.float32, device=x.device)
        with _lib.on_device(x.device):
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(lib.b2h_forward_fused(self._handle, ctypes.c_void_p(x.data_ptr()),
                                             ctypes.c_void_p(y.data_ptr()), B, T, flags, float(factor),
                                             ctypes.c_void_p(nf.data_ptr()) if nf is not None else None,
                                             _lib.KERNELS[self.precision], ctypes.c_void_p(st)))
        return y

    def time_forward(self, x, y, iters, precision=None):
        """Average ms per launch over `iters` back-to-back launches, HIP events on
        the launch stream (b2h_time_forward)."""
        lib = self._ensure_handle()
        ms = ctypes.c_float()
        with _lib.on_device(x.device):
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(lib.b2h_time_forward(self._handle, ctypes.c_void_p(x.data_ptr()),
                                            ctypes.c_void_p(y.data_ptr()), x.shape[0], x.shape[1],
                                            _lib.KERNELS[precision or self.precision], int(iters),
                                            ctypes.c_void_p(st), ctypes.byref(ms)))
        return ms.value


class _ConvTrainFn(torch.autograd.Function):
    """y = ConvModel(x) with its gradient: b2h_train_forward / b2h_backward (exact fp32, kernel_train.h).
    The parameters go in as themselves (their own data_ptr, saved for backward, so autograd's version check
    catches an in-place edit between forward and backward); nothing else is saved, the backward recomputes."""

    @staticmethod
    def forward(ctx, model, x, *params):
        for p in params:
            if p.device != x.device or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("training needs contiguous float32 parameters on the input's device")
        lib, dev = model._ensure_created()
        x = _aligned(x)
        B, T = x.shape[0], x.shape[1]
        y = torch.empty((B, T, 21, 2), dtype=torch.float32, device=x.device)
        with _lib.on_device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.b2h_train_forward(model._handle, _ptrs(params), ctypes.c_void_p(x.data_ptr()),
                                             ctypes.c_void_p(y.data_ptr()), B, T, ctypes.c_void_p(st)))
        ctx.model = model
        ctx.save_for_backward(x, *params)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, *params = ctx.saved_tensors
        model = ctx.model
        need_dx = ctx.needs_input_grad[1]
        B, T = x.shape[0], x.shape[1]
        if B == 0:
            grads = [torch.zeros_like(p) for p in params]
            dx = torch.zeros_like(x) if need_dx else None
        else:
            lib, dev = model._ensure_created()
            dy = _aligned(dy.to(torch.float32).contiguous())   # autograd may hand over an expanded / CopySlices gradient
            grads = [torch.empty_like(p) for p in params]
            dx = torch.empty_like(x) if need_dx else None
            nbytes = lib.b2h_backward_workspace_bytes(model._handle, B, T)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
            with _lib.on_device(dev):
                st = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(lib.b2h_backward(model._handle, _ptrs(params), ctypes.c_void_p(x.data_ptr()),
                                            ctypes.c_void_p(dy.data_ptr()),
                                            ctypes.c_void_p(dx.data_ptr()) if dx is not None else None,
                                            _ptrs(grads), B, T, ctypes.c_void_p(ws.data_ptr()), nbytes,
                                            ctypes.c_void_p(st)))
        return (None, dx) + tuple(g if ctx.needs_input_grad[2 + i] else None for i, g in enumerate(grads))


def target_transform(body, hand, dif_encoding=True, normalize=True, factor=1280.0):
    """item["target_kp"]: (hand - body[:, 4]) / factor (steps/utils.py:194-201,180-190)."""
    lib = _lib.load()
    if body.device.type != "cuda":
        raise RuntimeError("target_transform runs on the GPU only")
    body = body.to(torch.float32).contiguous()
    hand = hand.to(device=body.device, dtype=torch.float32).contiguous()
    B, T = body.shape[0], body.shape[1]
    out = torch.empty_like(hand)
    flags = (1 if dif_encoding else 0) | (2 if normalize else 0)
    with _lib.on_device(body.device):
        st = torch.cuda.current_stream(body.device).cuda_stream
        _lib.check(lib.b2h_target_transform(ctypes.c_void_p(body.data_ptr()), ctypes.c_void_p(hand.data_ptr()),
                                            ctypes.c_void_p(out.data_ptr()), B, T, flags, float(factor),
                                            ctypes.c_void_p(st)))
    return out
