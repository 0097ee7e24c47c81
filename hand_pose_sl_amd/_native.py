"""The life cycle of the libb2h model handle behind a torch module, shared by ConvModel, TransformerEnc and
TextPoseTransformer: created on the parameters' device, re-created when that device (or whatever else the
handle was made for) changes, its weights repacked when a parameter is replaced or edited in place, destroyed
with the module; plus the workspace that only grows and the two pointer helpers of the training paths, the
source of the two transformers' dropout masks (`NativeDropout`) and their one autograd Function (`TrainFn`).
"""
import ctypes
import math

import torch

from . import _lib


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _aligned(t):
    """The kernels' 16-byte vector accesses: a contiguous slice of a larger batch may start anywhere."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


DROPOUT_SOURCES = ("torch", "native")


class NativeDropout:
    """Mixin of the two transformers: where the keep-masks of a training forward come from.  "torch" (the default)
    draws them with torch's generator; "native" with libb2h's own counter-based generator (b2h_dropout_masks,
    kernel_dropout_masks.h): one launch and one allocation per step, reproducible from (seed, step) alone."""

    dropout_source = "torch"
    _drop_seed = 0
    _drop_step = None     # one-element int64 tensor on the model's device: the step word the kernel reads

    def set_dropout_source(self, name, seed=None):
        """Select the source of later training forwards' dropout masks, "torch" (the default) or "native"; returns
        self.  "native" draws all masks of a step with one b2h_dropout_masks launch into one uint8 allocation:
        Philox4x32-10 keyed by `seed` (torch.initial_seed() when None) with the step count in the counter, so a run
        is reproducible from (seed, number of draws so far) and torch's generator is never touched.  The step count is
        a device word advanced by a stream-ordered op after every draw, so a captured step draws fresh masks on
        every replay.  Selecting "native" again restarts the count at 0.  The masks' order, shapes, dtype and meaning
        are those of "torch", their bits are not.  Measurements: DESIGN.md section 20."""
        if name not in DROPOUT_SOURCES:
            raise ValueError(f"dropout source must be one of {list(DROPOUT_SOURCES)}, got {name!r}")
        d = self.__dict__
        d["dropout_source"] = name
        if name == "native":
            d["_drop_seed"] = int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
            d["_drop_step"] = None      # made on the model's device here if it is a GPU already, else at the first draw
            if self._device().type == "cuda":
                self._drop_step_on(self._device())
        return self

    def _drop_step_on(self, dev):
        step = self.__dict__.get("_drop_step")
        if step is None:
            step = torch.zeros(1, dtype=torch.int64, device=dev)
        elif step.device != dev:
            step = step.to(dev)
        self.__dict__["_drop_step"] = step
        return step

    def _native_dropout_masks(self, order, p):
        """{key: mask} for the (key, shape) list `order`: views at 16-byte-aligned offsets of one uint8 allocation,
        mask number = position in `order`, filled by one b2h_dropout_masks call on the current stream that reads
        the step word, which a stream-ordered add then advances."""
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError(f"hand_pose_sl_amd.{self._NAME}: the native dropout source runs on an MI355X only")
        lib = _lib.load()
        sizes = [math.prod(shape) for _, shape in order]
        offsets, total = [], 0
        for n in sizes:
            offsets.append(total)
            total += (n + 15) // 16 * 16
        buf = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        masks = {key: buf[o:o + n].view(shape) for (key, shape), o, n in zip(order, offsets, sizes)}
        step = self._drop_step_on(dev)
        with _lib.on_device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.b2h_dropout_masks((ctypes.c_void_p * len(order))(*[base + o for o in offsets]),
                                             (ctypes.c_int64 * len(order))(*sizes), len(order), 0, p, self._drop_seed, 0,
                                             ctypes.c_void_p(step.data_ptr()), ctypes.c_void_p(st)))
            step.add_(1)
        return masks

    def _drawn_masks(self, p, *dims):
        """{key: mask} over `_mask_order(*dims)` from the selected source, drawn in that order; empty at p = 0."""
        if p == 0.0:
            return {}
        order = self._mask_order(*dims)
        if self.dropout_source == "native":
            return self._native_dropout_masks(order, p)
        dev = self._device()
        return {key: (torch.rand(shape, device=dev) >= p).to(torch.uint8) for key, shape in order}

    def _checked_masks(self, masks, p, dev, *dims):
        """The given {key: mask} as the list a training entry point takes (`_mask_order(*dims)`), each one validated."""
        if (p > 0.0) != bool(masks):
            raise ValueError("masks must be given exactly when the dropout probability is > 0")
        order = self._mask_order(*dims) if masks else []
        for key, shape in order:
            m = masks[key]
            if m.shape != shape or m.dtype != torch.uint8 or m.device != dev or not m.is_contiguous():
                raise RuntimeError(f"mask {key}: expected a contiguous uint8 tensor of shape {shape} on {dev}")
        return [masks[k] for k, _ in order]


class TrainRoutes:
    """Mixin of the two transformers: the two opt-in switches of a training step, `train_kernels` (the attentions) and
    `train_linear` (the Linear layers), each one of `_lib.TRAIN_KERNELS`, "valu" by default; TextPoseTransformer adds a
    third of the same kind, `train_whole` (its attentions of at most 128 x 128).  The models' setters validate through
    `_choose_train_route`; `_train_route()` hands the values to TrainFn."""

    train_kernels = "valu"
    train_linear = "valu"

    def _choose_train_route(self, attr, what, name):
        """self.<attr> = name if it is one of `_lib.TRAIN_KERNELS`, else ValueError and nothing changes; returns self."""
        if name not in _lib.TRAIN_KERNELS:
            raise ValueError(f"{what} must be one of {sorted(_lib.TRAIN_KERNELS)}, got {name!r}")
        setattr(self, attr, name)
        return self


class TrainFn(torch.autograd.Function):
    """y = model(lead, x) of a transformer in training mode with its gradient, through the model's b2h_*_train_forward
    / b2h_*_backward (exact fp32): `apply(model, p, masks, lead, x, *params)`.  `lead` is the model's leading tensor
    without a gradient: TransformerEnc's `pe` or TextPoseTransformer's token ids.  The parameters go in as themselves (their own data_ptr, saved for backward, so autograd's version check
    catches an in-place edit between forward and backward).  The context keeps the saved-activation buffer, `lead` and
    the masks alive; the backward needs neither x nor y (the reference's loop overwrites the prediction's tail in place
    before the loss).  The forward sets the handle to the model's route and records it, the backward sets it from
    that record: a backward runs the kernels its forward ran, whatever the model says by then.

    The model supplies what differs:
        _TRAIN_FNS                  the names of its train_bytes, train_forward and backward entry points
        _TRAIN_LEAD_IS_PARAM        whether `lead` travels in the parameter array and is checked like a parameter
                                    (`pe`), or is an argument of its own that only has to be aligned (the token ids)
        _train_shapes(lead, x)      the batch as the entry points take it, (B, T) or (B, S, T); y's shape; dx's shape
        _train_head(lead, params)   the entry points' arguments between the handle and x (forward) / the masks (backward)
        _train_route()              (setter entry point, value) pairs that select the kernels of a forward

    Key lengths (TextPoseTransformer's padding masks): `lead` may be a tuple (token ids, text_lengths, frame_lengths),
    each length an int64 (B,) tensor on the device or None.  They are not differentiable; the context carries them
    to the backward next to the token ids, and both passes then call the model's `_TRAIN_FNS_MASKED` pair, which
    takes the two arrays between the batch dimensions and the stream.  A bare tensor makes the calls it always made."""

    @staticmethod
    def _length_args(lengths):
        return tuple(ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in lengths)

    @staticmethod
    def _set_route(lib, model, route):
        for setter, value in route:
            _lib.check(getattr(lib, setter)(model._handle, value))

    @staticmethod
    def forward(ctx, model, p, masks, lead, x, *params):
        for t in ((lead,) if model._TRAIN_LEAD_IS_PARAM else ()) + params:
            if t.device != x.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("training needs contiguous float32 parameters on the input's device")
        lengths = ()
        if isinstance(lead, tuple):
            lead, *lengths = lead
        fns = model._TRAIN_FNS_MASKED if lengths else model._TRAIN_FNS
        lib, dev = model._ensure_created()
        x = _aligned(x)
        if not model._TRAIN_LEAD_IS_PARAM:
            lead = _aligned(lead)
        dims, yshape, xshape = model._train_shapes(lead, x)
        y = torch.empty(yshape, dtype=torch.float32, device=x.device)
        nbytes = getattr(lib, fns[0])(model._handle, *dims, 0)
        saved = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=x.device)
        route = model._train_route()
        with _lib.on_device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            TrainFn._set_route(lib, model, route)
            _lib.check(getattr(lib, fns[1])(
                model._handle, *model._train_head(lead, params), ctypes.c_void_p(x.data_ptr()),
                _ptrs(masks) if masks else None, p, ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(saved.data_ptr()), nbytes,
                *dims, *TrainFn._length_args(lengths), ctypes.c_void_p(st)))
        ctx.model, ctx.p, ctx.masks, ctx.dims, ctx.xshape, ctx.route = model, p, masks, dims, xshape, route
        ctx.fns, ctx.lengths = fns, tuple(lengths)
        ctx.save_for_backward(saved, lead, *params)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        saved, lead, *params = ctx.saved_tensors
        model, masks, dims = ctx.model, ctx.masks, ctx.dims
        need_dx = ctx.needs_input_grad[4]
        dev = saved.device
        if dims[0] == 0:
            grads = [torch.zeros_like(t) for t in params]
            dx = torch.zeros(ctx.xshape, dtype=torch.float32, device=dev) if need_dx else None
        else:
            lib, dev = model._ensure_created()
            dy = _aligned(dy.to(torch.float32).contiguous())   # autograd may hand over an expanded / CopySlices gradient
            grads = [torch.empty_like(t) for t in params]
            dx = torch.empty(ctx.xshape, dtype=torch.float32, device=dev) if need_dx else None
            nbytes = getattr(lib, ctx.fns[0])(model._handle, *dims, 1)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            with _lib.on_device(dev):
                st = torch.cuda.current_stream(dev).cuda_stream
                TrainFn._set_route(lib, model, ctx.route)
                _lib.check(getattr(lib, ctx.fns[2])(
                    model._handle, *model._train_head(lead, params), _ptrs(masks) if masks else None, ctx.p,
                    ctypes.c_void_p(dy.data_ptr()), ctypes.c_void_p(saved.data_ptr()), saved.numel(),
                    ctypes.c_void_p(dx.data_ptr()) if dx is not None else None, _ptrs(grads), ctypes.c_void_p(ws.data_ptr()),
                    nbytes, *dims, *TrainFn._length_args(ctx.lengths), ctypes.c_void_p(st)))
        return (None, None, None, None, dx) + tuple(g if ctx.needs_input_grad[5 + i] else None for i, g in enumerate(grads))


class NativeModule:
    """Mixin in front of nn.Module.  A model names its product class and its three entry points, and provides
        _device()        the device of its parameters
        _create_args()   the arguments of `_CREATE` before the handle pointer
        _tensors()       the tensors `_LOAD` packs, in its order
    and may override `_handle_key(dev)` (what one handle is made for) and `_load_args(ps)`.

    The state lives in the instance `__dict__` and is written there directly: nn.Module.__setattr__ would cost
    microseconds on the call path.  The class attributes are the values before the first use."""

    _NAME = _CREATE = _LOAD = _DESTROY = None
    _handle = None        # ctypes.c_void_p of the native model
    _made_key = None      # _handle_key(dev) the handle was created for
    _packed_key = None    # _made_key + (data_ptr, _version) of every tensor the handle's packed weights came from
    _workspace = None

    def _handle_key(self, dev):
        return (dev.index,)

    def _load_args(self, ps):
        return _ptrs(ps), len(ps), 1

    def _ensure_created(self):
        """The native model on the parameters' device, without packed weights (all a training path needs)."""
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError(f"hand_pose_sl_amd.{self._NAME} runs on an MI355X only: call model.to('cuda') "
                               "first (there is no CPU path in the product)")
        lib = _lib.load()
        d = self.__dict__
        made = self._handle_key(dev)
        if d.get("_handle") is None or d.get("_made_key") != made:
            self._free()
            with torch.cuda.device(dev):
                h = ctypes.c_void_p()
                _lib.check(getattr(lib, self._CREATE)(*self._create_args(), ctypes.byref(h)))
            d["_handle"] = h
            d["_made_key"] = made
        return lib, dev

    def _ensure_handle(self):
        """The native model with the current parameters packed; returns the library."""
        lib, dev = self._ensure_created()
        tensors = self._tensors()
        d = self.__dict__
        key = d["_made_key"] + tuple((p.data_ptr(), p._version) for p in tensors)
        if key == d.get("_packed_key"):
            return lib
        with torch.cuda.device(dev):
            ps = [p.detach().to(torch.float32).contiguous() for p in tensors]
            torch.cuda.current_stream(dev).synchronize()
            _lib.check(getattr(lib, self._LOAD)(d["_handle"], *self._load_args(ps)))
        d["_packed_key"] = key
        return lib

    def _grown_workspace(self, need, dev):
        """At least `need` bytes on `dev`; the buffer is kept and only ever replaced by a larger one."""
        ws = self.__dict__.get("_workspace")
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            self.__dict__["_workspace"] = ws
        return ws

    def _free(self):
        d = self.__dict__
        if d.get("_handle") is not None:
            try:
                getattr(_lib.load(), self._DESTROY)(d["_handle"])
            except Exception:
                pass
            d["_handle"] = None
            d["_packed_key"] = None
            d["_made_key"] = None

    def __del__(self):
        self._free()
