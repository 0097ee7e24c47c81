"""The life cycle of the libb2h model handle behind a torch module, shared by ConvModel, TransformerEnc and
TextPoseTransformer: created on the parameters' device, re-created when that device (or whatever else the
handle was made for) changes, its weights repacked when a parameter is replaced or edited in place, destroyed
with the module; plus the workspace that only grows and the two pointer helpers of the training paths, and the
source of the two transformers' dropout masks (`NativeDropout`).
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
