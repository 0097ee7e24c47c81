"""The life cycle of the libb2h model handle behind a torch module, shared by ConvModel, TransformerEnc and
TextPoseTransformer: created on the parameters' device, re-created when that device (or whatever else the
handle was made for) changes, its weights repacked when a parameter is replaced or edited in place, destroyed
with the module; plus the workspace that only grows and the two pointer helpers of the training paths.
"""
import ctypes

import torch

from . import _lib


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _aligned(t):
    """The kernels' 16-byte vector accesses: a contiguous slice of a larger batch may start anywhere."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


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
