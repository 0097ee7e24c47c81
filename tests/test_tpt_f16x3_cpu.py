"""TextPoseTransformer's f16x3 switch without a GPU: `set_precision` on the mirror, the constructor's unchanged
refusal, and `b2h_tpt_set_kernel` declared, typed, exported and refusing bad arguments."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from tpt_ref import build


def test_set_precision_selects_and_returns_the_model():
    model = build(50, 1, 1)
    assert model.precision == "fp32"                         # the default stays exact fp32
    assert model.set_precision("f16x3") is model and model.precision == "f16x3"
    assert model.set_precision("fp32") is model and model.precision == "fp32"
    with pytest.raises(ValueError, match="precision"):
        model.set_precision("bf16")
    assert model.precision == "fp32"                         # a refused name changes nothing
    with pytest.raises(ValueError, match="precision"):
        build(50, 1, 1, precision="f16x3")                   # the constructor keeps accepting only "fp32"


def test_set_kernel_declared_typed_exported_and_checked():
    from hand_pose_sl_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "b2h.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+b2h_tpt_set_kernel\s*\(\s*b2h_tpt\s*\*\s*m\s*,\s*int\s+kernel\s*\)", header)
    assert _lib.SYMBOLS["b2h_tpt_set_kernel"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    lib = _lib.load()
    assert lib.b2h_tpt_set_kernel(None, 1) == _lib.ERR_INVALID
    assert lib.b2h_tpt_set_kernel(None, 0) == _lib.ERR_INVALID
    assert "NULL" in _lib.last_error()
