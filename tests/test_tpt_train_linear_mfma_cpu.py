"""The opt-in fp32 MFMA Linear kernels of TextPoseTransformer training (kernel_train_linear_mfma.h,
b2h_tpt_set_train_linear, TextPoseTransformer.set_train_linear) without a GPU: the two entry points are declared, typed
and exported and answer a NULL model; the Python switch, independent of set_train_kernels; the three b2h_ml_* kernels
compile for gfx950 without scratch, spills or static LDS (their register counts are printed: pytest -s; DESIGN.md
section 19 quotes them)."""
import os
import warnings

import pytest

import hand_pose_sl_amd as hps
from conftest import ROOT
from hand_pose_sl_amd import _lib
from kernel_remarks import kernel_remarks

ML_KERNELS = ["b2h_ml_linearE", "b2h_ml_linear_dxE", "b2h_ml_linear_dwE"]    # as the mangled names spell them


def test_entry_points_declared_typed_exported_and_null_safe():
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    assert "int b2h_tpt_set_train_linear(b2h_tpt* m, int kernel);" in header
    assert "const char* b2h_tpt_train_linear_name(const b2h_tpt* m);" in header
    assert "typedef enum b2h_train_kernel { B2H_TRAIN_VALU = 0, B2H_TRAIN_MFMA = 1 } b2h_train_kernel;" in header
    assert "kernel_train_linear_mfma.h" in header
    assert "b2h_tpt_set_train_linear" in _lib.SYMBOLS and "b2h_tpt_train_linear_name" in _lib.SYMBOLS
    assert _lib.TRAIN_KERNELS == {"valu": 0, "mfma": 1}  # one enum, both switches
    lib = _lib.load()                                   # types every symbol: a missing export raises here
    for kernel in (0, 1, 2, -1):
        assert lib.b2h_tpt_set_train_linear(None, kernel) == _lib.ERR_INVALID
    assert lib.b2h_tpt_train_linear_name(None) is None


def test_python_switch_is_independent_of_train_kernels():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        m = hps.TextPoseTransformer(50, 12, 2, 4, 128, 42, 1, 1, dropout=0.1)
    assert m.train_linear == "valu" and m.train_kernels == "valu"
    assert m.set_train_linear("mfma") is m and m.train_linear == "mfma" and m.train_kernels == "valu"
    assert m.set_train_kernels("mfma") is m and m.train_linear == "mfma" and m.train_kernels == "mfma"
    assert m.set_train_linear("valu") is m and m.train_linear == "valu" and m.train_kernels == "mfma"
    m.set_train_linear("mfma")
    for bad in ("MFMA", "fp32", "", None, 1):
        with pytest.raises(ValueError):
            m.set_train_linear(bad)
    assert m.train_linear == "mfma" and m.train_kernels == "mfma"   # a refused name changes nothing
    m.set_train_kernels("valu")
    assert m.train_linear == "mfma"


def test_ml_kernels_have_no_scratch_spills_or_static_lds():
    kernels, _ = kernel_remarks()
    new = {n: r for n, r in kernels.items() if "b2h_ml_" in n}
    assert len(new) == 3 and all(any(k in n for n in new) for k in ML_KERNELS), sorted(new)
    for name, res in sorted(new.items()):
        print(name, "VGPRs", res["VGPRs"], "AGPRs", res["AGPRs"], "occupancy", res["Occupancy [waves/SIMD]"])
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)   # dynamic LDS only; the caps are raised at creation
