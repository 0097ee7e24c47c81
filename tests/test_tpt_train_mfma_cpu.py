"""The opt-in fp32 MFMA training attention (kernel_train_attn_mfma.h, b2h_tpt_set_train_kernel,
TextPoseTransformer.set_train_kernels) without a GPU: the two entry points are declared, typed and exported and
answer a NULL model; the Python switch; the three b2h_mt_* kernels compile for gfx950 without scratch, spills or
static LDS (their VGPR counts are printed: pytest -s; DESIGN.md section 17 quotes them)."""
import os
import warnings

import pytest

import hand_pose_sl_amd as hps
from conftest import ROOT
from hand_pose_sl_amd import _lib
from kernel_remarks import kernel_remarks

MFMA_KERNELS = ["b2h_mt_sdpaE", "b2h_mt_sdpa_bwd_kvE", "b2h_mt_sdpa_bwd_qE"]    # as the mangled names spell them


def test_entry_points_declared_typed_exported_and_null_safe():
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    assert "typedef enum b2h_train_kernel { B2H_TRAIN_VALU = 0, B2H_TRAIN_MFMA = 1 } b2h_train_kernel;" in header
    assert "int b2h_tpt_set_train_kernel(b2h_tpt* m, int kernel);" in header
    assert "const char* b2h_tpt_train_attn_name(const b2h_tpt* m, int64_t T);" in header
    assert "kernel_train_attn_mfma.h" in header
    assert "b2h_tpt_set_train_kernel" in _lib.SYMBOLS and "b2h_tpt_train_attn_name" in _lib.SYMBOLS
    assert _lib.TRAIN_KERNELS == {"valu": 0, "mfma": 1}
    lib = _lib.load()                                   # types every symbol: a missing export raises here
    for kernel in (0, 1, 2):
        assert lib.b2h_tpt_set_train_kernel(None, kernel) == _lib.ERR_INVALID
    assert lib.b2h_tpt_train_attn_name(None, 200) is None
    assert all(lib.b2h_tpt_train_bytes(None, 2, 40, 200, which) == 0 for which in (0, 1))


def test_python_switch():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        m = hps.TextPoseTransformer(50, 12, 2, 4, 128, 42, 1, 1, dropout=0.1)
    assert m.train_kernels == "valu"
    assert m.set_train_kernels("mfma") is m and m.train_kernels == "mfma"
    assert m.set_train_kernels("valu") is m and m.train_kernels == "valu"
    for bad in ("MFMA", "fp32", "", None, 1):
        with pytest.raises(ValueError):
            m.set_train_kernels(bad)
    assert m.train_kernels == "valu"                    # a refused name changes nothing


def test_mfma_kernels_have_no_scratch_spills_or_static_lds():
    kernels, _ = kernel_remarks()
    new = {n: r for n, r in kernels.items() if "b2h_mt_" in n}
    assert len(new) == 3 and all(any(k in n for n in new) for k in MFMA_KERNELS), sorted(new)
    for name, res in sorted(new.items()):
        print(name, "VGPRs", res["VGPRs"], "AGPRs", res["AGPRs"], "occupancy", res["Occupancy [waves/SIMD]"])
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)   # dynamic LDS only; the caps are raised at creation
