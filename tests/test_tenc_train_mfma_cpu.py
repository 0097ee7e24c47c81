"""The two opt-in fp32 MFMA switches of TransformerEnc training (b2h_tenc_set_train_kernel: the whole-matrix attention
pair of kernel_train_attn_whole_mfma.h; b2h_tenc_set_train_linear: the Linear trio of kernel_train_linear_mfma.h;
TransformerEnc.set_train_kernels / set_train_linear) without a GPU: the four entry points are declared, typed and
exported and answer a NULL model; the Python switches, independent of each other; the two b2h_mw_* kernels compile for
gfx950 without scratch, spills or static LDS (their register counts are printed: pytest -s; DESIGN.md section 25 quotes
them)."""
import os
import warnings

import pytest

import hand_pose_sl_amd as hps
from conftest import ROOT
from hand_pose_sl_amd import _lib
from kernel_remarks import kernel_remarks

MW_KERNELS = ["b2h_mw_sdpaE", "b2h_mw_sdpa_bwdE"]       # as the mangled names spell them
DECLARATIONS = {
    "b2h_tenc_set_train_kernel": "int b2h_tenc_set_train_kernel(b2h_tenc* m, int kernel);",
    "b2h_tenc_set_train_linear": "int b2h_tenc_set_train_linear(b2h_tenc* m, int kernel);",
    "b2h_tenc_train_attn_name": "const char* b2h_tenc_train_attn_name(const b2h_tenc* m, int64_t T);",
    "b2h_tenc_train_linear_name": "const char* b2h_tenc_train_linear_name(const b2h_tenc* m);",
}


def test_entry_points_declared_typed_exported_and_null_safe():
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    for name, line in DECLARATIONS.items():
        assert line in header, name
        assert name in _lib.SYMBOLS, name
    assert "typedef enum b2h_train_kernel { B2H_TRAIN_VALU = 0, B2H_TRAIN_MFMA = 1 } b2h_train_kernel;" in header
    assert "kernel_train_attn_whole_mfma.h" in header
    assert _lib.TRAIN_KERNELS == {"valu": 0, "mfma": 1}  # unchanged: one enum, four switches
    lib = _lib.load()                                   # types every symbol: a missing export raises here
    for kernel in (0, 1, 2):
        assert lib.b2h_tenc_set_train_kernel(None, kernel) == _lib.ERR_INVALID
        assert lib.b2h_tenc_set_train_linear(None, kernel) == _lib.ERR_INVALID
    for T in (0, 1, 100):
        assert lib.b2h_tenc_train_attn_name(None, T) is None
    assert lib.b2h_tenc_train_linear_name(None) is None


def _model():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return hps.TransformerEnc(24, 4, 128, 42, 1, dropout=0.1)


def test_python_switches_default_validate_and_are_independent():
    m = _model()
    assert m.train_kernels == "valu" and m.train_linear == "valu"
    assert m._train_route() == (("b2h_tenc_set_train_kernel", 0), ("b2h_tenc_set_train_linear", 0))
    assert m.set_train_linear("mfma") is m and (m.train_kernels, m.train_linear) == ("valu", "mfma")
    assert m._train_route() == (("b2h_tenc_set_train_kernel", 0), ("b2h_tenc_set_train_linear", 1))
    assert m.set_train_kernels("mfma") is m and (m.train_kernels, m.train_linear) == ("mfma", "mfma")
    assert m.set_train_linear("valu") is m and (m.train_kernels, m.train_linear) == ("mfma", "valu")
    assert m._train_route() == (("b2h_tenc_set_train_kernel", 1), ("b2h_tenc_set_train_linear", 0))
    for setter in (m.set_train_kernels, m.set_train_linear):
        for bad in ("MFMA", "", None, 1):
            with pytest.raises(ValueError):
                setter(bad)
    assert (m.train_kernels, m.train_linear) == ("mfma", "valu")    # a refused name changes nothing
    assert m.set_train_kernels("valu") is m and (m.train_kernels, m.train_linear) == ("valu", "valu")
    assert _model().train_kernels == "valu"             # a new model does not inherit another's setting


def test_validation_is_shared_with_text_pose_transformer():
    from hand_pose_sl_amd._native import TrainRoutes
    assert issubclass(hps.TransformerEnc, TrainRoutes) and issubclass(hps.TextPoseTransformer, TrainRoutes)
    assert "_choose_train_route" not in vars(hps.TransformerEnc) and "_choose_train_route" not in vars(hps.TextPoseTransformer)


def test_mw_kernels_have_no_scratch_spills_or_static_lds():
    kernels, _ = kernel_remarks()
    new = {n: r for n, r in kernels.items() if "b2h_mw_" in n}
    assert len(new) == 2 and all(any(k in n for n in new) for k in MW_KERNELS), sorted(new)
    for name, res in sorted(new.items()):
        print(name, "VGPRs", res["VGPRs"], "AGPRs", res["AGPRs"], "occupancy", res["Occupancy [waves/SIMD]"])
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)   # dynamic LDS only; the caps are raised at creation
