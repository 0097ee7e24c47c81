"""The native dropout masks (b2h_dropout_masks, kernel_dropout_masks.h, set_dropout_source) without a GPU: the numpy
restatement of the generator (philox_ref.py) against Random123's known answers and the issue's two pinned vectors; the
three entry points declared, typed, exported; every refusal of b2h_dropout_masks, which launches nothing, and its
no-op cases; the Python switch on both models; the kernel compiles for gfx950 without scratch or spills (its register
counts are printed: pytest -s; DESIGN.md section 20 quotes them)."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import hand_pose_sl_amd as hps
import philox_ref
from conftest import ROOT
from hand_pose_sl_amd import _lib
from kernel_remarks import kernel_remarks


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_restatement_reproduces_the_known_answers():
    f = 0xFFFFFFFF
    assert _hex(philox_ref.philox4x32_10(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(philox_ref.philox4x32_10(f, f, f, f, f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(philox_ref.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_restatement_reproduces_the_pinned_masks():
    assert philox_ref.mask(20, 2, 5, 3, 0.5).tolist() == [1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0]
    assert philox_ref.mask(20, 2, 5, 3, 0.1).tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1]
    # the mapping's other rules: thr from float32(p); p = 0 keeps all, p = 1 none; the step enters mod 2^32; an element
    # does not depend on the mask's size
    assert philox_ref.threshold(0.1) == int(np.ceil(float(np.float32(0.1)) * 2.0 ** 32)) != int(np.ceil(0.1 * 2.0 ** 32))
    assert philox_ref.threshold(0.0) == 0 and philox_ref.threshold(1.0) == 2 ** 32 and philox_ref.threshold(0.5) == 2 ** 31
    assert philox_ref.mask(50, 0, 0, 3, 0.0).all() and not philox_ref.mask(50, 0, 0, 3, 1.0).any()
    assert np.array_equal(philox_ref.mask(50, 1, 2 ** 32 + 7, 3, 0.5), philox_ref.mask(50, 1, 7, 3, 0.5))
    assert np.array_equal(philox_ref.mask(50, 1, 7, 3, 0.5)[:21], philox_ref.mask(21, 1, 7, 3, 0.5))
    assert not np.array_equal(philox_ref.mask(64, 1, 7, 3, 0.5), philox_ref.mask(64, 1, 7, 3 + 2 ** 32, 0.5))


def test_entry_points_declared_typed_and_exported():
    header = " ".join(open(os.path.join(ROOT, "include", "b2h.h")).read().split())
    for decl in ("int b2h_dropout_masks(uint8_t* const* masks, const int64_t* numel, int n_masks, int first_index, float p, "
                 "uint64_t seed, uint64_t step, const uint64_t* step_dev, void* stream);",
                 "int64_t b2h_tpt_mask_numel(const b2h_tpt* m, int64_t B, int64_t S, int64_t T, int64_t* numel, int capacity);",
                 "int64_t b2h_tenc_mask_numel(const b2h_tenc* m, int64_t B, int64_t T, int64_t* numel, int capacity);"):
        assert decl in header, decl
    assert "drawn by the caller" not in header and "kernel_dropout_masks.h" in header
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    assert _lib.SYMBOLS["b2h_dropout_masks"] == (ctypes.c_int, [ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.c_int, ctypes.c_int,
                                                                ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, vp, vp])
    assert _lib.SYMBOLS["b2h_tpt_mask_numel"] == (i64, [vp, i64, i64, i64, ctypes.POINTER(i64), ctypes.c_int])
    assert _lib.SYMBOLS["b2h_tenc_mask_numel"] == (i64, [vp, i64, i64, ctypes.POINTER(i64), ctypes.c_int])
    lib = _lib.load()                                   # types every symbol: a missing export raises here
    out = (i64 * 4)(-7, -7, -7, -7)
    assert lib.b2h_tpt_mask_numel(None, 2, 7, 15, out, 4) == 0 and lib.b2h_tenc_mask_numel(None, 2, 9, out, 4) == 0
    assert lib.b2h_tpt_mask_numel(None, 2, 7, 15, None, 0) == 0 and lib.b2h_tenc_mask_numel(None, 2, 9, None, 0) == 0
    assert list(out) == [-7] * 4                        # nothing written


def _call(lib, ptrs, sizes, n=None, first=0, p=0.5):
    masks = None if ptrs is None else (ctypes.c_void_p * len(ptrs))(*ptrs)
    numel = None if sizes is None else (ctypes.c_int64 * len(sizes))(*sizes)
    n = (len(ptrs) if ptrs is not None else len(sizes)) if n is None else n
    return lib.b2h_dropout_masks(masks, numel, n, first, p, 3, 5, None, None)


def test_refusals_launch_nothing_and_no_ops_return_ok():
    """No GPU here: a call that reached a launch would fail with another status (B2H_ERR_HIP), so ERR_INVALID with a
    message shows the refusal came first; the pointers are made-up addresses that nothing dereferences."""
    lib = _lib.load()
    good = 0x10000
    refused = {
        "NULL masks": lambda: _call(lib, None, [16]),
        "NULL numel": lambda: _call(lib, [good], None),
        "n_masks < 0": lambda: _call(lib, [good], [16], n=-1),
        "first_index < 0": lambda: _call(lib, [good], [16], first=-1),
        "NULL mask pointer": lambda: _call(lib, [good, None], [16, 16]),
        "NULL pointer of an empty mask": lambda: _call(lib, [None], [0]),
        "misaligned by 1": lambda: _call(lib, [good + 1], [16]),
        "misaligned by 8": lambda: _call(lib, [good, good + 8], [16, 16]),
        "misaligned, 70th of 70": lambda: _call(lib, [good + 32 * i for i in range(69)] + [good + 4], [16] * 70),
        "numel < 0": lambda: _call(lib, [good, good + 64], [16, -1]),
        "p < 0": lambda: _call(lib, [good], [16], p=-1e-6),
        "p > 1": lambda: _call(lib, [good], [16], p=1.0 + 2.0 ** -20),
        "p NaN": lambda: _call(lib, [good], [16], p=float("nan")),
        "p inf": lambda: _call(lib, [good], [16], p=float("inf")),
        "bad p with nothing to draw": lambda: _call(lib, [good], [0], p=2.0),
    }
    for what, call in refused.items():
        assert call() == _lib.ERR_INVALID, what
        assert _lib.last_error(), what
        with pytest.raises(ValueError):
            _lib.check(call())
    assert lib.b2h_dropout_masks(None, None, 0, 0, 0.5, 3, 5, None, None) == _lib.OK          # n_masks == 0
    assert _call(lib, [good, good + 16, good + 16], [0, 0, 0]) == _lib.OK                     # all sizes 0
    assert _call(lib, [good + 16 * i for i in range(70)], [0] * 70, first=2 ** 31 - 71, p=1.0) == _lib.OK
    assert _call(lib, [good], [0], p=0.0) == _lib.OK


def _models():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return [hps.TextPoseTransformer(50, 12, 2, 4, 128, 42, 1, 1, dropout=0.1), hps.TransformerEnc(24, 4, 128, 42, 1, dropout=0.1)]


@pytest.mark.parametrize("which", [0, 1], ids=["TextPoseTransformer", "TransformerEnc"])
def test_python_switch(which):
    import torch
    m = _models()[which]
    assert m.dropout_source == "torch" and type(m).dropout_source == "torch"
    torch.manual_seed(1234)
    assert m.set_dropout_source("native") is m and m.dropout_source == "native"
    assert m._drop_seed == 1234 == torch.initial_seed()        # no seed given: torch's
    assert m.set_dropout_source("native", seed=2 ** 40 + 5) is m and m._drop_seed == 2 ** 40 + 5
    assert m._drop_step is None                                # made on the GPU, at the first draw
    for bad in ("Native", "philox", "", None, 1):
        with pytest.raises(ValueError):
            m.set_dropout_source(bad)
    assert m.dropout_source == "native" and m._drop_seed == 2 ** 40 + 5    # a refused name changes nothing
    assert m.set_dropout_source("torch") is m and m.dropout_source == "torch"
    assert _models()[which].dropout_source == "torch"          # per model, not per class
    assert "dropout_source" not in m.state_dict() and not any("drop" in k for k in m.state_dict() if "dropout" not in k)
    m.set_dropout_source("native", seed=3)
    with pytest.raises(RuntimeError):                          # no CPU path, and no quiet fall-back to torch's draw
        m._draw_dropout_masks(2, 7, 15) if which == 0 else m._draw_dropout_masks(2, 9)


def test_mask_orders_of_the_two_models():
    import tpt_train_ref
    tpt, tenc = _models()
    assert tpt._mask_order(2, 7, 15) == tpt_train_ref.mask_shapes(2, 7, 15, 1, 1)
    assert tenc._mask_order(2, 9) == [("pos", (2, 9, 24)), ((0, "attn"), (2, 4, 9, 9)), ((0, "drop1"), (2, 9, 128)),
                                      ((0, "ff"), (2, 9, 128)), ((0, "drop2"), (2, 9, 128))]


def test_kernel_has_no_scratch_or_spills():
    kernels, listing = kernel_remarks()
    new = {n: res for n, res in kernels.items() if "b2h_dropout_masks_k" in n}
    assert len(new) == 1, sorted(new)
    for name, res in new.items():
        print(name, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "occupancy", res["Occupancy [waves/SIMD]"])
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)
    text = open(listing).read()
    body = text[text.index("b2h_dropout_masks_kENS_6DmArgsE:"):]
    body = body[:body.index("s_endpgm")]
    # one 16-byte store for the whole chunks, byte stores for the tail, no atomics; the round products are v_mad_u64_u32
    assert len(re.findall(r"\bglobal_store_dwordx4\b", body)) == 1 and "atomic" not in body
    assert len(re.findall(r"\bv_mad_u64_u32\b", body)) >= 60
