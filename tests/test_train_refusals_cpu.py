"""The one refusal of the four transformer training entry points that needs no GPU: a NULL model, whatever else is
wrong with the call.  The rest of the refusals are pinned in test_train_refusals_gpu.py."""
import ctypes

from hand_pose_sl_amd import _lib

NAN = float("nan")


def test_null_model_is_refused_first():
    lib = _lib.load()
    ptrs = (ctypes.c_void_p * 1)(None)
    expected = (_lib.ERR_INVALID, "model is NULL")
    for params, p in ((ptrs, 0.0), (None, NAN)):
        calls = (lib.b2h_tenc_train_forward(None, params, None, None, p, None, None, 0, 1, 2, None),
                 lib.b2h_tenc_backward(None, params, None, p, None, None, 0, None, None, None, 0, 1, 2, None),
                 lib.b2h_tpt_train_forward(None, params, None, None, None, p, None, None, 0, 1, 2, 3, None),
                 lib.b2h_tpt_backward(None, params, None, None, p, None, None, 0, None, None, None, 0, 1, 2, 3, None))
        for rc in calls:
            assert (rc, lib.b2h_last_error().decode()) == expected
