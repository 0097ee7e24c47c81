"""Whole-store inference without a GPU: the three new entry points in the header, the ctypes table and the library; the
window plan (a host function) against the restatement tests/rows_ref.py and against its own contract -- every row
addressed exactly once; every host refusal of b2h_scatter_rows and b2h_joint_error before any device work; the refusals of
the Python surface that need no store on a device; the kernels' resource usage."""
import ctypes
import os

import numpy as np
import pytest
import torch

import batch_ref
import hand_pose_sl_amd as hps
import rows_ref
from conftest import ROOT
from hand_pose_sl_amd import _lib
from kernel_remarks import kernel_remarks

OK, INVALID, SHAPE = _lib.OK, _lib.ERR_INVALID, _lib.ERR_SHAPE
i64, vp = ctypes.c_int64, ctypes.c_void_p
i64p = ctypes.POINTER(i64)


def test_entry_points_declared_typed_and_exported():
    header = " ".join(open(os.path.join(ROOT, "include", "b2h.h")).read().split())
    for decl in (
            "enum b2h_coverage { B2H_COVER_ALL = 0, B2H_COVER_FIRST = 1 };",
            "int64_t b2h_window_plan(const int64_t* offsets, int64_t n_utt, int64_t T, int coverage, int64_t* utt_plan, "
            "int64_t* start_plan, int64_t* skip_plan, int64_t capacity);",
            "int b2h_scatter_rows(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body, "
            "const int64_t* utt, const int64_t* start, const int64_t* skip, int64_t B, int64_t T, int predict, int flags, "
            "float factor, const float* pred, float conf, float* rows_out, void* stream);",
            "int b2h_joint_error(const float* rows_pred, const float* rows_true, int64_t n_rows, const int64_t* offsets, "
            "int64_t n_utt, int n_body, float* utt_sum, int32_t* utt_count, double* total_sum, int64_t* total_count, "
            "void* stream);"):
        assert decl in header, decl
    f = ctypes.c_float
    assert _lib.SYMBOLS["b2h_window_plan"] == (i64, [i64p, i64, i64, ctypes.c_int, i64p, i64p, i64p, i64])
    assert _lib.SYMBOLS["b2h_scatter_rows"] == (ctypes.c_int, [vp, i64, vp, i64, ctypes.c_int, vp, vp, vp, i64, i64, ctypes.c_int,
                                                               ctypes.c_int, f, vp, f, vp, vp])
    assert _lib.SYMBOLS["b2h_joint_error"] == (ctypes.c_int, [vp, vp, i64, vp, i64, ctypes.c_int, vp, vp, vp, vp, vp])
    assert _lib.COVERAGE == {"all": 0, "first": 1}
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ("b2h_window_plan", "b2h_scatter_rows", "b2h_joint_error"))
    assert {"window_plan", "predict_dataset", "joint_pixel_error"} <= set(hps.__all__)
    assert all(callable(getattr(hps, n)) for n in ("window_plan", "predict_dataset", "joint_pixel_error"))


# ---- the window plan ---------------------------------------------------------------------------------------------------
def _native_plan(offsets, T, coverage, capacity=None):
    """b2h_window_plan called as the header says: once for the count, once to fill `capacity` (default: all) entries."""
    lib = _lib.load()
    off = (i64 * len(offsets))(*offsets)
    count = lib.b2h_window_plan(off, len(offsets) - 1, T, coverage, None, None, None, 0)
    assert count >= 0, _lib.last_error()
    cap = count if capacity is None else capacity
    arrays = [(i64 * (cap + 1))(*([-7] * (cap + 1))) for _ in range(3)]            # one canary word behind each
    assert lib.b2h_window_plan(off, len(offsets) - 1, T, coverage, *arrays, cap) == count
    assert all(a[cap] == -7 for a in arrays)
    return count, [list(a)[:cap] for a in arrays]


def _length_lists(T):
    every = list(range(3 * T + 2))                                                 # 0 .. 3T + 1, each once
    g = np.random.default_rng(100 + T)
    return [every, every[::-1], [0], [], [3 * T + 1] * 3] + [g.integers(0, 3 * T + 2, size=6).tolist() for _ in range(6)]


def _offsets(lengths, first=0):
    return [first] + (first + np.cumsum(lengths, dtype=np.int64)).tolist() if len(lengths) else [first]


def _fixture_lengths(name):
    off = batch_ref.load_fixture(name)["store"][1]
    return (off[1:] - off[:-1]).tolist()


PLAN_CASES = [(T, ln, 0) for T in (1, 2, 7) for ln in _length_lists(T)] + [(7, [0, 5, 9], 11)] + [
    (7, _fixture_lengths(name), 0) for name in ("h5_store", "json_store")]


@pytest.mark.parametrize("T,lengths,first", PLAN_CASES, ids=[f"{i}-T{c[0]}" for i, c in enumerate(PLAN_CASES)])
def test_plan_equals_the_restatement_and_covers_every_row_once(T, lengths, first):
    offsets = _offsets(lengths, first)
    count, (utt, start, skip) = _native_plan(offsets, T, 0)
    assert [utt, start, skip] == list(rows_ref.plan(lengths, T, "all")) and count == len(utt)
    assert utt == sorted(utt)                                                      # ascending utterances
    seen = {}
    for e, (u, s, k) in enumerate(zip(utt, start, skip)):
        L = lengths[u]
        assert L > 0 and 0 <= k < T
        if L > T:
            assert 0 <= s <= L - T                                                 # no start the clamp would change
        else:
            assert (s, k) == (0, 0)
        for t in range(k, min(L, T)):
            seen.setdefault(offsets[u] + s + t, []).append(e)
    assert sorted(seen) == list(range(first, first + sum(lengths)))                # every row of the store ...
    assert all(len(v) == 1 for v in seen.values())                                 # ... by exactly one (entry, frame >= skip)
    # B2H_COVER_FIRST: one entry per non-empty utterance, at 0
    count, (utt, start, skip) = _native_plan(offsets, T, 1)
    assert utt == [u for u, L in enumerate(lengths) if L > 0] and count == len(utt)
    assert not any(start) and not any(skip)
    assert [utt, start, skip] == list(rows_ref.plan(lengths, T, "first"))


def test_plan_of_the_fixture_stores_hits_every_branch():
    assert rows_ref.plan([0, 1, 3, 7, 8, 19], 7) == ([1, 2, 3, 4, 4, 5, 5, 5], [0, 0, 0, 0, 1, 0, 7, 12], [0, 0, 0, 0, 6, 0, 0, 2])
    for name in ("h5_store", "json_store"):
        ds_offsets = batch_ref.load_fixture(name)["store"][1]
        for coverage in ("all", "first"):
            got = hps.window_plan(ds_offsets, 7, coverage)
            assert all(t.dtype == torch.int64 and t.device.type == "cpu" for t in got)
            assert [t.tolist() for t in got] == list(rows_ref.plan(_fixture_lengths(name), 7, coverage))


def test_plan_capacity():
    offsets = _offsets([0, 1, 3, 7, 8, 19])
    count, full = _native_plan(offsets, 7, 0)
    assert count == 8
    for cap in (0, 1, 5, 7):                                                       # a prefix, the count all the same
        n, part = _native_plan(offsets, 7, 0, capacity=cap)
        assert n == 8 and part == [a[:cap] for a in full]
    lib = _lib.load()
    off = (i64 * len(offsets))(*offsets)
    assert lib.b2h_window_plan(off, 6, 7, 0, None, None, None, 0) == 8             # count only: no array needed
    assert lib.b2h_window_plan(None, 0, 7, 0, None, None, None, 0) == 0            # no utterance: not even offsets
    empty = (i64 * 3)(0, 0, 0)
    assert lib.b2h_window_plan(empty, 2, 7, 0, None, None, None, 4) == 0           # nothing to store: the arrays may be NULL


def test_plan_refusals_carry_their_message():
    lib = _lib.load()
    off = (i64 * 3)(0, 3, 12)
    out = [(i64 * 4)() for _ in range(3)]
    cases = [((off, 2, 0, 0, *out, 4), "T must be >= 1"), ((off, 2, -1, 0, *out, 4), "T must be >= 1"),
             ((off, -1, 7, 0, *out, 4), "negative"), ((off, 2, 7, 0, *out, -1), "negative"),
             ((off, 2, 7, 2, *out, 4), "coverage"), ((off, 2, 7, -1, *out, 4), "coverage"),
             ((None, 2, 7, 0, *out, 4), "offsets is NULL"),
             (((i64 * 3)(0, 5, 4), 2, 7, 0, *out, 4), "ascend"), (((i64 * 3)(-1, 5, 6), 2, 7, 0, *out, 4), "ascend"),
             ((off, 2, 7, 0, None, out[1], out[2], 4), "is NULL"), ((off, 2, 7, 0, out[0], None, out[2], 4), "is NULL"),
             ((off, 2, 7, 0, out[0], out[1], None, 1), "is NULL")]
    for args, message in cases:
        assert lib.b2h_window_plan(*args) == -1, args
        assert message in _lib.last_error(), (args, _lib.last_error())
    assert lib.b2h_window_plan(off, 2, 7, 0, *out, 4) == 3
    with pytest.raises(ValueError, match="ascend"):
        hps.window_plan(torch.tensor([0, 5, 4]), 7)
    with pytest.raises(ValueError, match="T must be >= 1"):
        hps.window_plan(torch.tensor([0, 5, 9]), 0)
    with pytest.raises(ValueError, match="coverage must be one of"):
        hps.window_plan(torch.tensor([0, 5, 9]), 7, "last")
    with pytest.raises(ValueError, match="int64"):
        hps.window_plan(torch.tensor([0, 5, 9], dtype=torch.int32), 7)


# ---- refusals of the two device entry points -----------------------------------------------------------------------
# Made-up, well-separated, 8-byte-aligned addresses that nothing dereferences: a call that got past the host checks
# would ask the HIP runtime about them and fail with another status.
_S = {k: 0x10000000 * (i + 1) for i, k in enumerate(("rows", "offsets", "utt", "start", "skip", "pred", "rows_out"))}
_STORE = 100 * 162 * 4


def _scatter(**kw):
    a = dict(_S, n_rows=100, n_utt=5, n_body=12, B=3, T=7, predict=0, flags=3, factor=1280.0, conf=1.0)
    a.update(kw)
    p = lambda k: None if a[k] is None else vp(a[k])
    return _lib.load().b2h_scatter_rows(p("rows"), a["n_rows"], p("offsets"), a["n_utt"], a["n_body"], p("utt"), p("start"),
                                        p("skip"), a["B"], a["T"], a["predict"], a["flags"], a["factor"], p("pred"), a["conf"],
                                        p("rows_out"), None)


SCATTER_REFUSALS = [
    (dict(n_body=10), INVALID, "n_body"), (dict(n_body=0), INVALID, "n_body"),
    (dict(predict=3), INVALID, "predict"), (dict(predict=-1), INVALID, "predict"),
    (dict(predict=1, n_body=8), INVALID, "n_body = 12"), (dict(predict=2, n_body=8), INVALID, "n_body = 12"),
    (dict(flags=8), INVALID, "flag"), (dict(flags=-1), INVALID, "flag"),
    (dict(factor=0.0), INVALID, "factor"), (dict(factor=-1.0), INVALID, "factor"), (dict(factor=float("nan")), INVALID, "factor"),
    (dict(conf=float("nan")), INVALID, "conf must be finite"), (dict(conf=float("inf")), INVALID, "conf must be finite"),
    (dict(conf=float("-inf")), INVALID, "conf must be finite"),
    (dict(B=-1), SHAPE, "negative"), (dict(T=-1), SHAPE, "negative"), (dict(n_utt=-1), SHAPE, "negative"),
    (dict(n_rows=-1), SHAPE, "negative"),
    (dict(T=(1 << 24) + 1), SHAPE, "too large"), (dict(B=1 << 31), SHAPE, "too large"),
    (dict(rows=None), INVALID, "rows is NULL"), (dict(offsets=None), INVALID, "offsets is NULL"),
    (dict(utt=None), INVALID, "utt is NULL"), (dict(pred=None), INVALID, "pred is NULL"),
    (dict(rows_out=None), INVALID, "rows_out is NULL"),
] + [(dict([(k, _S[k] + 4)]), INVALID, k + " must be 8-byte aligned") for k in _S] + [
    (dict(rows_out=_S["rows"]), INVALID, "overlaps rows"),                          # in place: not allowed
    (dict(rows_out=_S["rows"] + _STORE - 8), INVALID, "overlaps rows"),             # the store's last words
    (dict(rows_out=_S["rows"] - _STORE + 8), INVALID, "overlaps rows"),
    (dict(rows_out=_S["offsets"] + 40), INVALID, "overlaps offsets"),
    (dict(rows_out=_S["utt"] + 16), INVALID, "overlaps utt"),
    (dict(rows_out=_S["start"]), INVALID, "overlaps start"),
    (dict(rows_out=_S["skip"] - _STORE + 8), INVALID, "overlaps skip"),
    (dict(rows_out=_S["pred"] + 3 * 7 * 21 * 8 - 8), INVALID, "overlaps pred"),
]


@pytest.mark.parametrize("kw,status,message", SCATTER_REFUSALS,
                         ids=[f"{i}-{m.replace(' ', '_')}" for i, (_, _, m) in enumerate(SCATTER_REFUSALS)])
def test_scatter_rows_host_refusal(kw, status, message):
    assert _scatter(**kw) == status
    assert message in _lib.last_error()


def test_scatter_rows_no_ops_and_optional_operands():
    lib = _lib.load()
    call = lambda n_body, B, T, conf: lib.b2h_scatter_rows(None, 0, None, 0, n_body, None, None, None, B, T, 0, 0, 1.0, None, conf,
                                                           None, None)
    # B * T == 0: nothing is looked at, after the argument checks
    assert call(8, 0, 7, 1.0) == OK and call(8, 4, 0, 1.0) == OK
    assert call(9, 0, 7, 1.0) == INVALID and call(8, 0, 7, float("nan")) == INVALID
    if not torch.cuda.is_available():
        # start and skip may be left out, an empty store has no rows to point at, rows_out may end where the store begins,
        # the pad flag is accepted: these get past every host check, to the first question to the HIP runtime
        for kw in (dict(start=None), dict(skip=None), dict(start=None, skip=None), dict(rows=None, rows_out=None, n_rows=0),
                   dict(rows_out=_S["rows"] - _STORE), dict(rows_out=_S["rows"] + _STORE), dict(flags=7),
                   dict(factor=0.0, flags=5), dict(conf=0.0), dict(conf=-2.5)):
            assert _scatter(**kw) == _lib.ERR_HIP, (kw, _lib.last_error())


_E = {k: 0x10000000 * (i + 1) for i, k in enumerate(
    ("rows_pred", "rows_true", "offsets", "utt_sum", "utt_count", "total_sum", "total_count"))}


def _error(**kw):
    a = dict(_E, n_rows=100, n_utt=5, n_body=12)
    a.update(kw)
    p = lambda k: None if a[k] is None else vp(a[k])
    return _lib.load().b2h_joint_error(p("rows_pred"), p("rows_true"), a["n_rows"], p("offsets"), a["n_utt"], a["n_body"],
                                       p("utt_sum"), p("utt_count"), p("total_sum"), p("total_count"), None)


ERROR_REFUSALS = [
    (dict(n_rows=-1), SHAPE, "negative"), (dict(n_utt=-1), SHAPE, "negative"),
    (dict(n_body=10), INVALID, "n_body"), (dict(n_body=0), INVALID, "n_body"),
    (dict(total_sum=None), INVALID, "both or neither"), (dict(total_count=None), INVALID, "both or neither"),
    (dict(n_utt=(1 << 30) + 1), SHAPE, "too large"), (dict(n_rows=(1 << 40) + 1), SHAPE, "too large"),
    (dict(rows_pred=None), INVALID, "rows_pred is NULL"), (dict(rows_true=None), INVALID, "rows_true is NULL"),
    (dict(offsets=None), INVALID, "offsets is NULL"), (dict(utt_sum=None), INVALID, "utt_sum is NULL"),
    (dict(utt_count=None), INVALID, "utt_count is NULL"),
] + [(dict([(k, _E[k] + 2)]), INVALID, k + " must be 4-byte aligned") for k in ("rows_pred", "rows_true", "utt_sum", "utt_count")] + [
    (dict([(k, _E[k] + 4)]), INVALID, k + " must be 8-byte aligned") for k in ("offsets", "total_sum", "total_count")] + [
    (dict(utt_sum=_E["rows_pred"] + 4), INVALID, "overlaps rows_pred"),
    (dict(utt_count=_E["rows_true"] + _STORE - 4), INVALID, "overlaps rows_true"),
    (dict(total_sum=_E["offsets"] + 40), INVALID, "overlaps offsets"),
    (dict(total_count=_E["rows_pred"] - 21 * 8 + 8), INVALID, "overlaps rows_pred"),
    (dict(utt_count=_E["utt_sum"] + 5 * 21 * 4 - 4), INVALID, "two outputs overlap"),
    (dict(total_count=_E["total_sum"] + 8), INVALID, "two outputs overlap"),
    (dict(total_sum=_E["utt_count"]), INVALID, "two outputs overlap"),
]


@pytest.mark.parametrize("kw,status,message", ERROR_REFUSALS,
                         ids=[f"{i}-{m.replace(' ', '_')}" for i, (_, _, m) in enumerate(ERROR_REFUSALS)])
def test_joint_error_host_refusal(kw, status, message):
    assert _error(**kw) == status
    assert message in _lib.last_error()


def test_joint_error_no_ops_and_optional_operands():
    lib = _lib.load()
    assert lib.b2h_joint_error(None, None, 0, None, 0, 8, None, None, None, None, None) == OK     # no utterance, no totals
    assert lib.b2h_joint_error(None, None, 0, None, 0, 9, None, None, None, None, None) == INVALID
    if not torch.cuda.is_available():
        # floats at 4 bytes, the totals left out, an empty store, an output that ends where an input begins
        for kw in (dict(rows_pred=_E["rows_pred"] + 4, rows_true=_E["rows_true"] + 12, utt_sum=_E["utt_sum"] + 4,
                        utt_count=_E["utt_count"] + 12),
                   dict(total_sum=None, total_count=None), dict(rows_pred=None, rows_true=None, n_rows=0),
                   dict(utt_sum=_E["rows_pred"] - 5 * 21 * 4), dict(rows_pred=_E["rows_true"]),          # two inputs may alias
                   dict(rows_pred=None, rows_true=None, offsets=None, utt_sum=None, utt_count=None, n_rows=0, n_utt=0)):
            assert _error(**kw) == _lib.ERR_HIP, (kw, _lib.last_error())


# ---- the Python surface: what is refused without a store on a device ------------------------------------------------
def test_python_refusals_that_need_no_gpu():
    model = hps.ConvModel(30, "ReLU", False)
    for loader in (None, [], [{"body_kp": torch.zeros(1, 7, 12, 2)}], "loader"):
        with pytest.raises(ValueError, match=r"DeviceLoader\(ds, batch_size, max_frames"):
            hps.predict_dataset(model, loader)
    with pytest.raises(ValueError, match="two DeviceDatasets"):
        hps.joint_pixel_error(torch.zeros(3, 162), torch.zeros(3, 162))
    with pytest.raises(ValueError, match="two DeviceDatasets"):
        hps.joint_pixel_error(None, None)


# ---- the kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["b2h_scatter_rows_k", "b2h_joint_error_k", "b2h_joint_total_k"])
def test_kernels_have_no_scratch_spills_or_lds(kernel):
    kernels, _ = kernel_remarks()
    new = {n: res for n, res in kernels.items() if kernel in n}
    assert len(new) == 1, sorted(new)
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)


def test_new_kernel_names_match_no_filter_of_the_other_test_files():
    """The other families count their kernels by substring; none of those may pick up a kernel of this family."""
    filters = ("b2h_build_batch_k", "b2h_embed_dwords", "b2h_fwd", "b2h_attn", "b2h_tenc_chain", "b2h_epoch", "b2h_tpt_",
               "b2h_tt_", "b2h_lt_", "b2h_mt_", "b2h_ml_", "b2h_mw_", "b2h_tptt_", "b2h_train_", "b2h_l1_backward",
               "b2h_adam_step_k", "b2h_dropout_masks_k")
    for kernel in ("b2h_scatter_rows_k", "b2h_joint_error_k", "b2h_joint_total_k"):
        assert not [f for f in filters if f in kernel], kernel
