"""Overlapping inference windows without a GPU: the two new entry points in the header, the ctypes table and the library;
b2h_window_plan_overlap (a host function) against the restatement tests/blend_ref.py and against its own contract -- a
window overlaps the used frames of the one before it by exactly K, fades never intersect, every row has one owner, K = 0
is b2h_window_plan; every host refusal of both functions with its message; the refusals of the Python surface and of
the CLI that need no store on a device; the new kernel's resource usage."""
import ctypes
import os

import numpy as np
import pytest
import torch

import blend_ref
import hand_pose_sl_amd as hps
import rows_ref
from conftest import ROOT
from hand_pose_sl_amd import _lib, infer
from kernel_remarks import kernel_remarks

OK, INVALID, SHAPE = _lib.OK, _lib.ERR_INVALID, _lib.ERR_SHAPE
i64, vp, f32 = ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
i64p = ctypes.POINTER(i64)


def test_entry_points_declared_typed_and_exported():
    header = " ".join(open(os.path.join(ROOT, "include", "b2h.h")).read().split())
    for decl in (
            "enum b2h_blend { B2H_BLEND_LINEAR = 0, B2H_BLEND_CENTRE = 1 };",
            "int64_t b2h_window_plan_overlap(const int64_t* offsets, int64_t n_utt, int64_t T, int64_t overlap, "
            "int64_t* utt_plan, int64_t* start_plan, int64_t* skip_plan, int64_t capacity);",
            "int b2h_scatter_rows_blend(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body, "
            "const int64_t* utt_plan, const int64_t* start_plan, const int64_t* skip_plan, int64_t n_plan, int64_t entry0, "
            "int64_t B, int64_t T, int predict, int flags, float factor, const float* pred, const float* pred_before, "
            "int blend, float conf, float* rows_out, void* stream);",
            "#define B2H_VERSION 100"):
        assert decl in header, decl
    assert _lib.SYMBOLS["b2h_window_plan_overlap"] == (i64, [i64p, i64, i64, i64, i64p, i64p, i64p, i64])
    assert _lib.SYMBOLS["b2h_scatter_rows_blend"] == (ctypes.c_int, [vp, i64, vp, i64, ctypes.c_int, vp, vp, vp, i64, i64, i64, i64,
                                                                     ctypes.c_int, ctypes.c_int, f32, vp, vp, ctypes.c_int, f32, vp, vp])
    assert _lib.BLEND == {"linear": blend_ref.LINEAR, "centre": blend_ref.CENTRE} == {"linear": 0, "centre": 1}
    lib = _lib.load()
    assert hasattr(lib, "b2h_window_plan_overlap") and hasattr(lib, "b2h_scatter_rows_blend")
    assert callable(hps.DeviceLoader.write_back_blend)


# ---- the plan -----------------------------------------------------------------------------------------------------------
def _native_plan(offsets, T, K, capacity=None):
    """b2h_window_plan_overlap called as the header says: once for the count, once to fill `capacity` (default: all)."""
    lib = _lib.load()
    off = (i64 * len(offsets))(*offsets)
    count = lib.b2h_window_plan_overlap(off, len(offsets) - 1, T, K, None, None, None, 0)
    assert count >= 0, _lib.last_error()
    cap = count if capacity is None else capacity
    arrays = [(i64 * (cap + 1))(*([-7] * (cap + 1))) for _ in range(3)]            # one canary word behind each
    assert lib.b2h_window_plan_overlap(off, len(offsets) - 1, T, K, *arrays, cap) == count
    assert all(a[cap] == -7 for a in arrays)
    return count, [list(a)[:cap] for a in arrays]


def _lengths(T, K):
    return [0, 1, T, T + 1, 2 * T - K - 1, 2 * T - K, 2 * T - K + 1, 5 * T + 3]


def _offsets(lengths, first=0):
    return [first] + (first + np.cumsum(lengths, dtype=np.int64)).tolist()


PLAN_CASES = [(T, K) for T in (1, 2, 8, 13) for K in range(T // 2 + 1)]


@pytest.mark.parametrize("T,K", PLAN_CASES)
def test_plan_equals_the_restatement_and_keeps_its_invariants(T, K):
    lengths = _lengths(T, K)
    for first in (0, 11):
        offsets = _offsets(lengths, first)
        count, (utt, start, skip) = _native_plan(offsets, T, K)
        assert [utt, start, skip] == list(blend_ref.plan(lengths, T, K)) and count == len(utt)
    assert utt == sorted(utt) and set(utt) == {u for u, L in enumerate(lengths) if L > 0}
    owner = {}
    for e, (u, s, k) in enumerate(zip(utt, start, skip)):
        L = lengths[u]
        first_of_utt, last_of_utt = e == 0 or utt[e - 1] != u, e + 1 == len(utt) or utt[e + 1] != u
        assert 0 <= k < T
        if L <= T:
            assert (s, k) == (0, 0) and first_of_utt and last_of_utt
        else:
            assert 0 <= s <= L - T                                                 # no start the clamp would change
            assert last_of_utt == (s == L - T)                                     # the last window ends with the utterance
        if first_of_utt:
            assert (s, k) == (0, 0)
        else:
            assert start[e - 1] + T - (s + k) == K                                 # overlaps the used frames before it by K
            assert k == 0 or last_of_utt                                           # only a last window skips
        # fade-in [s + k, s + k + K) and fade-out [next used frame, s + T) of one window never intersect
        if not first_of_utt and not last_of_utt:
            assert s + k + K <= start[e + 1] + skip[e + 1]
        end = min(L, T) if last_of_utt else start[e + 1] + skip[e + 1] - s
        assert k < end <= T                                                        # every window owns something
        for t in range(k, end):
            owner.setdefault(offsets[u] + s + t, []).append(e)
    assert sorted(owner) == list(range(first, first + sum(lengths)))               # every row of the store ...
    assert all(len(v) == 1 for v in owner.values())                                # ... has exactly one owner
    # the restatement's ownership map says the same
    got = blend_ref.owned(offsets, utt, start, skip, T, offsets[-1])
    assert sorted(row for _, _, row, _ in got) == sorted(owner)
    assert all(owner[row] == [e] for e, _, row, _ in got)
    regions = [r for _, _, _, r in got if r is not None]
    assert all(w == K and 0 <= p < K and 0 <= ta < T for ta, p, w in regions)
    long = sum(len([e for e in range(len(utt)) if utt[e] == u]) - 1 for u in set(utt))
    assert len(regions) == K * long                                                # K blended rows per window boundary


@pytest.mark.parametrize("T", [1, 2, 8, 13])
def test_plan_without_overlap_is_the_window_plan(T):
    lib = _lib.load()
    lengths = _lengths(T, 0) + list(range(3 * T + 2))
    offsets = _offsets(lengths)
    count, plan = _native_plan(offsets, T, 0)
    off = (i64 * len(offsets))(*offsets)
    arrays = [(i64 * count)() for _ in range(3)]
    assert lib.b2h_window_plan(off, len(lengths), T, 0, *arrays, count) == count
    assert [list(a) for a in arrays] == plan == [list(v) for v in rows_ref.plan(lengths, T)]
    got = hps.window_plan(torch.tensor(offsets), T, overlap=0)
    assert [t.tolist() for t in got] == plan


def test_plan_capacity_and_the_python_wrapper():
    offsets = _offsets(_lengths(8, 3))
    count, full = _native_plan(offsets, 8, 3)
    assert count == len(full[0]) > 8
    for cap in (0, 1, 5, count - 1):                                               # a prefix, the count all the same
        n, part = _native_plan(offsets, 8, 3, capacity=cap)
        assert n == count and part == [a[:cap] for a in full]
    lib = _lib.load()
    assert lib.b2h_window_plan_overlap(None, 0, 8, 3, None, None, None, 0) == 0    # no utterance: not even offsets
    empty = (i64 * 3)(0, 0, 0)
    assert lib.b2h_window_plan_overlap(empty, 2, 8, 3, None, None, None, 4) == 0   # nothing to store: the arrays may be NULL
    got = hps.window_plan(torch.tensor(offsets), 8, overlap=3)
    assert all(t.dtype == torch.int64 and t.device.type == "cpu" for t in got)
    assert [t.tolist() for t in got] == full
    # the example of the design notes: 19 rows, T = 7, K = 2 -> stride 5
    assert blend_ref.plan([19], 7, 2) == ([0, 0, 0, 0], [0, 5, 10, 12], [0, 0, 0, 3])


def test_plan_refusals_carry_their_message():
    lib = _lib.load()
    off = (i64 * 3)(0, 3, 30)
    out = [(i64 * 8)() for _ in range(3)]
    cases = [((off, 2, 0, 0, *out, 8), "T must be >= 1"), ((off, 2, -1, 0, *out, 8), "T must be >= 1"),
             ((off, -1, 7, 2, *out, 8), "negative"), ((off, 2, 7, 2, *out, -1), "negative"),
             ((None, 2, 7, 2, *out, 8), "offsets is NULL"),
             (((i64 * 3)(0, 5, 4), 2, 7, 2, *out, 8), "ascend"), (((i64 * 3)(-1, 5, 6), 2, 7, 2, *out, 8), "ascend"),
             ((off, 2, 7, -1, *out, 8), "overlap -1, T 7"), ((off, 2, 7, 4, *out, 8), "overlap 4, T 7"),
             ((off, 2, 8, 5, *out, 8), "overlap 5, T 8"), ((off, 2, 1, 1, *out, 8), "overlap 1, T 1"),
             ((off, 2, 7, 2, None, out[1], out[2], 8), "is NULL"), ((off, 2, 7, 2, out[0], None, out[2], 8), "is NULL"),
             ((off, 2, 7, 2, out[0], out[1], None, 1), "is NULL")]
    for args, message in cases:
        assert lib.b2h_window_plan_overlap(*args) == -1, args
        assert message in _lib.last_error(), (args, _lib.last_error())
    assert lib.b2h_window_plan_overlap(off, 2, 7, 3, *out, 8) == 7                 # 3 rows: 1 window; 27 rows, stride 4: 6
    assert lib.b2h_window_plan_overlap(off, 2, 8, 4, *out, 8) == 7
    with pytest.raises(ValueError, match="overlap 4, T 7"):
        hps.window_plan(torch.tensor([0, 5, 9]), 7, overlap=4)
    with pytest.raises(ValueError, match="overlap -2, T 7"):
        hps.window_plan(torch.tensor([0, 5, 9]), 7, overlap=-2)
    with pytest.raises(ValueError, match="needs coverage='all'"):
        hps.window_plan(torch.tensor([0, 5, 9]), 7, "first", overlap=2)
    with pytest.raises(ValueError, match="coverage must be one of"):
        hps.window_plan(torch.tensor([0, 5, 9]), 7, "last", overlap=2)


# ---- refusals of the device entry point ------------------------------------------------------------------------------
# Made-up, well-separated, 8-byte-aligned addresses that nothing dereferences: a call that got past the host checks
# would ask the HIP runtime about them and fail with another status.
_S = {k: 0x10000000 * (i + 1) for i, k in enumerate(
    ("rows", "offsets", "utt_plan", "start_plan", "skip_plan", "pred", "pred_before", "rows_out"))}
_STORE = 100 * 162 * 4


def _blend(**kw):
    a = dict(_S, n_rows=100, n_utt=5, n_body=12, n_plan=9, entry0=2, B=3, T=7, predict=0, flags=3, factor=1280.0, blend=0,
             conf=1.0)
    a.update(kw)
    p = lambda k: None if a[k] is None else vp(a[k])
    return _lib.load().b2h_scatter_rows_blend(
        p("rows"), a["n_rows"], p("offsets"), a["n_utt"], a["n_body"], p("utt_plan"), p("start_plan"), p("skip_plan"),
        a["n_plan"], a["entry0"], a["B"], a["T"], a["predict"], a["flags"], a["factor"], p("pred"), p("pred_before"), a["blend"],
        a["conf"], p("rows_out"), None)


BLEND_REFUSALS = [
    # b2h_scatter_rows's own
    (dict(n_body=10), INVALID, "n_body"), (dict(predict=3), INVALID, "predict"), (dict(predict=1, n_body=8), INVALID, "n_body = 12"),
    (dict(flags=8), INVALID, "flag"), (dict(factor=0.0), INVALID, "factor"), (dict(factor=float("nan")), INVALID, "factor"),
    (dict(conf=float("nan")), INVALID, "conf must be finite"), (dict(conf=float("inf")), INVALID, "conf must be finite"),
    (dict(B=-1), SHAPE, "negative"), (dict(T=-1), SHAPE, "negative"), (dict(n_utt=-1), SHAPE, "negative"),
    (dict(n_rows=-1), SHAPE, "negative"), (dict(n_plan=-1), SHAPE, "negative"),
    (dict(T=(1 << 24) + 1), SHAPE, "too large"), (dict(B=1 << 31, n_plan=1 << 32), SHAPE, "too large"),
    (dict(n_plan=(1 << 40) + 1), SHAPE, "plan too large"),
    (dict(rows=None), INVALID, "rows is NULL"), (dict(offsets=None), INVALID, "offsets is NULL"),
    (dict(pred=None), INVALID, "pred is NULL"), (dict(rows_out=None), INVALID, "rows_out is NULL"),
    # its own
    (dict(blend=2), INVALID, "blend must be a b2h_blend value"), (dict(blend=-1), INVALID, "blend must be a b2h_blend value"),
    (dict(entry0=-1), INVALID, "entry0 -1, B 3, n_plan 9"), (dict(entry0=7), INVALID, "entry0 7, B 3, n_plan 9"),
    (dict(B=10, entry0=0), INVALID, "entry0 0, B 10, n_plan 9"), (dict(n_plan=0, entry0=0), INVALID, "entry0 0, B 3, n_plan 0"),
    (dict(utt_plan=None), INVALID, "utt_plan is NULL"), (dict(start_plan=None), INVALID, "start_plan is NULL"),
    (dict(skip_plan=None), INVALID, "skip_plan is NULL"),
] + [(dict([(k, _S[k] + 4)]), INVALID, k + " must be 8-byte aligned") for k in _S] + [
    (dict(rows_out=_S["rows"]), INVALID, "overlaps rows"),
    (dict(rows_out=_S["utt_plan"] + 64), INVALID, "overlaps utt_plan"),             # the plan's last word
    (dict(rows_out=_S["start_plan"]), INVALID, "overlaps start_plan"),
    (dict(rows_out=_S["skip_plan"] - _STORE + 8), INVALID, "overlaps skip_plan"),
    (dict(rows_out=_S["pred"] + 3 * 7 * 21 * 8 - 8), INVALID, "overlaps pred"),
    (dict(rows_out=_S["pred_before"] + 7 * 21 * 8 - 8), INVALID, "overlaps pred_before"),
    (dict(rows_out=_S["pred_before"] - _STORE + 8), INVALID, "overlaps pred_before"),
]


@pytest.mark.parametrize("kw,status,message", BLEND_REFUSALS,
                         ids=[f"{i}-{m.replace(' ', '_')}" for i, (_, _, m) in enumerate(BLEND_REFUSALS)])
def test_scatter_rows_blend_host_refusal(kw, status, message):
    assert _blend(**kw) == status
    assert message in _lib.last_error()


def test_scatter_rows_blend_refusal_order_no_ops_and_optional_operands():
    # b2h_scatter_rows's scalar checks come first, the blend's own before the no-op and the pointers
    assert _blend(conf=float("nan"), blend=5) == INVALID and "conf" in _lib.last_error()
    assert _blend(blend=5, entry0=-1, rows=None) == INVALID and "blend" in _lib.last_error()
    assert _blend(entry0=-1, rows=None) == INVALID and "entry0" in _lib.last_error()
    lib = _lib.load()
    call = lambda n_body, B, T, blend, entry0, n_plan: lib.b2h_scatter_rows_blend(
        None, 0, None, 0, n_body, None, None, None, n_plan, entry0, B, T, 0, 0, 1.0, None, None, blend, 1.0, None, None)
    # B * T == 0: no pointer is looked at, after the argument checks
    assert call(8, 0, 7, 0, 0, 0) == OK and call(8, 4, 0, 1, 2, 6) == OK and call(8, 0, 7, 0, 5, 5) == OK
    assert call(9, 0, 7, 0, 0, 0) == INVALID and call(8, 0, 7, 2, 0, 0) == INVALID and call(8, 0, 7, 0, 6, 5) == INVALID
    if not torch.cuda.is_available():
        # pred_before may be left out or alias pred, an empty store has no rows to point at, the batch may be the plan's
        # first or last entries: these get past every host check, to the first question to the HIP runtime
        for kw in (dict(pred_before=None), dict(pred_before=None, entry0=0), dict(pred_before=_S["pred"] + 7 * 21 * 8),
                   dict(rows=None, rows_out=None, n_rows=0), dict(entry0=6), dict(entry0=0, B=9), dict(blend=1),
                   dict(rows_out=_S["pred_before"] + 7 * 21 * 8), dict(flags=7)):
            assert _blend(**kw) == _lib.ERR_HIP, (kw, _lib.last_error())


# ---- the Python surface and the CLI: what is refused without a store on a device -----------------------------------
def _stub_loader(max_frames):
    """What predict_dataset's refusals read of a DeviceLoader, without the store on a device that a real one needs."""
    loader = object.__new__(hps.DeviceLoader)
    loader.__dict__.update(ds=type("Store", (), {"n_body": 12, "tokens": None})(), max_frames=max_frames, batch_size=2,
                           predict="right_hand", _augment=None)
    return loader


def test_python_refusals_that_need_no_gpu():
    model = hps.ConvModel(30, "ReLU", False)
    for overlap in (-1, 5, 9, 100):
        with pytest.raises(ValueError, match=r"overlap must be in 0 \.\. max_frames // 2 = 4"):
            hps.predict_dataset(model, _stub_loader(9), overlap=overlap)
    with pytest.raises(ValueError, match=r"max_frames // 2 = 0"):
        hps.predict_dataset(model, _stub_loader(1), overlap=1)
    for blend in ("cubic", "center", None, 0):
        with pytest.raises(ValueError, match="blend must be one of"):
            hps.predict_dataset(model, _stub_loader(9), overlap=2, blend=blend)
    with pytest.raises(ValueError, match="needs coverage='all'"):
        hps.predict_dataset(model, _stub_loader(9), coverage="first", overlap=2)
    with pytest.raises(ValueError, match=r"DeviceLoader\(ds, batch_size, max_frames"):
        hps.predict_dataset(model, None, overlap=2)


def test_cli_overlap_needs_all_frames(tmp_path):
    common = ["--data", str(tmp_path), "--model-checkpoint", str(tmp_path / "none.pth"), "--output-folder", str(tmp_path / "out")]
    with pytest.raises(SystemExit, match="--overlap needs --all-frames"):
        infer.main(common + ["--overlap", "6"])
    with pytest.raises(SystemExit, match=r"--overlap must be in 0 \.\. --max-frames // 2 = 8"):
        infer.main(common + ["--all-frames", "--max-frames", "16", "--overlap", "9"])
    with pytest.raises(SystemExit) as bad:                                          # argparse's own: an unknown --blend
        infer.main(common + ["--all-frames", "--overlap", "6", "--blend", "cubic"])
    assert bad.value.code == 2
    assert not (tmp_path / "out").exists()


# ---- the property the feature is for, on the CPU oracle ----------------------------------------------------------------
def test_oracle_conv_model_shows_the_seams_and_the_halo_removes_them():
    """The ConvModel of tests/test_predict_overlap_gpu.py's halo test (same seed, same store) through the CPU oracle:
    windows of 32 that touch differ from the whole 70-frame utterance next to every boundary, by far more than the 1e-3
    the GPU test asks for; windows that overlap by 16 with blend CENTRE do not, and LINEAR still mixes in edge frames."""
    import oracle
    torch.manual_seed(blend_ref.HALO_SEED)
    state = {k: v.detach() for k, v in hps.ConvModel(30, "ReLU", False).state_dict().items()}
    forward = lambda x: oracle.torch_forward(torch.from_numpy(x), state).numpy()
    rows = blend_ref.halo_rows()
    whole, touching, centre, linear = (blend_ref.windowed(forward, rows, T, K, blend).astype(np.float64)
                                       for T, K, blend in ((70, 0, 0), (32, 0, 0), (32, 16, blend_ref.CENTRE), (32, 16, blend_ref.LINEAR)))
    near = blend_ref.near_seams(32)
    assert near.sum() == 3 * (16 + 14)                                             # seams at rows 32 and 64 of 70
    assert np.abs(centre - whole).max() <= 2e-5
    assert np.abs(touching - whole)[near].max() > 1e-2 and np.abs(touching - whole)[~near].max() <= 2e-5
    assert 1e-3 < np.abs(linear - whole).max() < np.abs(touching - whole).max()


# ---- the kernel ---------------------------------------------------------------------------------------------------------
def test_blend_kernel_has_no_scratch_spills_or_lds():
    kernels, _ = kernel_remarks()
    new = {n: res for n, res in kernels.items() if "b2h_scatter_rows_blend_k" in n}
    assert len(new) == 1, sorted(new)
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)
    assert len([n for n in kernels if "b2h_scatter_rows_k" in n]) == 1             # the sibling's filter still finds only it


def test_new_kernel_name_matches_no_filter_of_the_other_test_files():
    filters = ("b2h_build_batch_k", "b2h_embed_dwords", "b2h_fwd", "b2h_attn", "b2h_tenc_chain", "b2h_epoch", "b2h_tpt_",
               "b2h_tt_", "b2h_lt_", "b2h_mt_", "b2h_ml_", "b2h_mw_", "b2h_tptt_", "b2h_train_", "b2h_l1_backward",
               "b2h_adam_step_k", "b2h_dropout_masks_k", "b2h_scatter_rows_k", "b2h_joint_error_k", "b2h_joint_total_k")
    assert not [f for f in filters if f in "b2h_scatter_rows_blend_k"]
