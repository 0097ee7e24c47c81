"""Captured training epochs without a GPU: the three new entry points in the header, the ctypes table and the library;
their host refusals before any device work; the restatement tests/plan_ref.py of the epoch plan -- a bijection at every
size, different per epoch and seed, every crop start in range --; the kernels' resource usage."""
import ctypes
import os

import pytest
import torch

import hand_pose_sl_amd as hps
import plan_ref
from conftest import ROOT
from hand_pose_sl_amd import _lib
from kernel_remarks import kernel_remarks

OK, INVALID, SHAPE, HIP = _lib.OK, _lib.ERR_INVALID, _lib.ERR_SHAPE, _lib.ERR_HIP


def test_entry_points_declared_typed_and_exported():
    header = " ".join(open(os.path.join(ROOT, "include", "b2h.h")).read().split())
    for decl in (
            "int b2h_epoch_plan(const int64_t* offsets, int64_t n_utt, int64_t T, int shuffle, int random_crop, uint64_t seed, "
            "uint64_t epoch, int64_t* utt_plan, int64_t* start_plan, void* stream);",
            "int b2h_build_batch_planned(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body, "
            "const int64_t* tokens, int64_t S, const int64_t* utt_plan, const int64_t* start_plan, int64_t n_plan, "
            "const int64_t* step, int64_t B, int64_t T, int predict, int flags, float factor, float* input_kp, "
            "float* target_kp, float* target_conf, int64_t* text_tokens, int64_t* n_frames, void* stream);",
            "int b2h_epoch_record(const float* loss, float* losses, int64_t n_losses, int64_t* step, void* stream);"):
        assert decl in header, decl
    lib = _lib.load()
    for name, n_args in (("b2h_epoch_plan", 10), ("b2h_build_batch_planned", 22), ("b2h_epoch_record", 5)):
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == n_args, name
        assert hasattr(lib, name), name
    # the planned build is b2h_build_batch's argument list with utt_plan / start_plan, plus n_plan and step
    plain, planned = _lib.SYMBOLS["b2h_build_batch"][1], _lib.SYMBOLS["b2h_build_batch_planned"][1]
    assert planned[:9] == plain[:9] and planned[9:11] == [ctypes.c_int64, ctypes.c_void_p] and planned[11:] == plain[9:]
    assert "GraphTrainer" in hps.__all__


# ---- refusals: made-up, well-separated, aligned addresses that nothing dereferences ------------------------------------
_P = {"offsets": 0x10000000, "utt_plan": 0x20000000, "start_plan": 0x30000000}


def _plan(**kw):
    a = dict(_P, n_utt=6, T=7, shuffle=1, random_crop=1, seed=3, epoch=0)
    a.update(kw)
    p = lambda k: None if a[k] is None else ctypes.c_void_p(a[k])
    return _lib.load().b2h_epoch_plan(p("offsets"), a["n_utt"], a["T"], a["shuffle"], a["random_crop"], a["seed"], a["epoch"],
                                      p("utt_plan"), p("start_plan"), None)


PLAN_REFUSALS = [
    (dict(n_utt=-1), SHAPE, "negative"), (dict(T=-1), SHAPE, "negative"), (dict(n_utt=(1 << 30) + 1), SHAPE, "too large"),
    (dict(shuffle=2), INVALID, "0 or 1"), (dict(random_crop=-1), INVALID, "0 or 1"),
    (dict(utt_plan=None), INVALID, "utt_plan is NULL"), (dict(start_plan=None), INVALID, "start_plan is NULL"),
    (dict(offsets=None), INVALID, "offsets is NULL"),
    (dict(offsets=_P["offsets"] + 4), INVALID, "offsets must be 8-byte aligned"),
    (dict(utt_plan=_P["utt_plan"] + 4), INVALID, "utt_plan must be 8-byte aligned"),
    (dict(start_plan=_P["start_plan"] + 2), INVALID, "start_plan must be 8-byte aligned"),
    (dict(start_plan=_P["utt_plan"] + 40), INVALID, "two outputs overlap"),                  # the plan's last entry
    (dict(utt_plan=_P["offsets"] + 48), INVALID, "overlaps offsets"),                        # offsets has n_utt + 1 entries
    (dict(start_plan=_P["offsets"] - 40), INVALID, "overlaps offsets"),
]


@pytest.mark.parametrize("kw,status,message", PLAN_REFUSALS, ids=[f"{i}-{m.replace(' ', '_')}" for i, (_, _, m) in enumerate(PLAN_REFUSALS)])
def test_epoch_plan_host_refusal(kw, status, message):
    assert _plan(**kw) == status
    assert message in _lib.last_error()


def test_epoch_plan_no_ops_and_optional_operands():
    assert _plan(n_utt=0) == OK and _plan(n_utt=0, utt_plan=None, start_plan=None, offsets=None, random_crop=0) == OK
    if not torch.cuda.is_available():
        # past every host check, to the first question to the HIP runtime: start_plan and offsets left out without
        # random_crop, buffers that touch without overlapping
        for kw in (dict(), dict(random_crop=0, start_plan=None), dict(random_crop=0, offsets=None),
                   dict(utt_plan=_P["offsets"] + 56), dict(start_plan=_P["utt_plan"] + 48)):
            assert _plan(**kw) == HIP, (kw, _lib.last_error())


_B = {k: 0x10000000 * (i + 1) for i, k in enumerate(
    ("rows", "offsets", "tokens", "utt_plan", "start_plan", "step", "input_kp", "target_kp", "target_conf", "text_tokens", "n_frames"))}


def _planned(**kw):
    a = dict(_B, n_rows=100, n_utt=5, n_body=12, S=5, n_plan=5, B=3, T=7, predict=0, flags=3, factor=1280.0)
    a.update(kw)
    p = lambda k: None if a[k] is None else ctypes.c_void_p(a[k])
    return _lib.load().b2h_build_batch_planned(
        p("rows"), a["n_rows"], p("offsets"), a["n_utt"], a["n_body"], p("tokens"), a["S"], p("utt_plan"), p("start_plan"),
        a["n_plan"], p("step"), a["B"], a["T"], a["predict"], a["flags"], a["factor"], p("input_kp"), p("target_kp"),
        p("target_conf"), p("text_tokens"), p("n_frames"), None)


PLANNED_REFUSALS = [
    (dict(n_body=10), INVALID, "n_body"), (dict(predict=3), INVALID, "predict"), (dict(flags=8), INVALID, "flag"),
    (dict(factor=0.0), INVALID, "factor"), (dict(S=129), INVALID, "S"), (dict(tokens=None), INVALID, "both or neither"),
    (dict(B=-1), SHAPE, "negative"), (dict(n_plan=-1), SHAPE, "negative"), (dict(n_plan=(1 << 40) + 1), SHAPE, "too large"),
    (dict(utt_plan=None), INVALID, "utt_plan is NULL"), (dict(step=None), INVALID, "step is NULL"),
    (dict(n_frames=None), INVALID, "n_frames is NULL"),
    (dict(utt_plan=_B["utt_plan"] + 4), INVALID, "utt_plan must be 8-byte aligned"),
    (dict(start_plan=_B["start_plan"] + 4), INVALID, "start_plan must be 8-byte aligned"),
    (dict(step=_B["step"] + 4), INVALID, "step must be 8-byte aligned"),
    (dict(input_kp=_B["input_kp"] + 4), INVALID, "input_kp must be 8-byte aligned"),
    (dict(n_frames=_B["utt_plan"] + 32), INVALID, "overlaps utt_plan"),                      # the plan's fifth entry: past B
    (dict(text_tokens=_B["start_plan"] + 32), INVALID, "overlaps start_plan"),
    (dict(n_frames=_B["step"]), INVALID, "overlaps step"),
    (dict(target_kp=_B["rows"] + 8), INVALID, "overlaps rows"),
    (dict(target_conf=_B["n_frames"] + 8), INVALID, "two outputs overlap"),
]


@pytest.mark.parametrize("kw,status,message", PLANNED_REFUSALS, ids=[f"{i}-{m.replace(' ', '_')}" for i, (_, _, m) in enumerate(PLANNED_REFUSALS)])
def test_planned_build_host_refusal(kw, status, message):
    assert _planned(**kw) == status
    assert message in _lib.last_error()


def test_planned_build_no_ops_and_optional_operands():
    assert _planned(B=0) == OK and _planned(T=0) == OK
    if not torch.cuda.is_available():
        for kw in (dict(), dict(start_plan=None), dict(n_plan=0, utt_plan=None, start_plan=None),
                   dict(n_frames=_B["utt_plan"] + 40), dict(n_frames=_B["step"] + 8)):
            assert _planned(**kw) == HIP, (kw, _lib.last_error())


_R = {"loss": 0x10000000, "losses": 0x20000000, "step": 0x30000000}


def _record(**kw):
    a = dict(_R, n_losses=4)
    a.update(kw)
    p = lambda k: None if a[k] is None else ctypes.c_void_p(a[k])
    return _lib.load().b2h_epoch_record(p("loss"), p("losses"), a["n_losses"], p("step"), None)


RECORD_REFUSALS = [
    (dict(n_losses=-1), SHAPE, "negative"),
    (dict(loss=None), INVALID, "loss is NULL"), (dict(losses=None), INVALID, "losses is NULL"), (dict(step=None), INVALID, "step is NULL"),
    (dict(loss=_R["loss"] + 2), INVALID, "4-byte aligned"), (dict(losses=_R["losses"] + 1), INVALID, "4-byte aligned"),
    (dict(step=_R["step"] + 4), INVALID, "step must be 8-byte aligned"),
    (dict(loss=_R["losses"] + 12), INVALID, "overlaps loss"), (dict(loss=_R["step"] + 4), INVALID, "overlaps loss"),
    (dict(step=_R["losses"] + 8), INVALID, "two outputs overlap"),
]


@pytest.mark.parametrize("kw,status,message", RECORD_REFUSALS, ids=[f"{i}-{m.replace(' ', '_')}" for i, (_, _, m) in enumerate(RECORD_REFUSALS)])
def test_epoch_record_host_refusal(kw, status, message):
    assert _record(**kw) == status
    assert message in _lib.last_error()


def test_epoch_record_optional_operands():
    if not torch.cuda.is_available():
        for kw in (dict(), dict(n_losses=0, losses=None), dict(loss=_R["losses"] + 16), dict(step=_R["losses"] + 16)):
            assert _record(**kw) == HIP, (kw, _lib.last_error())


# ---- the plan's restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(range(1, 71)) + [1000, 4097])
def test_restated_order_is_a_bijection(n):
    for seed, epoch in ((0, 0), (0x123456789ABCDEF, 5)):
        assert sorted(plan_ref.order(n, True, seed, epoch)) == list(range(n)), (seed, epoch)
    assert plan_ref.order(n, False, 9, 9) == list(range(n))


def test_restated_half_width():
    assert [plan_ref.half_width(n) for n in (1, 2, 4, 5, 16, 17, 64, 65, 4096, 4097, 1 << 30)] == [1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 15]


def test_restated_order_differs_between_epochs_and_seeds():
    a = plan_ref.order(70, True, 1, 0)
    assert a != list(range(70))
    assert a != plan_ref.order(70, True, 1, 1) and a != plan_ref.order(70, True, 2, 0)
    assert a == plan_ref.order(70, True, 1, 0)                                    # and is a function of them
    assert a != plan_ref.order(70, True, 1, 1 << 32) and a != plan_ref.order(70, True, 1 << 32 | 1, 0)   # the high halves count


def test_restated_starts_stay_in_range():
    lengths = [0, 1, 6, 7, 8, 19, 500]
    offsets = [0]
    for v in lengths:
        offsets.append(offsets[-1] + v)
    T, seen = 7, {i: set() for i in range(len(lengths))}
    for epoch in range(40):
        utt, start = plan_ref.plan(offsets, len(lengths), T, True, True, 7, epoch)
        for u, s in zip(utt, start):
            assert 0 <= s <= max(lengths[u] - T, 0), (u, s)
            seen[u].add(s)
    assert all(seen[u] == {0} for u in range(4))                                  # the utterance fits: 0
    assert seen[4] == {0, 1} and len(seen[5]) >= 10 and max(seen[6]) > 400        # both ends of a room of 1; spread
    assert plan_ref.starts(offsets, list(range(7)), T, False, 7, 0) == [0] * 7
    # a crop draw shares no Philox block with a Feistel round: the tags differ
    assert plan_ref.TAG_CROP not in range(plan_ref.TAG_ROUND0, plan_ref.TAG_ROUND0 + 4)


def test_trainer_refuses_a_host_loader_before_any_gpu_work():
    m = hps.ConvModel(30, "ReLU", False)
    with pytest.raises(ValueError, match="DeviceLoader"):
        hps.GraphTrainer(m, [{"body_kp": torch.zeros(1, 4, 12, 2)}], hps.Adam(m.parameters()))


# ---- the kernels -------------------------------------------------------------------------------------------------------
def test_kernels_have_no_scratch_spills_or_lds():
    kernels, _ = kernel_remarks()
    for kernel in ("b2h_epoch_plan_k", "b2h_epoch_record_k", "b2h_build_batch_k"):
        new = {n: res for n, res in kernels.items() if kernel in n}
        assert len(new) == 1, (kernel, sorted(new))
        for name, res in new.items():
            assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
            assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)
