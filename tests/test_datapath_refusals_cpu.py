"""(CPU) The host refusals of the entry points whose operands are checked through one table (check_ops of b2h_api.hip):
b2h_build_batch, _planned and _aug, b2h_scatter_rows and _blend, b2h_epoch_plan, b2h_joint_error, and b2h_epoch_record
beside them.  A sweep: every pointer operand in turn NULL, 4 bytes off its alignment, laid over the first output; every
empty shape alone and with each of these.  (status, message) of every case is compared with
golden/datapath_refusals.json, recorded from the library BEFORE the tables were merged, so the order of the checks, the
per-operand alignment and the part a zero-byte operand plays in the overlap check are pinned as callers saw them.

    python tests/test_datapath_refusals_cpu.py <libb2h.so>     prints the cases of that library as JSON lines"""
import ctypes
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hand_pose_sl_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datapath_refusals.json")
vp = ctypes.c_void_p
AUG = _lib.AugmentStruct(0.1, 0.1, 0.5, 0.01)


def _addresses(names):
    return {k: 0x10000000 * (i + 1) for i, k in enumerate(names)}


def _p(a, k):
    return None if a[k] is None else vp(a[k])


# name -> (symbol, pointer operands in table order, the first output, scalar defaults, empty shapes, the call)
BATCH = dict(n_rows=100, n_utt=5, n_body=12, S=9, B=3, T=7, predict=0, flags=3, factor=1280.0, n_plan=8, entry0=0)
BATCH_OUT = ("input_kp", "target_kp", "target_conf", "text_tokens", "n_frames")
EMPTY_BATCH = (dict(B=0), dict(T=0), dict(n_utt=0), dict(n_rows=0), dict(n_plan=0))
ENTRIES = {
    "build_batch": ("b2h_build_batch", ("rows", "offsets", "tokens", "utt", "start") + BATCH_OUT, "input_kp", BATCH, EMPTY_BATCH,
                    lambda a: (_p(a, "rows"), a["n_rows"], _p(a, "offsets"), a["n_utt"], a["n_body"], _p(a, "tokens"), a["S"],
                               _p(a, "utt"), _p(a, "start"), a["B"], a["T"], a["predict"], a["flags"], a["factor"],
                               *[_p(a, k) for k in BATCH_OUT], None)),
    "build_batch_planned": ("b2h_build_batch_planned", ("rows", "offsets", "tokens", "utt", "start", "step") + BATCH_OUT,
                            "input_kp", BATCH, EMPTY_BATCH,
                            lambda a: (_p(a, "rows"), a["n_rows"], _p(a, "offsets"), a["n_utt"], a["n_body"], _p(a, "tokens"),
                                       a["S"], _p(a, "utt"), _p(a, "start"), a["n_plan"], _p(a, "step"), a["B"], a["T"],
                                       a["predict"], a["flags"], a["factor"], *[_p(a, k) for k in BATCH_OUT], None)),
    "build_batch_aug": ("b2h_build_batch_aug", ("rows", "offsets", "tokens", "utt", "start", "step", "key") + BATCH_OUT,
                        "input_kp", BATCH, EMPTY_BATCH,
                        lambda a: (_p(a, "rows"), a["n_rows"], _p(a, "offsets"), a["n_utt"], a["n_body"], _p(a, "tokens"), a["S"],
                                   _p(a, "utt"), _p(a, "start"), a["n_plan"], _p(a, "step"), a["entry0"], ctypes.byref(AUG),
                                   _p(a, "key"), a["B"], a["T"], a["predict"], a["flags"], a["factor"],
                                   *[_p(a, k) for k in BATCH_OUT], None)),
    "scatter_rows": ("b2h_scatter_rows", ("rows", "offsets", "utt", "start", "skip", "pred", "rows_out"), "rows_out",
                     dict(BATCH, conf=1.0), EMPTY_BATCH[:4],
                     lambda a: (_p(a, "rows"), a["n_rows"], _p(a, "offsets"), a["n_utt"], a["n_body"], _p(a, "utt"),
                                _p(a, "start"), _p(a, "skip"), a["B"], a["T"], a["predict"], a["flags"], a["factor"],
                                _p(a, "pred"), a["conf"], _p(a, "rows_out"), None)),
    "scatter_rows_blend": ("b2h_scatter_rows_blend", ("rows", "offsets", "utt", "start", "skip", "pred", "pred_before", "rows_out"),
                           "rows_out", dict(BATCH, conf=1.0, blend=0), EMPTY_BATCH,
                           lambda a: (_p(a, "rows"), a["n_rows"], _p(a, "offsets"), a["n_utt"], a["n_body"], _p(a, "utt"),
                                      _p(a, "start"), _p(a, "skip"), a["n_plan"], a["entry0"], a["B"], a["T"], a["predict"],
                                      a["flags"], a["factor"], _p(a, "pred"), _p(a, "pred_before"), a["blend"], a["conf"],
                                      _p(a, "rows_out"), None)),
    "epoch_plan": ("b2h_epoch_plan", ("offsets", "utt_plan", "start_plan"), "utt_plan",
                   dict(n_utt=5, T=7, shuffle=1, random_crop=1), (dict(n_utt=0), dict(T=0), dict(random_crop=0)),
                   lambda a: (_p(a, "offsets"), a["n_utt"], a["T"], a["shuffle"], a["random_crop"], 3, 1, _p(a, "utt_plan"),
                              _p(a, "start_plan"), None)),
    "epoch_record": ("b2h_epoch_record", ("loss", "losses", "step"), "losses", dict(n_losses=6), (dict(n_losses=0),),
                     lambda a: (_p(a, "loss"), _p(a, "losses"), a["n_losses"], _p(a, "step"), None)),
    "joint_error": ("b2h_joint_error", ("rows_pred", "rows_true", "offsets", "utt_sum", "utt_count", "total_sum", "total_count"),
                    "utt_sum", dict(n_rows=100, n_utt=5, n_body=12), (dict(n_utt=0), dict(n_rows=0), dict(n_utt=0, n_rows=0)),
                    lambda a: (_p(a, "rows_pred"), _p(a, "rows_true"), a["n_rows"], _p(a, "offsets"), a["n_utt"], a["n_body"],
                               _p(a, "utt_sum"), _p(a, "utt_count"), _p(a, "total_sum"), _p(a, "total_count"), None)),
}


def sweep(name):
    """[(case id, keyword changes)] of one entry point."""
    _, operands, first_out, _, empties, _ = ENTRIES[name]
    at = _addresses(operands)
    second_out = operands[operands.index(first_out) + 1] if first_out != operands[-1] else None
    moves = [("plain", {})]
    for k in operands:
        moves.append((k + "=NULL", {k: None}))
        moves.append((k + "+4", {k: at[k] + 4}))
        if k != first_out:
            moves.append((k + "@" + first_out, {k: at[first_out] + 8}))     # 8 bytes inside it: also for a zero-byte operand
        elif second_out:
            moves.append((k + "@" + second_out, {k: at[second_out] + 8}))
    cases = list(moves)
    for e in empties:
        tag = ",".join(f"{k}={v}" for k, v in e.items())
        cases += [(tag + " " + i, dict(kw, **e)) for i, kw in moves]
    return cases


def run(lib, name):
    """{case id: [status, message]}; the message only of a refusal the host made (not of the HIP runtime's answer)."""
    symbol, operands, _, scalars, _, call = ENTRIES[name]
    fn = getattr(lib, symbol)
    fn.restype, fn.argtypes = _lib.SYMBOLS[symbol]
    lib.b2h_last_error.restype = ctypes.c_char_p
    out = {}
    for case, kw in sweep(name):
        a = dict(_addresses(operands), **scalars)
        a.update(kw)
        status = fn(*call(a))
        host = status in (_lib.ERR_INVALID, _lib.ERR_SHAPE)
        out[case] = [status, lib.b2h_last_error().decode() if host else ""]
    return out


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_sweep_equals_the_record_of_the_library_before_the_tables_were_merged(name):
    import torch
    want = json.load(open(GOLDEN))[name]
    got = run(_lib.load(), name)
    assert sorted(got) == sorted(want)
    gpu = torch.cuda.is_available()
    differing = {}
    for case, (status, message) in want.items():
        if status == _lib.ERR_HIP and gpu:
            # past every host check: without a GPU the runtime's first answer, with one a pointer that is no device memory
            if got[case][0] != _lib.ERR_INVALID or "device" not in got[case][1]:
                differing[case] = (want[case], got[case])
        elif got[case] != [status, message]:
            differing[case] = (want[case], got[case])
    assert not differing, differing
    assert len(want) >= 20 and any(s == _lib.ERR_INVALID for s, _ in want.values())


if __name__ == "__main__":
    library = ctypes.CDLL(os.path.abspath(sys.argv[1]))
    for entry in sorted(ENTRIES):
        for case_id, result in sorted(run(library, entry).items()):
            print(json.dumps([entry, case_id] + result))
