"""The device-resident training set without a GPU: the new entry point in the header, the ctypes table and the library;
every host refusal of b2h_build_batch before any device work; the torch restatement tests/batch_ref.py against the
fixtures made from the reference's own datasets and transforms (tests/golden/make_golden_batches.py), bit for bit; the
host-side packer and the validation of DeviceDataset / DeviceLoader; the kernel's resource usage."""
import ctypes
import os

import numpy as np
import pytest
import torch

import batch_ref
import hand_pose_sl_amd as hps
from conftest import ROOT
from hand_pose_sl_amd import _lib, dataset
from kernel_remarks import kernel_remarks

OK, INVALID, SHAPE = _lib.OK, _lib.ERR_INVALID, _lib.ERR_SHAPE


def test_entry_point_declared_typed_and_exported():
    header = " ".join(open(os.path.join(ROOT, "include", "b2h.h")).read().split())
    decl = ("int b2h_build_batch(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body, "
            "const int64_t* tokens, int64_t S, const int64_t* utt, const int64_t* start, int64_t B, int64_t T, int predict, "
            "int flags, float factor, float* input_kp, float* target_kp, float* target_conf, int64_t* text_tokens, "
            "int64_t* n_frames, void* stream);")
    assert decl in header
    assert "enum b2h_batch_flags { B2H_BATCH_DIF_ENCODING = 1, B2H_BATCH_NORMALIZE = 2, B2H_BATCH_PAD_FRAME0 = 4 };" in header
    assert (_lib.BATCH_DIF_ENCODING, _lib.BATCH_NORMALIZE, _lib.BATCH_PAD_FRAME0) == (1, 2, 4)
    res, args = _lib.SYMBOLS["b2h_build_batch"]
    assert res is ctypes.c_int and len(args) == 20
    assert hasattr(_lib.load(), "b2h_build_batch")
    assert {"DeviceDataset", "DeviceLoader", "train_epoch"} <= set(hps.__all__)


# ---- refusals -------------------------------------------------------------------------------------------------------
# Made-up, well-separated, 8-byte-aligned addresses that nothing dereferences: a call that got past the host checks
# would ask the HIP runtime about them and fail with another status.
_A = {k: 0x10000000 * (i + 1) for i, k in enumerate(
    ("rows", "offsets", "tokens", "utt", "start", "input_kp", "target_kp", "target_conf", "text_tokens", "n_frames"))}


def _call(**kw):
    a = dict(_A, n_rows=100, n_utt=5, n_body=12, S=5, B=3, T=7, predict=0, flags=3, factor=1280.0)
    a.update(kw)
    p = lambda k: None if a[k] is None else ctypes.c_void_p(a[k])
    return _lib.load().b2h_build_batch(p("rows"), a["n_rows"], p("offsets"), a["n_utt"], a["n_body"], p("tokens"), a["S"],
                                       p("utt"), p("start"), a["B"], a["T"], a["predict"], a["flags"], a["factor"],
                                       p("input_kp"), p("target_kp"), p("target_conf"), p("text_tokens"), p("n_frames"), None)


REFUSALS = [
    (dict(n_body=10), INVALID, "n_body"), (dict(n_body=0), INVALID, "n_body"),
    (dict(predict=3), INVALID, "predict"), (dict(predict=-1), INVALID, "predict"),
    (dict(predict=1, n_body=8), INVALID, "n_body = 12"), (dict(predict=2, n_body=8), INVALID, "n_body = 12"),
    (dict(flags=8), INVALID, "flag"), (dict(flags=-1), INVALID, "flag"),
    (dict(factor=0.0), INVALID, "factor"), (dict(factor=-1.0), INVALID, "factor"), (dict(factor=float("nan")), INVALID, "factor"),
    (dict(S=0), INVALID, "S"), (dict(S=129), INVALID, "S"),
    (dict(tokens=None), INVALID, "both or neither"), (dict(text_tokens=None), INVALID, "both or neither"),
    (dict(B=-1), SHAPE, "negative"), (dict(T=-1), SHAPE, "negative"), (dict(n_utt=-1), SHAPE, "negative"),
    (dict(n_rows=-1), SHAPE, "negative"),
    (dict(T=(1 << 24) + 1), SHAPE, "too large"), (dict(B=1 << 31), SHAPE, "too large"),
    (dict(rows=None), INVALID, "rows is NULL"), (dict(offsets=None), INVALID, "offsets is NULL"),
    (dict(utt=None), INVALID, "utt is NULL"), (dict(input_kp=None), INVALID, "input_kp is NULL"),
    (dict(target_kp=None), INVALID, "target_kp is NULL"), (dict(n_frames=None), INVALID, "n_frames is NULL"),
] + [(dict([(k, _A[k] + 4)]), INVALID, k + " must be 8-byte aligned") for k in _A] + [
    (dict(input_kp=_A["rows"] + 8), INVALID, "overlaps rows"),
    (dict(n_frames=_A["rows"] + 100 * 162 * 4 - 8), INVALID, "overlaps rows"),       # the store's last word
    (dict(target_kp=_A["offsets"] + 40), INVALID, "overlaps offsets"),
    (dict(target_conf=_A["tokens"] + 5 * 5 * 8 - 8), INVALID, "overlaps tokens"),
    (dict(text_tokens=_A["utt"] + 16), INVALID, "overlaps utt"),
    (dict(n_frames=_A["start"]), INVALID, "overlaps start"),
    (dict(target_kp=_A["input_kp"] + 3 * 7 * 12 * 8 - 8), INVALID, "two outputs overlap"),
    (dict(target_conf=_A["n_frames"] + 8), INVALID, "two outputs overlap"),
]


@pytest.mark.parametrize("kw,status,message", REFUSALS, ids=[f"{i}-{m.replace(' ', '_')}" for i, (_, _, m) in enumerate(REFUSALS)])
def test_host_refusal(kw, status, message):
    assert _call(**kw) == status
    assert message in _lib.last_error()


def test_no_ops_and_optional_operands():
    lib = _lib.load()
    none = [None] * 5
    # B * T == 0: nothing is looked at, after the argument checks
    assert lib.b2h_build_batch(None, 0, None, 0, 8, None, 0, None, None, 0, 7, 0, 0, 1.0, *none, None) == OK
    assert lib.b2h_build_batch(None, 0, None, 0, 8, None, 0, None, None, 4, 0, 0, 0, 1.0, *none, None) == OK
    assert lib.b2h_build_batch(None, 0, None, 0, 9, None, 0, None, None, 0, 7, 0, 0, 1.0, *none, None) == INVALID
    if not torch.cuda.is_available():
        # start, target_conf and the token pair may be left out, an empty store has no rows to point at, an output may
        # end where the store begins: these get past every host check, to the first question to the HIP runtime
        for kw in (dict(start=None), dict(target_conf=None), dict(tokens=None, text_tokens=None, S=0),
                   dict(rows=None, n_rows=0), dict(input_kp=_A["rows"] - 3 * 7 * 12 * 8),
                   dict(n_frames=_A["rows"] + 100 * 162 * 4), dict(factor=0.0, flags=5)):
            assert _call(**kw) == _lib.ERR_HIP, (kw, _lib.last_error())


# ---- the restatement against the reference's batches -----------------------------------------------------------------
def test_fixtures_cover_the_issue():
    assert batch_ref.fixture_names() == ["h5_store", "json_store"]
    h5, js = batch_ref.load_fixture("h5_store"), batch_ref.load_fixture("json_store")
    assert (h5["n_body"], h5["T"], h5["S"], h5["selections"]) == (8, 7, 5, ["first"])
    assert (js["n_body"], js["T"], js["S"], js["selections"]) == (12, 7, 5, ["first", "randomcrop"])
    assert (h5["store"][1][1:] - h5["store"][1][:-1]).tolist() == [0, 1, 3, 7, 8, 19]
    assert (js["store"][1][1:] - js["store"][1][:-1]).tolist() == [1, 3, 7, 8, 19]
    assert len(h5["expected"]) == 4 * 3 and len(js["expected"]) == 12 * 2 * 3
    for rec in (h5, js):
        rows = rec["store"][0].reshape(-1, 3, rec["n_body"] + 42)
        assert float(rows[:, :2].max()) > 1000 and 0 <= float(rows[:, 2].min()) and float(rows[:, 2].max()) <= 1   # pixels, [0, 1]
        assert rec["lists"]["c"].tolist() == sorted(rec["lists"]["c"].tolist(), reverse=True)     # descending, one id twice
        assert len(set(rec["lists"]["c"].tolist())) < len(rec["lists"]["c"])
    drawn = torch.cat([js["starts"][("randomcrop", ln)] for ln in js["lists"]])
    assert int(drawn.max()) > 0                                               # a crop that does not start at 0


@pytest.mark.parametrize("name", ["h5_store", "json_store"])
def test_restatement_reproduces_every_fixture_bit_for_bit(name):
    rec = batch_ref.load_fixture(name)
    rows, offsets, n_body, tokens = rec["store"]
    assert rec["expected"]
    for (predict, dif, norm, sel, ln), want in rec["expected"].items():
        got = batch_ref.batch(rows, offsets, n_body, tokens, rec["lists"][ln], rec["starts"][(sel, ln)], rec["T"], predict,
                              bool(dif), bool(norm), 1280, rec["frame0"])
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]) and batch_ref.same_bits(got[k], want[k]), (predict, dif, norm, sel, ln, k)


def test_restatement_clamps_starts_and_ignores_them_in_short_utterances():
    rec = batch_ref.load_fixture("json_store")
    rows, offsets, n_body, tokens = rec["store"]
    utt = torch.tensor([4, 4, 4, 2, 1])                    # 19, 19, 19, 7 and 3 frames at T = 7
    a = batch_ref.batch(rows, offsets, n_body, tokens, utt, torch.tensor([-5, 12, 99, 3, 2]), 7, frame0=True)
    b = batch_ref.batch(rows, offsets, n_body, tokens, utt, torch.tensor([0, 12, 12, 0, 0]), 7, frame0=True)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["input_kp"][0], a["input_kp"][1])


def test_packer_reproduces_the_store_rows_of_the_json_fixture():
    rec = batch_ref.load_fixture("json_store")
    packed = np.concatenate([dataset.frames_to_rows(u) for u in rec["frames"]], axis=0)
    assert packed.dtype == np.float32 and np.array_equal(packed, rec["store"][0].numpy())
    # wrapped as merged-JSON entries: the same rows
    merged = [{"json_path": f"f{i}.json", "json_data": fr} for i, fr in enumerate(rec["frames"][2])]
    assert np.array_equal(dataset.frames_to_rows(merged), dataset.frames_to_rows(rec["frames"][2]))
    # the 8-joint row codec that exists is this layout at n_body 8: h5_row_to_item splits a store row into its parts
    h5 = batch_ref.load_fixture("h5_store")
    it = hps.openpose.h5_row_to_item(h5["store"][0].numpy()[:4])
    assert np.array_equal(hps.openpose.item_to_h5_row(it["body_kp"], it["left_hand_kp"], it["right_hand_kp"], it["body_conf"],
                                                      it["left_hand_conf"], it["right_hand_conf"]), h5["store"][0].numpy()[:4])


# ---- DeviceDataset / DeviceLoader validate on the host ----------------------------------------------------------------
def test_device_dataset_rejects_a_bad_store():
    rows = torch.zeros((6, 150))
    good = torch.tensor([0, 2, 2, 6])
    for bad in ([0, 4, 2, 6], [0, 2, 6, 5], [1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 4, 7]):
        with pytest.raises(ValueError, match="ascend"):
            hps.DeviceDataset(rows, torch.tensor(bad), 8)
    with pytest.raises(ValueError, match=r"\(N, 162\)"):
        hps.DeviceDataset(rows, good, 12)                           # a 150-wide row is not a 12-joint store
    with pytest.raises(ValueError, match=r"\(N, 150\)"):
        hps.DeviceDataset(torch.zeros((6, 162)), good, 8)
    with pytest.raises(ValueError, match="n_body"):
        hps.DeviceDataset(rows, good, 10)
    with pytest.raises(ValueError, match="float32"):
        hps.DeviceDataset(rows.double(), good, 8)
    with pytest.raises(ValueError, match="int64"):
        hps.DeviceDataset(rows, good.int(), 8)
    for tok in (torch.zeros((2, 5), dtype=torch.int64), torch.zeros((3, 0), dtype=torch.int64),
                torch.zeros((3, 129), dtype=torch.int64), torch.zeros((3,), dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"tokens must be \(3, S\)"):
            hps.DeviceDataset(rows, good, 8, tokens=tok)
    with pytest.raises(ValueError, match="tokens must be int64"):
        hps.DeviceDataset(rows, good, 8, tokens=torch.zeros((3, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\(n_frames, 150\)"):
        hps.DeviceDataset.from_h5_rows([np.zeros((3, 162), np.float32)])
    with pytest.raises(RuntimeError, match="GPU"):
        hps.DeviceDataset(rows, good, 8, device="cpu")              # no host fallback


# ---- the kernel -------------------------------------------------------------------------------------------------------
def test_kernel_has_no_scratch_spills_or_lds():
    kernels, _ = kernel_remarks()
    new = {n: res for n, res in kernels.items() if "b2h_build_batch_k" in n}
    assert len(new) == 1, sorted(new)
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)
