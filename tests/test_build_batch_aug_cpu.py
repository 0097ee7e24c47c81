"""The augmented batch build without a GPU: b2h_build_batch_aug in the header, the ctypes table and the library; every
host refusal before any device work; `Augment`'s validation and its rotate_tan; the numpy restatement
tests/augment_ref.py -- the identity at zero parameters against tests/batch_ref.py on the committed fixtures, the
geometry of the rotation and scale, the mirror --; the kernel's resource usage.  The reference has no augmentation: the
definition is the project's own (include/b2h.h)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import augment_ref
import batch_ref
import hand_pose_sl_amd as hps
from conftest import ROOT
from hand_pose_sl_amd import _lib
from kernel_remarks import kernel_remarks

OK, INVALID, SHAPE, HIP = _lib.OK, _lib.ERR_INVALID, _lib.ERR_SHAPE, _lib.ERR_HIP


def test_entry_point_declared_typed_and_exported():
    header = " ".join(open(os.path.join(ROOT, "include", "b2h.h")).read().split())
    decl = ("int b2h_build_batch_aug(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body, "
            "const int64_t* tokens, int64_t S, const int64_t* utt, const int64_t* start, int64_t n_plan, const int64_t* step, "
            "int64_t entry0, const b2h_augment* aug, const uint64_t* key, int64_t B, int64_t T, int predict, int flags, "
            "float factor, float* input_kp, float* target_kp, float* target_conf, int64_t* text_tokens, int64_t* n_frames, "
            "void* stream);")
    assert decl in header
    assert "typedef struct b2h_augment {" in header and "} b2h_augment;" in header
    assert "#define B2H_VERSION 100 " in header and _lib.load().b2h_version() == 100
    res, args = _lib.SYMBOLS["b2h_build_batch_aug"]
    assert res is ctypes.c_int and len(args) == 25
    # the planned build's list with entry0, aug and key behind step
    planned = _lib.SYMBOLS["b2h_build_batch_planned"][1]
    assert args[:11] == planned[:11] and args[14:] == planned[11:]
    assert [f[0] for f in _lib.AugmentStruct._fields_] == ["scale", "rotate_tan", "mirror_p", "jitter"]
    assert ctypes.sizeof(_lib.AugmentStruct) == 16
    assert hasattr(_lib.load(), "b2h_build_batch_aug")
    assert "Augment" in hps.__all__


# ---- refusals -------------------------------------------------------------------------------------------------------
# Made-up, well-separated, 8-byte-aligned addresses that nothing dereferences (tests/test_build_batch_cpu.py): a call
# that got past the host checks would ask the HIP runtime about them and fail with another status.
_A = {k: 0x10000000 * (i + 1) for i, k in enumerate(
    ("rows", "offsets", "tokens", "utt", "start", "step", "key", "input_kp", "target_kp", "target_conf", "text_tokens",
     "n_frames"))}
_AUG = dict(scale=0.2, rotate_tan=0.1, mirror_p=0.5, jitter=3.0)
NO_AUG = object()


def _call(*more, **kw):
    a = dict(_A, n_rows=100, n_utt=5, n_body=12, S=5, n_plan=5, entry0=0, B=3, T=7, predict=0, flags=3, factor=1280.0, aug=_AUG)
    for m in more + (kw,):
        a.update(m)
    p = lambda k: None if a[k] is None else ctypes.c_void_p(a[k])
    aug = None if a["aug"] is NO_AUG else ctypes.byref(_lib.AugmentStruct(**dict(_AUG, **a["aug"])))
    return _lib.load().b2h_build_batch_aug(
        p("rows"), a["n_rows"], p("offsets"), a["n_utt"], a["n_body"], p("tokens"), a["S"], p("utt"), p("start"), a["n_plan"],
        p("step"), a["entry0"], aug, p("key"), a["B"], a["T"], a["predict"], a["flags"], a["factor"], p("input_kp"),
        p("target_kp"), p("target_conf"), p("text_tokens"), p("n_frames"), None)


_EAGER = dict(step=None)
NAN, INF = float("nan"), float("inf")
REFUSALS = [
    # what b2h_build_batch_planned refuses, with the step word ...
    (dict(n_body=10), INVALID, "n_body"), (dict(predict=3), INVALID, "predict"), (dict(predict=1, n_body=8), INVALID, "n_body = 12"),
    (dict(flags=8), INVALID, "flag"), (dict(factor=0.0), INVALID, "factor"), (dict(factor=NAN), INVALID, "factor"),
    (dict(S=0), INVALID, "S"), (dict(S=129), INVALID, "S"),
    (dict(tokens=None), INVALID, "both or neither"), (dict(text_tokens=None), INVALID, "both or neither"),
    (dict(B=-1), SHAPE, "negative"), (dict(T=-1), SHAPE, "negative"), (dict(n_utt=-1), SHAPE, "negative"),
    (dict(n_rows=-1), SHAPE, "negative"), (dict(n_plan=-1), SHAPE, "negative"),
    (dict(T=(1 << 24) + 1), SHAPE, "too large"), (dict(B=1 << 31), SHAPE, "too large"), (dict(n_plan=(1 << 40) + 1), SHAPE, "too large"),
    (dict(rows=None), INVALID, "rows is NULL"), (dict(offsets=None), INVALID, "offsets is NULL"),
    (dict(utt=None), INVALID, "utt_plan is NULL"), (dict(input_kp=None), INVALID, "input_kp is NULL"),
    (dict(target_kp=None), INVALID, "target_kp is NULL"), (dict(n_frames=None), INVALID, "n_frames is NULL"),
    (dict(utt=_A["utt"] + 4), INVALID, "utt_plan must be 8-byte aligned"),
    (dict(start=_A["start"] + 4), INVALID, "start_plan must be 8-byte aligned"),
    (dict(step=_A["step"] + 4), INVALID, "step must be 8-byte aligned"),
] + [(dict([(k, _A[k] + 4)]), INVALID, k + " must be 8-byte aligned")
     for k in ("rows", "offsets", "tokens", "input_kp", "target_kp", "target_conf", "text_tokens", "n_frames")] + [
    (dict(input_kp=_A["rows"] + 8), INVALID, "overlaps rows"),
    (dict(target_kp=_A["offsets"] + 40), INVALID, "overlaps offsets"),
    (dict(target_conf=_A["tokens"] + 5 * 5 * 8 - 8), INVALID, "overlaps tokens"),
    (dict(n_frames=_A["utt"] + 32), INVALID, "overlaps utt_plan"),                       # the plan's fifth entry: past B
    (dict(text_tokens=_A["start"] + 32), INVALID, "overlaps start_plan"),
    (dict(n_frames=_A["step"]), INVALID, "overlaps step"),
    (dict(target_kp=_A["input_kp"] + 3 * 7 * 12 * 8 - 8), INVALID, "two outputs overlap"),
    # ... and without it b2h_build_batch's: utt and start hold B entries under their own names
    (dict(_EAGER, n_body=0), INVALID, "n_body"), (dict(_EAGER, B=1 << 31), SHAPE, "too large"),
    (dict(_EAGER, utt=None), INVALID, "utt is NULL"), (dict(_EAGER, utt=_A["utt"] + 4), INVALID, "utt must be 8-byte aligned"),
    (dict(_EAGER, start=_A["start"] + 4), INVALID, "start must be 8-byte aligned"),
    (dict(_EAGER, text_tokens=_A["utt"] + 16), INVALID, "overlaps utt"), (dict(_EAGER, n_frames=_A["start"]), INVALID, "overlaps start"),
    # its own
    (dict(aug=NO_AUG), INVALID, "aug is NULL"), (dict(_EAGER, aug=NO_AUG), INVALID, "aug is NULL"),
    (dict(key=None), INVALID, "key is NULL"), (dict(_EAGER, key=None), INVALID, "key is NULL"),
    (dict(key=_A["key"] + 4), INVALID, "key must be 8-byte aligned"),
    (dict(n_frames=_A["key"] + 8), INVALID, "overlaps key"),                             # the epoch word
    (dict(key=_A["input_kp"] + 3 * 7 * 12 * 8 - 8), INVALID, "overlaps key"),            # the seed word in input_kp's last
    (dict(aug=dict(scale=-0.1)), INVALID, "aug.scale"), (dict(aug=dict(scale=1.0)), INVALID, "aug.scale"),
    (dict(aug=dict(scale=NAN)), INVALID, "aug.scale"), (dict(aug=dict(scale=INF)), INVALID, "aug.scale"),
    (dict(aug=dict(rotate_tan=-0.1)), INVALID, "aug.rotate_tan"), (dict(aug=dict(rotate_tan=1.5)), INVALID, "aug.rotate_tan"),
    (dict(aug=dict(rotate_tan=NAN)), INVALID, "aug.rotate_tan"),
    (dict(aug=dict(mirror_p=-0.5)), INVALID, "aug.mirror_p"), (dict(aug=dict(mirror_p=1.25)), INVALID, "aug.mirror_p"),
    (dict(aug=dict(mirror_p=NAN)), INVALID, "aug.mirror_p"),
    (dict(aug=dict(jitter=-1.0)), INVALID, "aug.jitter"), (dict(aug=dict(jitter=INF)), INVALID, "aug.jitter"),
    (dict(aug=dict(jitter=NAN)), INVALID, "aug.jitter"), (dict(_EAGER, aug=dict(jitter=NAN)), INVALID, "aug.jitter"),
    (dict(n_plan=(1 << 32) + 1), SHAPE, "n_plan <= 2^32"),
    (dict(_EAGER, entry0=-1), SHAPE, "entry0"), (dict(_EAGER, entry0=(1 << 32) - 2), SHAPE, "entry0"),
    (dict(entry0=-1), SHAPE, "entry0"),
]


@pytest.mark.parametrize("kw,status,message", REFUSALS, ids=[f"{i}-{m.replace(' ', '_')}" for i, (_, _, m) in enumerate(REFUSALS)])
def test_host_refusal(kw, status, message):
    assert _call(**kw) == status
    assert message in _lib.last_error()


def test_no_ops_and_what_gets_past_the_host_checks():
    assert _call(B=0) == OK and _call(T=0) == OK and _call(_EAGER, B=0) == OK
    assert _call(B=0, aug=dict(scale=1.0)) == INVALID                 # the description is checked before the no-op
    if not torch.cuda.is_available():
        # the limits themselves, a step word or none, a plan not looked at without one, every parameter at its edge:
        # past every host check, to the first question to the HIP runtime
        for kw in (dict(), _EAGER, dict(start=None), dict(_EAGER, start=None), dict(_EAGER, n_plan=-7),
                   dict(n_plan=1 << 32, utt=1 << 48, start=1 << 49), dict(_EAGER, entry0=(1 << 32) - 3), dict(target_conf=None),
                   dict(aug=dict(scale=0.0, rotate_tan=0.0, mirror_p=0.0, jitter=0.0)),
                   dict(aug=dict(scale=float(np.nextafter(np.float32(1), np.float32(0))), rotate_tan=1.0, mirror_p=1.0, jitter=1e30)),
                   dict(n_frames=_A["key"] + 16), dict(key=_A["input_kp"] + 3 * 7 * 12 * 8)):
            assert _call(**kw) == HIP, (kw, _lib.last_error())


# ---- Augment ----------------------------------------------------------------------------------------------------------
def test_augment_validates_and_converts():
    a = hps.Augment()
    assert (a.scale, a.rotate_deg, a.mirror, a.jitter, a.rotate_tan) == (0.0, 0.0, 0.0, 0.0, 0.0)
    a = hps.Augment(scale=0.2, rotate_deg=15, mirror=0.5, jitter=3)
    assert a.scale == float(np.float32(0.2)) and a.mirror == 0.5 and a.jitter == 3.0 and a.rotate_deg == 15.0
    for deg in (0.0, 1.0, 15, 30.0, 89.5, 90):
        want = np.float32(math.tan(math.radians(deg) / 2.0))          # in double, rounded once
        got = hps.Augment(rotate_deg=deg).rotate_tan
        assert isinstance(got, float) and np.float32(got) == want and got == float(want), deg
    assert hps.Augment(rotate_deg=90).rotate_tan == 1.0 and hps.Augment(rotate_deg=30).rotate_tan == float(np.float32(0.2679491924311227))
    for bad in (dict(scale=-0.1), dict(scale=1.0), dict(scale=1.5), dict(scale=float("nan")), dict(scale=1 - 1e-9),
                dict(rotate_deg=-1), dict(rotate_deg=90.001), dict(rotate_deg=float("inf")),
                dict(mirror=-0.1), dict(mirror=1.1), dict(mirror=float("nan")),
                dict(jitter=-1), dict(jitter=float("inf")), dict(jitter=float("nan")), dict(jitter=1e39),
                dict(scale="0.1"), dict(mirror=None), dict(jitter=True)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            hps.Augment(**bad)
    with pytest.raises(AttributeError, match="frozen"):
        a.scale = 0.5
    with pytest.raises(AttributeError, match="frozen"):
        del a.jitter
    assert a == hps.Augment(0.2, 15, 0.5, 3) and hash(a) == hash(hps.Augment(0.2, 15, 0.5, 3)) and a != hps.Augment(0.2, 15, 0.5, 4)
    assert eval(repr(a), {"Augment": hps.Augment}) == a
    p = augment_ref.params(a)
    assert all(isinstance(v, np.float32) for v in p) and p.rotate_tan == np.float32(a.rotate_tan)


# ---- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h5_store", "json_store"])
def test_restatement_at_zero_parameters_is_the_plain_batch_bit_for_bit(name):
    rec = batch_ref.load_fixture(name)
    rows, offsets, n_body, tokens = rec["store"]
    zero = augment_ref.params(hps.Augment())
    assert rec["expected"]
    for (predict, dif, norm, sel, ln), want in rec["expected"].items():
        args = (rows, offsets, n_body, tokens, rec["lists"][ln], rec["starts"][(sel, ln)], rec["T"], predict, bool(dif),
                bool(norm), 1280, rec["frame0"])
        plain = batch_ref.batch(*args)
        got = augment_ref.batch(*args, par=zero, seed=5, epoch=3, entry0=11)
        assert set(got) == set(plain) == set(want)
        for k in want:
            assert batch_ref.same_bits(got[k], plain[k]) and batch_ref.same_bits(got[k], want[k]), (predict, dif, norm, sel, ln, k)


def _random_rows(n, n_body, seed):
    gen = np.random.default_rng(seed)
    J = n_body + 42
    a = gen.random((n, 3, J), dtype=np.float32) * np.array([1280.0, 720.0, 1.0], np.float32).reshape(1, 3, 1)
    return np.ascontiguousarray(a.reshape(n, 3 * J))


@pytest.mark.parametrize("n_body", [8, 12])
def test_rotation_and_scale_keep_every_pairwise_distance_times_s(n_body):
    """|distance' - s * distance| <= 2e-3 px in float64: about eight float32 roundings at magnitude <= 2048 (ulp 1.2e-4
    each way) plus |c^2 + sn^2 - 1| <= 2e-7 on distances <= 1840 px.  Derived, not tuned."""
    par = augment_ref.params(hps.Augment(scale=0.25, rotate_deg=30))
    J = n_body + 42
    rows = _random_rows(40, n_body, 100 + n_body)
    seen_s, seen_t, worst, worst_unit = [], [], 0.0, 0.0
    for p in range(12):
        s, c, sn, mirror = augment_ref.draws(par, p, epoch=p % 3, seed=21)
        assert not mirror and 0.75 <= float(s) <= 1.25 and abs(float(sn)) <= 0.5 + 1e-6 and float(c) >= math.cos(math.radians(30)) - 1e-6
        worst_unit = max(worst_unit, abs(float(c) ** 2 + float(sn) ** 2 - 1.0))
        v = augment_ref.virtual_rows(rows, n_body, par, p, p % 3, 21).reshape(-1, 3, J).astype(np.float64)
        o = rows.reshape(-1, 3, J).astype(np.float64)
        assert np.array_equal(v[:, 2], o[:, 2])                                            # confidences untouched
        dv = np.hypot(v[:, 0, :, None] - v[:, 0, None, :], v[:, 1, :, None] - v[:, 1, None, :])
        do = np.hypot(o[:, 0, :, None] - o[:, 0, None, :], o[:, 1, :, None] - o[:, 1, None, :])
        worst = max(worst, float(np.abs(dv - float(s) * do).max()))
        seen_s.append(float(s))
        seen_t.append(float(sn))
    print(f"worst |d' - s d| = {worst:.3e} px, worst |c^2 + sn^2 - 1| = {worst_unit:.3e}")
    assert worst <= 2e-3 and worst_unit <= 2e-7
    assert min(seen_s) < 1 < max(seen_s) and min(seen_t) < 0 < max(seen_t)                 # both directions were drawn


@pytest.mark.parametrize("n_body", [8, 12])
def test_mirror_alone(n_body):
    par = augment_ref.params(hps.Augment(mirror=1.0))
    J, M = n_body + 42, augment_ref.mirror_map(n_body)
    assert sorted(M) == list(range(J)) and [M[M[q]] for q in range(J)] == list(range(J)) and M[1] == 1     # an involution
    assert M[:n_body] == [0, 1, 5, 6, 7, 2, 3, 4, 9, 8, 11, 10][:n_body]
    assert all(M[n_body + k] == n_body + 21 + k for k in range(21))
    rows = _random_rows(40, n_body, 200 + n_body)
    assert all(augment_ref.mirrors(par, 3, 1, range(8)))                                  # p = 1: every sequence
    v = augment_ref.virtual_rows(rows, n_body, par, 5, 1, 3).reshape(-1, 3, J)
    o = rows.reshape(-1, 3, J)
    assert np.array_equal(v[:, :, 1].view(np.int32), o[:, :, 1].view(np.int32))           # the chest, bit for bit
    assert np.array_equal(v[:, 2].view(np.int32), o[:, 2][:, M].view(np.int32))           # confidences permuted exactly
    assert np.array_equal(v[:, 1].view(np.int32), o[:, 1][:, M].view(np.int32))           # y' == y_M exactly
    cx = o[:, 0, 1:2].astype(np.float64)
    assert float(np.abs(v[:, 0].astype(np.float64) + o[:, 0][:, M].astype(np.float64) - 2 * cx).max()) <= 1e-3
    assert not np.array_equal(v[:, 0], o[:, 0])
    # no mirror is drawn at probability 0, whatever the word
    assert not any(augment_ref.mirrors(augment_ref.params(hps.Augment(scale=0.1)), 3, 1, range(64)))


def test_draws_depend_on_index_epoch_and_seed_only():
    par = augment_ref.params(hps.Augment(scale=0.2, rotate_deg=15, mirror=0.5, jitter=3))
    base = augment_ref.draws(par, 4, 1, 9)
    assert augment_ref.draws(par, 4, 1, 9) == base
    for other in ((5, 1, 9), (4, 2, 9), (4, 1, 10), (4, 1 + (1 << 32), 9), (4, 1, 9 + (1 << 32))):
        assert augment_ref.draws(par, *other)[:3] != base[:3], other
    j = augment_ref.jitter(par, 4, 1, 9, 8, 29)
    assert j.shape == (8, 29, 2) and j.dtype == np.float32 and float(np.abs(j).max()) <= 3.0 and float(np.abs(j).max()) > 2.5
    assert len(np.unique(j)) == j.size                                                     # no two joints share a word
    assert np.array_equal(j, augment_ref.jitter(par, 4, 1 + (1 << 32), 9, 8, 29))          # the epoch's low word only
    assert not np.array_equal(j, augment_ref.jitter(par, 4, 2, 9, 8, 29))


# ---- the kernel -------------------------------------------------------------------------------------------------------
def test_kernel_has_no_scratch_spills_or_lds():
    kernels, _ = kernel_remarks()
    new = {n: res for n, res in kernels.items() if "b2h_build_batch_aug_k" in n}
    assert len(new) == 1, sorted(new)
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)
