"""The augmented batch build on the MI355X: b2h_build_batch_aug (kernel_build_batch_aug.h) against the numpy restatement
tests/augment_ref.py, bit for bit, for every predict mode, pad and transform combination, two seeds and three epochs;
zero parameters against b2h_build_batch; a step word against entry0; the keying; poisoned guard bands at the weakest
alignment the header promises; a captured build replayed over step and epoch words; `DeviceLoader(augment=)`.
The reference has no augmentation: this is parity with the project's own definition (include/b2h.h)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import augment_ref
import batch_ref
import hand_pose_sl_amd as hps
import plan_ref
import poison
from hand_pose_sl_amd import _lib

pytestmark = pytest.mark.gpu
DIF, NORM, FRAME0 = _lib.BATCH_DIF_ENCODING, _lib.BATCH_NORMALIZE, _lib.BATCH_PAD_FRAME0
FLOATS = ("input_kp", "target_kp", "target_conf")
LENGTHS = [0, 1, 5, 8, 13, 30]
T, B, S = 8, 6, 4
UTT = [5, 0, 3, 1, 4, 2]                   # every length once
START = [25, 0, 7, 0, -3, 2]               # 25 > 30 - 8 and -3 < 0 are clamped; the others belong to utterances that fit
ENTRY0 = 12
EPOCHS = (0, 1, (1 << 32) + 1)
AUGMENT = hps.Augment(scale=0.2, rotate_deg=15, mirror=0.5, jitter=3)
PAR = augment_ref.params(AUGMENT)
ZERO = augment_ref.params(hps.Augment())
MODES = [(8, "right_hand"), (12, "right_hand"), (12, "right_index"), (12, "right_3fingers")]


def _pick_seeds(count=2):
    """The first seeds under which both mirror outcomes occur among the six sequences, in every epoch: on the CPU."""
    out = []
    for seed in range(1, 1000):
        if all(len(set(augment_ref.mirrors(PAR, seed, e, range(ENTRY0, ENTRY0 + B)))) == 2 for e in EPOCHS):
            out.append(seed)
            if len(out) == count:
                return out
    raise AssertionError("no seed found")


SEEDS = _pick_seeds()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _signed(v):
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def _key(seed, epoch, dev=None):
    return torch.tensor([_signed(seed), _signed(epoch)], dtype=torch.int64, device=dev)


def _struct(par):
    return _lib.AugmentStruct(float(par.scale), float(par.rotate_tan), float(par.mirror_p), float(par.jitter))


def _flags(dif, norm, frame0):
    return (DIF if dif else 0) | (NORM if norm else 0) | (FRAME0 if frame0 else 0)


@functools.lru_cache(maxsize=None)
def _store(n_body, seed=7):
    gen = torch.Generator().manual_seed(seed + n_body)
    J = n_body + 42
    rows = torch.rand((sum(LENGTHS), 3, J), generator=gen) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)
    offsets = torch.tensor([0] + np.cumsum(LENGTHS).tolist(), dtype=torch.int64)
    tokens = torch.randint(0, 1000, (len(LENGTHS), S), generator=gen)
    return rows.reshape(-1, 3 * J).contiguous(), offsets, n_body, tokens


@functools.lru_cache(maxsize=None)
def _device_store(n_body, dev):
    return tuple(t.to(dev) if isinstance(t, torch.Tensor) else t for t in _store(n_body))


def _empty(dev, n_body, predict, n=B):
    ji, jt = batch_ref.joints(predict, n_body)
    return {"input_kp": torch.empty((n, T, ji, 2), device=dev), "target_kp": torch.empty((n, T, jt, 2), device=dev),
            "target_conf": torch.empty((n, T, jt), device=dev), "text_tokens": torch.empty((n, S), dtype=torch.int64, device=dev),
            "n_frames": torch.empty((n,), dtype=torch.int64, device=dev)}


def _native(dev, n_body, utt, start, predict, flags, par, key, entry0=0, step=None, n_plan=0, n=B, factor=1280.0):
    """One b2h_build_batch_aug call on the device store; `key` a device tensor {seed, epoch}.  Returns the batch dict."""
    rows, offsets, _, tokens = _device_store(n_body, dev)
    out = _empty(dev, n_body, predict, n)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().b2h_build_batch_aug(
        _p(rows), rows.shape[0], _p(offsets), len(LENGTHS), n_body, _p(tokens), S, _p(utt), _p(start), n_plan, _p(step), entry0,
        ctypes.byref(_struct(par)), _p(key), n, T, _lib.PREDICT[predict], flags, factor, _p(out["input_kp"]), _p(out["target_kp"]),
        _p(out["target_conf"]), _p(out["text_tokens"]), _p(out["n_frames"]), st))
    return out


def _plain(dev, n_body, utt, start, predict, flags, n=B):
    rows, offsets, _, tokens = _device_store(n_body, dev)
    out = _empty(dev, n_body, predict, n)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().b2h_build_batch(
        _p(rows), rows.shape[0], _p(offsets), len(LENGTHS), n_body, _p(tokens), S, _p(utt), _p(start), n, T,
        _lib.PREDICT[predict], flags, 1280.0, _p(out["input_kp"]), _p(out["target_kp"]), _p(out["target_conf"]),
        _p(out["text_tokens"]), _p(out["n_frames"]), st))
    return out


def _assert_same(got, want, what):
    assert set(got) >= set(want), what
    for k, w in want.items():
        assert batch_ref.same_bits(got[k].cpu(), w.cpu()), (what, k)


def _assert_unknown(got, b, what):
    for k in FLOATS:
        assert bool((got[k][b].cpu().view(torch.int32) == 0x7FC00000).all()), (what, k)
    assert got["text_tokens"][b].tolist() == [-1] * S and int(got["n_frames"][b]) == 0, what


# ---- 1. the restatement ------------------------------------------------------------------------------------------------
def test_the_seeds_draw_both_mirror_outcomes():
    assert len(SEEDS) == 2 and SEEDS[0] != SEEDS[1]
    for seed in SEEDS:
        for epoch in EPOCHS:
            assert sorted(set(augment_ref.mirrors(PAR, seed, epoch, range(ENTRY0, ENTRY0 + B)))) == [False, True], (seed, epoch)


@pytest.mark.parametrize("n_body,predict", MODES)
def test_kernel_equals_the_restatement(cuda_device, n_body, predict):
    """29 input joints (right_index) make the joint pairs of a jitter block straddle a 256-lane block boundary."""
    store = _store(n_body)
    utt, start = torch.tensor(UTT, device=cuda_device), torch.tensor(START, device=cuda_device)
    cases = 0
    for frame0 in (False, True):
        for dif in (False, True):
            for norm in (False, True):
                for seed in SEEDS:
                    for epoch in EPOCHS:
                        got = _native(cuda_device, n_body, utt, start, predict, _flags(dif, norm, frame0), PAR,
                                      _key(seed, epoch, cuda_device), ENTRY0)
                        want = augment_ref.batch(*store, UTT, START, T, predict, dif, norm, 1280, frame0, PAR, seed, epoch, ENTRY0)
                        _assert_same(got, want, (frame0, dif, norm, seed, epoch))
                        cases += 1
    assert cases == 2 * 4 * 2 * 3
    assert got["n_frames"].tolist() == [min(LENGTHS[u], T) for u in UTT]


@pytest.mark.parametrize("par", [augment_ref.Params(np.float32(0.2), 0, 0, 0), augment_ref.Params(0, np.float32(0.1), 0, 0),
                                 augment_ref.Params(0, 0, np.float32(1), 0), augment_ref.Params(0, 0, 0, np.float32(3)),
                                 augment_ref.Params(np.float32(0.999), np.float32(1), np.float32(0.25), np.float32(100))],
                         ids=["scale", "rotate", "mirror", "jitter", "extremes"])
def test_each_stage_alone_equals_the_restatement(cuda_device, par):
    utt, start = torch.tensor(UTT, device=cuda_device), torch.tensor(START, device=cuda_device)
    for n_body, predict, frame0 in ((8, "right_hand", False), (12, "right_index", True), (12, "right_3fingers", True)):
        got = _native(cuda_device, n_body, utt, start, predict, _flags(True, True, frame0), par, _key(SEEDS[0], 2, cuda_device), 3)
        want = augment_ref.batch(*_store(n_body), UTT, START, T, predict, True, True, 1280, frame0, par, SEEDS[0], 2, 3)
        _assert_same(got, want, (n_body, predict))


# ---- 2. zero parameters are the plain build ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_body,predict", MODES)
def test_zero_parameters_give_the_bits_of_the_plain_build(cuda_device, n_body, predict):
    utt = torch.tensor(UTT + [77, -1], device=cuda_device)             # and two ids the store does not have
    start = torch.tensor(START + [0, 0], device=cuda_device)
    for frame0 in (False, True):
        for dif in (False, True):
            for norm in (False, True):
                flags = _flags(dif, norm, frame0)
                want = _plain(cuda_device, n_body, utt, start, predict, flags, n=8)
                got = _native(cuda_device, n_body, utt, start, predict, flags, ZERO, _key(9, 4, cuda_device), 100, n=8)
                _assert_same(got, want, (frame0, dif, norm))
                _assert_unknown(got, 6, "foreign id")
                _assert_same(_native(cuda_device, n_body, utt, None, predict, flags, ZERO, _key(9, 4, cuda_device), n=8),
                             _plain(cuda_device, n_body, utt, None, predict, flags, n=8), "NULL start")


# ---- 3. a step word against entry0 -------------------------------------------------------------------------------------
PLAN_UTT = [5, 3, 4, 1, 2, 5, 0, 4, 4, 5, 1, 3, 2, 5]                    # 14 entries at B = 6: two full steps and a ragged one
PLAN_START = [3, 0, 1, 0, 5, 14, 0, 9, 2, 30, 0, 0, 0, 22]


@pytest.mark.parametrize("n_body,predict,frame0", [(8, "right_hand", False), (12, "right_index", True)])
def test_planned_build_equals_the_eager_build_at_entry0(cuda_device, n_body, predict, frame0):
    ds = hps.DeviceDataset(*_store(n_body)[:3], _store(n_body)[3])
    loader = hps.DeviceLoader(ds, B, T, predict=predict, pad="frame0" if frame0 else "zeros", plan_source="native",
                              seed=SEEDS[0], augment=AUGMENT)
    plan = (torch.tensor(PLAN_UTT, device=cuda_device), torch.tensor(PLAN_START, device=cuda_device))
    loader.plan_epoch(epoch=5)                                          # the epoch word; the plan itself is the test's
    word = torch.zeros(1, dtype=torch.int64, device=cuda_device)
    out = loader.empty_batch(B)
    for k in range(2):
        word.fill_(k)
        assert loader.build_planned(plan, word, out) is out
        eager = loader.build(plan[0][k * B:(k + 1) * B], plan[1][k * B:(k + 1) * B], entry0=k * B)
        _assert_same(out, eager, k)
        want = augment_ref.batch(*_store(n_body), PLAN_UTT[k * B:(k + 1) * B], PLAN_START[k * B:(k + 1) * B], T, predict, True, True,
                                 1280, frame0, PAR, SEEDS[0], 5, k * B)
        _assert_same(out, want, ("restatement", k))
        other = loader.build(plan[0][k * B:(k + 1) * B], plan[1][k * B:(k + 1) * B], entry0=k * B + 1)
        assert not torch.equal(other["input_kp"], eager["input_kp"])    # entry0 is what keys the draws
    word.fill_(2)                                                       # the last, partial step: two entries, then unknown
    loader.build_planned(plan, word, out)
    eager = loader.build(plan[0][12:], plan[1][12:], entry0=12)
    for k in eager:
        assert batch_ref.same_bits(out[k][:2].cpu(), eager[k].cpu()), k
    for b in range(2, B):
        _assert_unknown(out, b, "the plan's tail")
    for past in (3, -1, 1 << 40):                                       # a step past the plan: NaN / -1 / 0
        word.fill_(past)
        loader.build_planned(plan, word, out)
        for b in range(B):
            _assert_unknown(out, b, past)


# ---- 4. the keying -----------------------------------------------------------------------------------------------------
def test_keying(cuda_device):
    utt, start = torch.tensor(UTT, device=cuda_device), torch.tensor(START, device=cuda_device)
    flags = _flags(True, True, True)

    def run(par=PAR, seed=SEEDS[0], epoch=1, entry0=0):
        return _native(cuda_device, 12, utt, start, "right_index", flags, par, _key(seed, epoch, cuda_device), entry0)
    base = run()
    _assert_same(run(), base, "the same key")
    for what, other in (("epoch", run(epoch=2)), ("epoch, high word", run(epoch=1 + (1 << 32))), ("seed", run(seed=SEEDS[1])),
                        ("seed, high word", run(seed=SEEDS[0] + (1 << 32)))):
        assert not torch.equal(other["input_kp"], base["input_kp"]), what
        for k in ("text_tokens", "n_frames"):
            assert torch.equal(other[k], base[k]), (what, k)
    only = augment_ref.Params(0, 0, 0, np.float32(3))                   # jitter alone touches input_kp alone
    with_jitter, without = run(only), run(ZERO)
    for k in ("target_kp", "target_conf", "text_tokens", "n_frames"):
        assert batch_ref.same_bits(with_jitter[k].cpu(), without[k].cpu()), k
    assert not torch.equal(with_jitter["input_kp"], without["input_kp"])
    noise = (with_jitter["input_kp"] - without["input_kp"]).abs() * 1280
    assert 2.5 < float(noise.max()) <= 3.0 + 1e-3
    # frames of zero padding stay zeros (pad "zeros"): the utterance of one frame has seven of them
    padded = _native(cuda_device, 12, utt, start, "right_index", _flags(True, True, False), PAR, _key(SEEDS[0], 1, cuda_device))
    assert not bool(padded["input_kp"][3, 1:].any()) and bool(padded["input_kp"][3, 0].any())


def test_host_key_is_refused(cuda_device):
    utt = torch.tensor(UTT, device=cuda_device)
    with pytest.raises(ValueError, match="key is not"):
        _native(cuda_device, 8, utt, None, "right_hand", 3, PAR, _key(1, 0))


# ---- 5. poisoned buffers, at the weakest alignment the header promises --------------------------------------------------
@pytest.mark.parametrize("n_body,predict,frame0,planned,shift", [(8, "right_hand", False, False, 0), (12, "right_index", True, True, 8),
                                                                 (12, "right_3fingers", False, True, 8)])
def test_poisoned_buffers(cuda_device, n_body, predict, frame0, planned, shift):
    """Every output word written, nothing else written; with shift 8 every pointer sits 8 bytes past the 16-byte grid,
    the alignment include/b2h.h promises for all of them.  The planned case runs the plan's ragged last step."""
    rows, offsets, _, tokens = _store(n_body)
    ji, jt = batch_ref.joints(predict, n_body)
    flags, seed, epoch = _flags(True, True, frame0), SEEDS[1], (1 << 32) + 1
    lib, aug = _lib.load(), _struct(PAR)
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream)
    ins = {"rows": rows, "offsets": offsets, "tokens": tokens, "key": _key(seed, epoch)}
    if planned:
        ins.update(utt=torch.tensor(PLAN_UTT), start=torch.tensor(PLAN_START), step=torch.tensor([2]))
    else:
        ins.update(utt=torch.tensor(UTT), start=torch.tensor(START))
    outs = {"input_kp": (B, T, ji, 2), "target_kp": (B, T, jt, 2), "target_conf": (B, T, jt), "text_tokens": (B, S, 2),
            "n_frames": (B, 2)}                                          # an int64 output counts as two words
    out = poison.launch(
        lambda p: lib.b2h_build_batch_aug(p["rows"], rows.shape[0], p["offsets"], len(LENGTHS), n_body, p["tokens"], S, p["utt"],
                                          p["start"], len(PLAN_UTT), p.get("step"), ENTRY0, ctypes.byref(aug), p["key"], B, T,
                                          _lib.PREDICT[predict], flags, 1280.0, p["input_kp"], p["target_kp"], p["target_conf"],
                                          p["text_tokens"], p["n_frames"], st),
        ins, outs, cuda_device, shifts={k: shift for k in list(ins) + list(outs)})
    got = {k: out[k] for k in FLOATS}
    got["text_tokens"] = out["text_tokens"].view(torch.int64).view(B, S)
    got["n_frames"] = out["n_frames"].view(torch.int64).view(B)
    if planned:
        want = augment_ref.batch(rows, offsets, n_body, tokens, PLAN_UTT[12:], PLAN_START[12:], T, predict, True, True, 1280, frame0,
                                 PAR, seed, epoch, 12)
        for k, w in want.items():
            assert batch_ref.same_bits(got[k][:2].cpu(), w), k
        for b in range(2, B):
            _assert_unknown(got, b, "the plan's tail")
    else:
        _assert_same(got, augment_ref.batch(rows, offsets, n_body, tokens, UTT, START, T, predict, True, True, 1280, frame0, PAR,
                                            seed, epoch, ENTRY0), "poisoned")


# ---- 6. a captured build ------------------------------------------------------------------------------------------------
def test_captured_planned_build_follows_the_step_and_epoch_words(cuda_device):
    ds = hps.DeviceDataset(*_store(12)[:3], _store(12)[3])
    loader = hps.DeviceLoader(ds, B, T, predict="right_index", pad="frame0", plan_source="native", seed=SEEDS[1], augment=AUGMENT)
    plan = (torch.tensor(PLAN_UTT, device=cuda_device), torch.tensor(PLAN_START, device=cuda_device))
    word = torch.zeros(1, dtype=torch.int64, device=cuda_device)
    out = loader.empty_batch(B)
    loader.plan_epoch(epoch=0)
    s = torch.cuda.Stream(cuda_device)                                  # warm-up on a side stream, as torch's docs do
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        loader.build_planned(plan, word, out)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                       # one stream: no parallel branches
        assert loader.build_planned(plan, word, out) is out
    for epoch in (3, (1 << 32) + 1):
        loader.plan_epoch(epoch=epoch)                                  # rewrites the epoch word in place: no new capture
        for k in (1, 0, 2):
            word.fill_(k)
            graph.replay()
            n = min(B, len(PLAN_UTT) - k * B)
            eager = loader.build(plan[0][k * B:k * B + n], plan[1][k * B:k * B + n], entry0=k * B)
            want = augment_ref.batch(*_store(12), PLAN_UTT[k * B:k * B + n], PLAN_START[k * B:k * B + n], T, "right_index", True, True,
                                     1280, True, PAR, SEEDS[1], epoch, k * B)
            for name in want:
                assert batch_ref.same_bits(out[name][:n].cpu(), eager[name].cpu()), (epoch, k, name)
                assert batch_ref.same_bits(out[name][:n].cpu(), want[name]), (epoch, k, name, "restatement")
            for b in range(n, B):
                _assert_unknown(out, b, (epoch, k))


# ---- 7. DeviceLoader(augment=) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan_source", ["native", "torch"])
def test_loader_iterates_augmented_epochs_keyed_by_their_number(cuda_device, plan_source):
    rows, offsets, n_body, tokens = _store(8)
    ds = hps.DeviceDataset(rows, offsets, n_body, tokens)
    loader = hps.DeviceLoader(ds, 4, T, selection="randomcrop", shuffle=plan_source == "native", plan_source=plan_source, seed=SEEDS[0],
                              augment=AUGMENT)
    first = None
    for epoch in (0, 1):
        torch.manual_seed(3)                                            # the torch source draws its crops from torch
        batches = list(loader)
        assert len(batches) == 2 and loader.epochs_planned == epoch + 1
        if plan_source == "native":
            utt, start = plan_ref.plan(offsets.tolist(), 6, T, True, True, SEEDS[0], epoch)
        else:
            torch.manual_seed(3)
            utt, start = (t.tolist() for t in hps.DeviceLoader(ds, 4, T, selection="randomcrop").plan_epoch())
        for i, got in enumerate(batches):
            want = augment_ref.batch(rows, offsets, n_body, tokens, utt[4 * i:4 * i + 4], start[4 * i:4 * i + 4], T, "right_hand", True,
                                     True, 1280, False, PAR, SEEDS[0], epoch, 4 * i)
            _assert_same(got, want, (plan_source, epoch, i))
            assert got["body_kp"] is got["input_kp"]
        if first is None:
            first = batches
        elif plan_source == "torch":                                    # the same utterances and crops, another epoch word
            assert not torch.equal(first[0]["input_kp"], batches[0]["input_kp"])
    plain = hps.DeviceLoader(ds, 4, T, selection="first")
    assert plain.augment is None and plain._aug_key is None
    with pytest.raises(TypeError, match="Augment"):
        hps.DeviceLoader(ds, 4, T, augment=(0.1, 0, 0, 0))


def test_predict_dataset_refuses_an_augmenting_loader(cuda_device):
    rows, offsets, n_body, tokens = _store(12)
    ds = hps.DeviceDataset(rows, offsets, n_body, tokens)
    torch.manual_seed(32)
    conv = hps.ConvModel(30, "ReLU", False).to(cuda_device)
    with pytest.raises(ValueError, match="augment=None"):
        hps.predict_dataset(conv, hps.DeviceLoader(ds, 4, T, pad="frame0", augment=AUGMENT))
