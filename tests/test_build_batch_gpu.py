"""The device-resident training set on the MI355X: b2h_build_batch (kernel_build_batch.h) against the fixtures made
from the reference's own datasets and transforms and against the torch restatement tests/batch_ref.py on seeded random
stores -- exact equality, because every output element is a copy or one IEEE subtraction and one correctly rounded
division --; between poisoned guard bands; with ids the store does not have; `DeviceLoader` through `validate()`;
`train_epoch` against a hand-written loop; one captured step from the batch build to the Adam update."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import batch_ref
import hand_pose_sl_amd as hps
import poison
from hand_pose_sl_amd import _lib

pytestmark = pytest.mark.gpu
DIF, NORM, FRAME0 = _lib.BATCH_DIF_ENCODING, _lib.BATCH_NORMALIZE, _lib.BATCH_PAD_FRAME0
FLOATS = ("input_kp", "target_kp", "target_conf")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _flags(dif, norm, frame0):
    return (DIF if dif else 0) | (NORM if norm else 0) | (FRAME0 if frame0 else 0)


def _native(dev, store, utt, start, T, predict="right_hand", flags=DIF | NORM, factor=1280.0):
    """One b2h_build_batch call on a store of device tensors; returns the batch dict."""
    rows, offsets, n_body, tokens = store
    ji, jt = batch_ref.joints(predict, n_body)
    B = utt.shape[0]
    out = {"input_kp": torch.empty((B, T, ji, 2), device=dev), "target_kp": torch.empty((B, T, jt, 2), device=dev),
           "target_conf": torch.empty((B, T, jt), device=dev), "n_frames": torch.empty((B,), dtype=torch.int64, device=dev)}
    if tokens is not None:
        out["text_tokens"] = torch.empty((B, tokens.shape[1]), dtype=torch.int64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().b2h_build_batch(
        _p(rows), rows.shape[0], _p(offsets), offsets.numel() - 1, n_body, _p(tokens), 0 if tokens is None else tokens.shape[1],
        _p(utt), _p(start), B, T, _lib.PREDICT[predict], flags, factor, _p(out["input_kp"]), _p(out["target_kp"]),
        _p(out["target_conf"]), _p(out.get("text_tokens")), _p(out["n_frames"]), st))
    return out


def _to(dev, store):
    return tuple(t.to(dev) if isinstance(t, torch.Tensor) else t for t in store)


def _assert_same(got, want, what):
    assert set(got) >= set(want), what
    for k, w in want.items():
        g = got[k].cpu()
        assert torch.equal(g, w), (what, k, g.shape, w.shape)
        assert batch_ref.same_bits(g, w), (what, k, "sign of a zero")


# ---- 1. the reference's batches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h5_store", "json_store"])
def test_kernel_equals_every_fixture(cuda_device, name):
    rec = batch_ref.load_fixture(name)
    store = _to(cuda_device, rec["store"])
    assert len(rec["expected"]) >= 12
    for (predict, dif, norm, sel, ln), want in rec["expected"].items():
        utt, start = rec["lists"][ln].to(cuda_device), rec["starts"][(sel, ln)].to(cuda_device)
        got = _native(cuda_device, store, utt, start, rec["T"], predict, _flags(dif, norm, rec["frame0"]))
        _assert_same(got, want, (predict, dif, norm, sel, ln))
        if sel == "first":                                   # start = NULL is start = 0
            _assert_same(_native(cuda_device, store, utt, None, rec["T"], predict, _flags(dif, norm, rec["frame0"])), want, "NULL start")


# ---- 2. seeded random stores against the restatement -------------------------------------------------------------------
def _random_store(n_body, T, S, seed):
    gen = torch.Generator().manual_seed(seed)
    lengths = [0, 1, T - 1, T, T + 1, 3 * T]
    J = n_body + 42
    rows = torch.rand((sum(lengths), 3, J), generator=gen) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)
    offsets = torch.tensor([0] + np.cumsum(lengths).tolist(), dtype=torch.int64)
    tokens = None if S is None else torch.randint(0, 1000, (len(lengths), S), generator=gen)
    return (rows.reshape(-1, 3 * J).contiguous(), offsets, n_body, tokens), lengths


def _batches(T):
    """(utt, start): every length, starts at 0, at len - T, in the middle and out of range on both sides, B in {1, 3, 5}."""
    long, over = 5, 4                                                   # the utterances of 3 T and T + 1 frames
    out = [([u], [s]) for u in range(6) for s in (0, 1)]                # B = 1: every length
    out += [([long], [s]) for s in (2 * T, T, -1, 2 * T + 1, 1 << 40, -(1 << 40))]
    out += [([over, long, 3], [1, -7, 5]), ([long, 0, over], [T, 7, 0]), ([2, 1, 0], [0, 3, -2])]           # B = 3
    out += [([long] * 5, [0, 2 * T, T // 2 + 1, -3, 10 * T]), ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0]), ([5, 4, 3, 3, 5], [T + 1, 2, 0, 0, 2 * T - 1])]
    return out


@pytest.mark.parametrize("T", [1, 7, 64, 65])
def test_kernel_equals_the_restatement_on_random_stores(cuda_device, T):
    case = 0
    for n_body in (8, 12):
        for S in (1, 40, None):
            store, lengths = _random_store(n_body, T, S, 1000 * T + 10 * n_body + (S or 0))
            dstore = _to(cuda_device, store)
            for predict in (batch_ref.PREDICTS if n_body == 12 else batch_ref.PREDICTS[:1]):
                for frame0 in (False, True):
                    for utt, start in _batches(T):
                        case += 1
                        dif, norm = bool(case & 1), bool(case & 2)
                        want = batch_ref.batch(*store, utt, start, T, predict, dif, norm, 1280, frame0)
                        got = _native(cuda_device, dstore, torch.tensor(utt, device=cuda_device),
                                      torch.tensor(start, device=cuda_device), T, predict, _flags(dif, norm, frame0))
                        _assert_same(got, want, (n_body, S, predict, frame0, utt, start))
                        assert got["n_frames"].tolist() == [min(lengths[u], T) for u in utt]
    assert case == (1 + 3) * 2 * 3 * len(_batches(T))          # predict modes of both stores x pads x token shapes


def test_other_factor_and_no_conf(cuda_device):
    store, _ = _random_store(12, 7, 3, 5)
    dstore = _to(cuda_device, store)
    utt, start = [5, 2, 0], [9, 0, 0]
    want = batch_ref.batch(*store, utt, start, 7, "right_index", True, True, 3.0, True)
    got = _native(cuda_device, dstore, torch.tensor(utt, device=cuda_device), torch.tensor(start, device=cuda_device), 7,
                  "right_index", _flags(True, True, True), 3.0)
    _assert_same(got, want, "factor 3")                      # x / 3 is not x * (1 / 3)
    rows, offsets, n_body, tokens = dstore
    out = {k: torch.full_like(v, 7) for k, v in got.items()}
    dutt = torch.tensor(utt, device=cuda_device)
    _lib.check(_lib.load().b2h_build_batch(_p(rows), rows.shape[0], _p(offsets), 6, 12, None, 0, _p(dutt),
                                           None, 3, 7, 1, 0, 1.0, _p(out["input_kp"]), _p(out["target_kp"]), None, None,
                                           _p(out["n_frames"]), None))
    torch.cuda.synchronize()
    assert bool((out["target_conf"] == 7).all()) and bool((out["text_tokens"] == 7).all())   # left out: untouched
    _assert_same({k: out[k] for k in ("input_kp", "target_kp", "n_frames")},
                 {k: v for k, v in batch_ref.batch(*store, utt, None, 7, "right_index", False, False, 1, False).items()
                  if k in ("input_kp", "target_kp", "n_frames")}, "no conf, no tokens")


def test_host_memory_is_refused(cuda_device):
    store, _ = _random_store(8, 7, 3, 6)
    dstore = _to(cuda_device, store)
    with pytest.raises(ValueError, match="utt is not"):
        _native(cuda_device, dstore, torch.tensor([1, 2]), None, 7)                         # utt on the host
    with pytest.raises(ValueError, match="rows is not"):
        _native(cuda_device, (store[0],) + dstore[1:], torch.tensor([1, 2], device=cuda_device), None, 7)


# ---- 3. poisoned buffers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_body,predict,frame0", [(8, "right_hand", False), (12, "right_index", True), (12, "right_3fingers", False)])
def test_poisoned_buffers(cuda_device, n_body, predict, frame0):
    """The store's buffer ends with its last utterance, whose last window (start = len - T, and a start beyond it) ends
    at the guard band; a short and an empty utterance exercise both paddings."""
    T, S = 7, 5
    store, lengths = _random_store(n_body, T, S, 77 + n_body)
    rows, offsets, _, tokens = store
    utt, start = [5, 5, 2, 0, 1], [2 * T, 99, 0, 0, 0]
    B = len(utt)
    ji, jt = batch_ref.joints(predict, n_body)
    flags = _flags(True, True, frame0)
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream)
    out = poison.launch(
        lambda p: lib.b2h_build_batch(p["rows"], rows.shape[0], p["offsets"], len(lengths), n_body, p["tokens"], S, p["utt"],
                                      p["start"], B, T, _lib.PREDICT[predict], flags, 1280.0, p["input_kp"], p["target_kp"],
                                      p["target_conf"], p["text_tokens"], p["n_frames"], st),
        {"rows": rows, "offsets": offsets, "tokens": tokens, "utt": torch.tensor(utt), "start": torch.tensor(start)},
        {"input_kp": (B, T, ji, 2), "target_kp": (B, T, jt, 2), "target_conf": (B, T, jt), "text_tokens": (B, S, 2),
         "n_frames": (B, 2)}, cuda_device)                       # an int64 output counts as two words
    got = {k: out[k] for k in FLOATS}
    got["text_tokens"] = out["text_tokens"].view(torch.int64).view(B, S)
    got["n_frames"] = out["n_frames"].view(torch.int64).view(B)
    _assert_same(got, batch_ref.batch(*store, utt, start, T, predict, True, True, 1280, frame0), "poisoned")


# ---- 4. ids the store does not have ------------------------------------------------------------------------------------
@pytest.mark.parametrize("foreign", [-1, 6, 1 << 40, -(1 << 62)])
def test_foreign_id_is_loud_and_private(cuda_device, foreign):
    T = 7
    store, _ = _random_store(12, T, 5, 9)
    dstore = _to(cuda_device, store)
    utt, start = [5, foreign, 2, 4], [3, 1, 0, 1]
    for frame0 in (False, True):
        got = _native(cuda_device, dstore, torch.tensor(utt, device=cuda_device), torch.tensor(start, device=cuda_device), T,
                      "right_3fingers", _flags(True, True, frame0))
        ref = _native(cuda_device, dstore, torch.tensor([5, 2, 4], device=cuda_device), torch.tensor([3, 0, 1], device=cuda_device),
                      T, "right_3fingers", _flags(True, True, frame0))
        for k in FLOATS:
            bits = got[k][1].cpu().view(torch.int32)
            assert bool((bits == 0x7FC00000).all()), k                                    # the quiet NaN, every float
        assert got["text_tokens"][1].tolist() == [-1] * 5 and int(got["n_frames"][1]) == 0
        keep = torch.tensor([0, 2, 3], device=cuda_device)
        for k in ref:
            assert batch_ref.same_bits(got[k][keep], ref[k]), k
    # the losses then say so
    pred = torch.zeros_like(got["target_kp"])
    assert bool(torch.isnan(hps.weighted_pose_l1(pred, got["target_kp"], got["n_frames"], got["target_conf"])))


# ---- 5. DeviceLoader, and validate() over it ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dataset(name):
    rec = batch_ref.load_fixture(name)
    rows, offsets, n_body, tokens = rec["store"]
    if name == "json_store":
        ds = hps.DeviceDataset.from_frames(rec["frames"], tokens)
    else:
        ds = hps.DeviceDataset.from_h5_rows([rows[int(a):int(b)].numpy() for a, b in zip(offsets[:-1], offsets[1:])], tokens)
    assert torch.equal(ds.rows.cpu(), rows) and torch.equal(ds.offsets.cpu(), offsets) and ds.n_body == n_body
    return rec, ds


def _loader(name, predict="right_hand", dif=True, norm=True, batch_size=4, **kw):
    rec, ds = _dataset(name)
    return hps.DeviceLoader(ds, batch_size, rec["T"], selection="first", predict=predict, dif_encoding=bool(dif),
                            normalize=bool(norm), pad="frame0" if rec["frame0"] else "zeros", **kw)


@functools.lru_cache(maxsize=None)
def _h5_without_the_empty_utterance():
    """(host store, dataset) of the HDF5 fixture's utterances of 1, 3, 7, 8 and 19 frames.  The empty one is left to the
    parity tests: its loss is 0 / 0 = NaN, in the reference as here, which no equality of floats survives."""
    rec = batch_ref.load_fixture("h5_store")
    rows, offsets, n_body, tokens = rec["store"]
    assert offsets[:2].tolist() == [0, 0]
    store = (rows, offsets[1:].clone(), n_body, tokens[1:].clone())
    return store, hps.DeviceDataset(store[0], store[1], n_body, store[3])


def _h5_host_batches(batch_size):
    store, ds = _h5_without_the_empty_utterance()
    out = []
    for i in range(0, len(ds), batch_size):
        b = batch_ref.batch(*store, list(range(i, min(i + batch_size, len(ds)))), None, 7)
        b["body_kp"] = b["input_kp"]
        out.append(b)
    return out


def _host_batches(rec, predict, dif, norm):
    out = []
    for ln in ("a", "b"):
        b = dict(rec["expected"][(predict, dif, norm, "first", ln)])
        if predict == "right_hand":
            b["body_kp"] = b["input_kp"]
        out.append(b)
    return out


@pytest.mark.parametrize("name", ["h5_store", "json_store"])
def test_loader_pass_equals_the_fixtures(cuda_device, name):
    rec, ds = _dataset(name)
    for predict, dif, norm in batch_ref.variants(rec["n_body"]):
        loader = _loader(name, predict, dif, norm)
        assert len(loader) == 2 and len(_loader(name, predict, dif, norm, drop_last=True)) == 1
        batches = list(loader)
        assert len(batches) == 2 and batches[1]["n_frames"].shape[0] == len(ds) - 4        # a smaller last batch
        for got, want in zip(batches, _host_batches(rec, predict, dif, norm)):
            assert all(v.device == ds.device for v in got.values())
            _assert_same(got, want, (predict, dif, norm))
            assert ("body_kp" in got) == (predict == "right_hand")
            assert predict != "right_hand" or got["body_kp"] is got["input_kp"]


def test_loader_random_crops_follow_the_seed_and_stay_in_range(cuda_device):
    rec, ds = _dataset("json_store")
    loader = hps.DeviceLoader(ds, 5, rec["T"], pad="frame0", shuffle=True, generator=torch.Generator().manual_seed(3))
    utt = torch.tensor([4] * 1024 + [3] * 64 + [0] * 8, device=cuda_device)       # 19, 8 and 1 frames at T = 7
    torch.manual_seed(11)
    a = loader.draw_starts(utt)
    torch.manual_seed(11)
    assert torch.equal(a, loader.draw_starts(utt))
    assert sorted(set(a[:1024].tolist())) == list(range(13)) and set(a[1024:1088].tolist()) == {0, 1} and not a[1088:].any()
    torch.manual_seed(12)
    (batch,) = list(loader)
    assert sorted(batch["n_frames"].tolist()) == [1, 3, 7, 7, 7] and not bool(torch.isnan(batch["input_kp"]).any())


@pytest.mark.parametrize("loss", ["L1", "confL1"])
def test_validate_over_the_loader_equals_validate_over_host_batches(cuda_device, loss):
    import types
    torch.manual_seed(21)
    _, h5 = _h5_without_the_empty_utterance()
    loader = hps.DeviceLoader(h5, 2, 7, selection="first")
    assert len(loader) == 3
    tpt = hps.TextPoseTransformer(1000, 8, 2, 4, 128, 42, 1, 1).to(cuda_device)
    want = hps.validate(tpt, _h5_host_batches(2), loss=loss)
    assert hps.validate(tpt, loader, loss=loss) == want and np.isfinite(want)
    args = types.SimpleNamespace(loss=loss, model="TextPoseTransformer")
    assert hps.validate(tpt, loader, None, None, args) == want
    rec, _ = _dataset("json_store")
    conv = hps.ConvModel(30, "ReLU", False).to(cuda_device)
    want = hps.validate(conv, _host_batches(rec, "right_hand", 1, 1), loss=loss)
    assert hps.validate(conv, _loader("json_store"), loss=loss) == want and np.isfinite(want)


# ---- 6. train_epoch ----------------------------------------------------------------------------------------------------
def _model(dev, seed=31):
    torch.manual_seed(seed)
    return hps.TextPoseTransformer(1000, 8, 2, 4, 128, 42, 1, 1, dropout=0.0).to(dev)


@pytest.mark.parametrize("loss", ["L1", "confL1"])
def test_train_epoch_equals_a_hand_written_loop_over_host_batches(cuda_device, loss):
    _, ds = _h5_without_the_empty_utterance()
    loader = hps.DeviceLoader(ds, 2, 7, selection="first")
    assert len(loader) == 3                                             # 2, 2 and 1 utterances
    m = _model(cuda_device)
    got = hps.train_epoch(m, loader, hps.maskedPoseL1() if loss == "L1" else hps.poderatedPoseL1(), hps.Adam(m.parameters(), lr=1e-3))
    twin = _model(cuda_device).train()
    opt = hps.Adam(twin.parameters(), lr=1e-3)
    values = []
    for b in _h5_host_batches(2):                                       # traintest.py:87-123 over host-built batches
        prediction = twin(b["text_tokens"].to(cuda_device), b["input_kp"].to(cuda_device))
        target = b["target_kp"].to(cuda_device)
        if loss == "L1":
            value = hps.masked_pose_l1(prediction, target, b["n_frames"])
        else:
            value = hps.weighted_pose_l1(prediction, target, b["n_frames"], b["target_conf"])
        opt.zero_grad()
        value.backward()
        opt.step()
        values.append(value.item())
    assert got == sum(values) / 3 and np.isfinite(got)
    moved = 0
    for (k, a), b, c in zip(m.named_parameters(), twin.parameters(), _model(cuda_device).parameters()):
        assert torch.equal(a, b), k
        moved += int(not torch.equal(a, c))
    assert moved > 0                                                    # the epoch did train
    with pytest.raises(ValueError, match="TextPoseTransformer"):
        import types
        hps.train_epoch(m, loader, None, opt, types.SimpleNamespace(loss="L1", model="Conv"))
    with pytest.raises(ValueError, match="L1 or confL1"):
        hps.train_epoch(m, loader, "MSE", opt)


# ---- 7. one captured step, from the batch build to the Adam update ------------------------------------------------------
def test_captured_step_with_the_batch_build_equals_eager(cuda_device):
    rec, ds = _dataset("h5_store")
    loader = _loader("h5_store", batch_size=2)
    steps = [([5, 3], [1, 1]), ([4, 1], [12, 0]), ([2, 5], [0, 5])]    # utterance 5 has 19 frames, 4 has 8: crops at T = 7

    def one_step(m, opt, utt, start, out=None):
        b = loader.build(utt, start, out=out)
        opt.zero_grad(set_to_none=True)
        hps.masked_pose_l1(m(b["text_tokens"], b["input_kp"]), b["target_kp"], b["n_frames"]).backward()
        opt.step()
        return b

    m = _model(cuda_device).train()
    opt = hps.Adam(m.parameters(), lr=1e-3)
    utt, start = (torch.tensor(v, device=cuda_device) for v in steps[0])
    s = torch.cuda.Stream(cuda_device)                       # warm-up on a side stream, as torch's docs do: step 1
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        out = one_step(m, opt, utt, start)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):                            # one stream: no parallel branches
        assert loader.build(utt, start, out=out) is out
        hps.masked_pose_l1(m(out["text_tokens"], out["input_kp"]), out["target_kp"], out["n_frames"]).backward()
        opt.step()
    assert opt.steps_done() == 1                             # capturing ran nothing
    for u, st in steps[1:]:
        utt.copy_(torch.tensor(u))
        start.copy_(torch.tensor(st))
        graph.replay()
    torch.cuda.synchronize()
    assert opt.steps_done() == 3
    _assert_same(out, {k: v for k, v in batch_ref.batch(*rec["store"], *steps[2], rec["T"]).items()}, "the last replay's batch")
    twin = _model(cuda_device).train()
    twin_opt = hps.Adam(twin.parameters(), lr=1e-3)
    for u, st in steps:
        one_step(twin, twin_opt, torch.tensor(u, device=cuda_device), torch.tensor(st, device=cuda_device))
    for (k, a), b in zip(m.named_parameters(), twin.parameters()):
        assert torch.equal(a, b), k
    with pytest.raises(ValueError, match="out"):
        loader.build(torch.tensor([1, 2, 3], device=cuda_device), None, out=out)             # a batch of another size
