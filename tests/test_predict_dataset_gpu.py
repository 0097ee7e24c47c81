"""Whole-store inference on the MI355X: b2h_scatter_rows and b2h_joint_error (kernel_scatter_rows.h) against the numpy
restatement tests/rows_ref.py, bit for bit, between poisoned guard bands; the round trip build -> write-back; ids the
store does not have; `predict_dataset` against a hand-written loop for the three models and every `--predict` choice;
against the existing utterance inference path; `joint_pixel_error`; both entry points at the weakest pointer alignment
they promise; `infer --all-frames`."""
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

import batch_ref
import hand_pose_sl_amd as hps
import poison
import rows_ref
from hand_pose_sl_amd import _lib, infer

pytestmark = pytest.mark.gpu
T, FACTOR = 7, 1280.0
DEV = "cuda:0"


def _np_store(name):
    rows, offsets, n_body, tokens = batch_ref.load_fixture(name)["store"]
    return rows.numpy(), offsets.numpy(), n_body, tokens


def _lengths(offsets):
    return (offsets[1:] - offsets[:-1]).tolist()


def _guarded_rows(rows, dev, shift=0):
    """A copy of `rows` between poisoned guard bands: what rows_out starts as."""
    g = poison.Guarded(rows.size * 4, poison.POISON, None, dev, shift)
    g.body.copy_(torch.from_numpy(rows).reshape(-1).view(torch.int32))
    return g


def _scatter(dev, rows, offsets, n_body, utt, start, skip, predict, flags, pred, conf, factor=FACTOR, shift=0):
    """One b2h_scatter_rows launch on guarded operands (all `shift` bytes past the 16-byte grid); returns rows_out as numpy
    after checking every guard band and that no input changed."""
    ins = {"rows": torch.from_numpy(rows), "offsets": torch.from_numpy(offsets), "utt": torch.tensor(utt, dtype=torch.int64),
           "pred": torch.from_numpy(pred)}
    if start is not None:
        ins["start"] = torch.tensor(start, dtype=torch.int64)
    if skip is not None:
        ins["skip"] = torch.tensor(skip, dtype=torch.int64)
    g = {k: poison.guarded_input(v, True, dev, shift) for k, v in ins.items()}
    out = _guarded_rows(rows, dev, shift)
    ptr = lambda k: g[k].ptr if k in g else None
    assert all(b.ptr.value % 16 == shift for b in list(g.values()) + [out])
    rc = _lib.load().b2h_scatter_rows(ptr("rows"), rows.shape[0], ptr("offsets"), offsets.size - 1, n_body, ptr("utt"), ptr("start"),
                                      ptr("skip"), len(utt), T, _lib.PREDICT[predict], flags, factor, ptr("pred"), conf, out.ptr, None)
    torch.cuda.synchronize(dev)
    assert rc == 0, _lib.last_error()
    assert out.guards_intact() and all(b.guards_intact() for b in g.values())
    for k, v in ins.items():
        assert torch.equal(g[k].body, v.contiguous().reshape(-1).to(dev).view(torch.int32)), f"{k}: input modified"
    return out.view(torch.float32, rows.shape).cpu().numpy()


def _pred(B, nt, flags, seed):
    g = np.random.default_rng(seed)
    if flags & rows_ref.NORMALIZE:
        return g.standard_normal((B, T, nt, 2)).astype(np.float32)
    return (g.random((B, T, nt, 2)) * np.array([1280.0, 720.0])).astype(np.float32)      # pixel scale


def _check_scatter(dev, store, utt, start, skip, predict, flags, seed, conf=0.625):
    rows, offsets, n_body, _ = store
    nt = batch_ref.joints(predict, n_body)[1]
    pred = _pred(len(utt), nt, flags, seed)
    want, hit = rows_ref.scatter(rows, offsets, n_body, utt, start, skip, T, predict, flags, FACTOR, pred, conf, rows)
    got = _scatter(dev, rows, offsets, n_body, utt, start, skip, predict, flags, pred, conf)
    assert rows_ref.same_bits(got, want), (predict, flags, utt, start, skip)
    assert rows_ref.same_bits(got[~hit], rows[~hit])                 # every word that is not addressed keeps its bits
    return hit


# json_store: ids 0 .. 4 of 1, 3, 7, 8, 19 frames.  (utt, start, skip): starts the clamp changes (5 -> 1, -4 -> 0, 99 -> 12)
# or ignores (the short utterances); skip None, 0, mid-window, >= n, negative; id 4 twice with disjoint (start, skip).
JSON_BATCHES = [([4, 3, 1], [12, 5, 3], None), ([4, 4, 2], [0, 7, 0], [0, 3, 9]), ([3, 0, 4], [-4, 0, 99], [-2, 0, 2]),
                ([2, 1, 4], None, [1, 3, 6]), ([4, 2, 0], None, None)]


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("predict", batch_ref.PREDICTS)
def test_write_back_equals_the_restatement_json_store(cuda_device, predict, flags):
    store = _np_store("json_store")
    written = 0
    for i, (utt, start, skip) in enumerate(JSON_BATCHES):
        written += int(_check_scatter(cuda_device, store, utt, start, skip, predict, flags, 10 * flags + i).sum())
    assert written > 0


@pytest.mark.parametrize("flags", [0, 1, 2, 3, 7])
def test_write_back_equals_the_restatement_h5_store(cuda_device, flags):
    store = _np_store("h5_store")                                    # ids 0 .. 5 of 0, 1, 3, 7, 8, 19 frames
    for i, (utt, start, skip) in enumerate(JSON_BATCHES):
        _check_scatter(cuda_device, store, [u + 1 for u in utt], start, skip, "right_hand", flags, 50 + 10 * flags + i)
    hit = _check_scatter(cuda_device, store, [0, 5, 0], [0, 6, 0], [0, 1, 0], "right_hand", flags, 99)     # the empty utterance
    assert int(hit.sum()) == 6 * 21 * 3


def test_write_back_other_factor_and_conf(cuda_device):
    rows, offsets, n_body, _ = store = _np_store("json_store")
    pred = _pred(2, 12, 2, 7)
    for conf in (0.0, -1.5):
        want, _ = rows_ref.scatter(rows, offsets, n_body, [4, 1], [3, 0], None, T, "right_3fingers", 3, 3.0, pred, conf, rows)
        got = _scatter(cuda_device, *store[:3], [4, 1], [3, 0], None, "right_3fingers", 3, pred, conf, factor=3.0)
        assert rows_ref.same_bits(got, want)


@pytest.mark.parametrize("name", ["h5_store", "json_store"])
def test_unknown_utterances_write_nothing(cuda_device, name):
    rows, offsets, n_body, _ = _np_store(name)
    n_utt = offsets.size - 1
    broken = offsets.copy()
    broken[n_utt - 2] = broken[n_utt - 3] - 1                        # utterance n_utt - 3 ends before it begins
    beyond = offsets.copy()
    beyond[n_utt] = rows.shape[0] + 5                                # the last utterance ends past the store
    for off, utt in ((offsets, [-1, 1, n_utt, n_utt - 1, -(1 << 40), 1 << 40]), (broken, [n_utt - 3, 1, n_utt - 1]),
                     (beyond, [n_utt - 1, 1, n_utt - 2])):
        pred = _pred(len(utt), 21, 3, 11)
        want, hit = rows_ref.scatter(rows, off, n_body, utt, None, None, T, "right_hand", 3, FACTOR, pred, 1.0, rows)
        got = _scatter(cuda_device, rows, off, n_body, utt, None, None, "right_hand", 3, pred, 1.0)
        assert rows_ref.same_bits(got, want)
        assert rows_ref.same_bits(got[~hit], rows[~hit])
        lo, hi = int(off[1]), int(off[2])
        assert hit[lo:hi].any() and not rows_ref.same_bits(got[lo:hi], rows[lo:hi])      # the neighbour is written ...
        known = [b for b, _, _ in rows_ref.addressed_rows(off, utt, None, None, T, rows.shape[0])]
        assert 0 < len(set(known)) < len(utt)                                            # ... and someone is not


# ---- the round trip ------------------------------------------------------------------------------------------------------
def _dataset(name, dev):
    rows, offsets, n_body, tokens = batch_ref.load_fixture(name)["store"]
    return hps.DeviceDataset(rows, offsets, n_body, tokens=tokens, device=dev)


@pytest.mark.parametrize("name", ["h5_store", "json_store"])
def test_round_trip_build_then_write_back(cuda_device, name):
    """flags 0: the store's right-hand x, y come back bit for bit.  DIF | NORMALIZE: x -> fl(fl(fl(fl(x - w) / f) * f) + w),
    three roundings at 2^-24 of |x - w| and one of the result, 2^-22 max(|x|, |w|, |x - w|); the bound doubles that."""
    ds = _dataset(name, cuda_device)
    rows = ds.rows.cpu().numpy()
    J, h = ds.n_body + 42, ds.n_body + 21
    plan = hps.window_plan(ds, T)
    for dif, norm in ((False, False), (True, True)):
        loader = hps.DeviceLoader(ds, 4, T, selection="first", dif_encoding=dif, normalize=norm)
        batch = loader.build(plan[0], plan[1])
        out = loader.write_back(batch["target_kp"], *plan, torch.zeros_like(ds.rows), conf=0.5).cpu().numpy()
        x, y = rows[:, h:h + 21], rows[:, J + h:J + h + 21]
        gx, gy = out[:, h:h + 21], out[:, J + h:J + h + 21]
        assert (out[:, 2 * J + h:] == 0.5).all() and not out[:, :h].any() and not out[:, J:J + h].any()
        if not dif:
            assert rows_ref.same_bits(gx, x) and rows_ref.same_bits(gy, y)
            continue
        for got, want, w in ((gx, x, rows[:, 4:5]), (gy, y, rows[:, J + 4:J + 5])):
            bound = 2.0 ** -21 * np.maximum(np.maximum(np.abs(want), np.abs(w)), np.abs(want.astype(np.float64) - w))
            err = np.abs(got.astype(np.float64) - want)
            print(f"{name}: round trip max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert (err <= bound).all()


# ---- predict_dataset against the hand-written loop -------------------------------------------------------------------------
def _model(kind, dev, geometry=(12, 42), seed=5):
    torch.manual_seed(seed)
    if kind == "conv":
        m = hps.ConvModel(30, "ReLU", False)
    elif kind == "tenc":
        m = hps.TransformerEnc(24, 4, 128, 42, 1)
    else:
        m = hps.TextPoseTransformer(n_tokens=1000, n_joints=geometry[0], joints_dim=2, nhead=4, nhid=128, nout=geometry[1],
                                    n_enc_layers=1, n_dec_layers=1)
    return m.to(dev).eval()


def _forward(model, loader, batch):
    if not isinstance(model, hps.TextPoseTransformer):
        return model(batch["body_kp"])
    if loader.max_frames > 128:
        return model.forward_long(batch["text_tokens"], batch["input_kp"])
    return model(batch["text_tokens"], batch["input_kp"])


def _loop(model, loader, conf):
    """plan -> build -> model -> the restatement of the write-back, slice by slice."""
    ds, B, Tm = loader.ds, loader.batch_size, loader.max_frames
    rows, offsets = ds.rows.cpu().numpy(), ds.offsets.cpu().numpy()
    utt, start, skip = rows_ref.plan(_lengths(offsets), Tm)
    out = rows.copy()
    model.eval()
    for i in range(0, len(utt), B):
        u, s, k = utt[i:i + B], start[i:i + B], skip[i:i + B]
        with torch.no_grad():
            pred = _forward(model, loader, loader.build(u, s)).cpu().numpy()
        J = ds.n_body + 42
        d = np.arange(batch_ref.TARGET[loader.predict].start, batch_ref.TARGET[loader.predict].stop) + ds.n_body + 21
        f = np.float32(loader.factor)
        for b, t, row in rows_ref.addressed_rows(offsets, u, s, k, Tm, rows.shape[0]):
            x, y = pred[b, t, :, 0], pred[b, t, :, 1]
            if loader.flags & rows_ref.NORMALIZE:
                x, y = x * f, y * f
            if loader.flags & rows_ref.DIF:
                x, y = x + rows[row, 4], y + rows[row, J + 4]
            out[row, d], out[row, J + d], out[row, 2 * J + d] = x, y, np.float32(conf)
    return out


def _check_predict_dataset(model, loader, conf, training):
    ds = loader.ds
    model.train(training)
    got_ds = hps.predict_dataset(model, loader, conf=conf)
    assert model.training is training                                   # the mode is put back
    want = _loop(model, loader, conf)
    got, rows = got_ds.rows.cpu().numpy(), ds.rows.cpu().numpy()
    assert rows_ref.same_bits(got, want)
    assert got_ds.offsets is ds.offsets and got_ds.tokens is ds.tokens and got_ds.n_body == ds.n_body and len(got_ds) == len(ds)
    assert torch.equal(got_ds.lengths, ds.lengths) and got_ds.rows.data_ptr() != ds.rows.data_ptr()
    J = ds.n_body + 42
    d = np.arange(batch_ref.TARGET[loader.predict].start, batch_ref.TARGET[loader.predict].stop) + ds.n_body + 21
    other = np.ones(3 * J, bool)
    other[d] = other[J + d] = other[2 * J + d] = False
    assert rows_ref.same_bits(got[:, other], rows[:, other])            # body, left hand, unpredicted right-hand joints
    assert (got[:, 2 * J + d] == np.float32(conf)).all() and got.shape[0] > 0
    assert not rows_ref.same_bits(got[:, d], rows[:, d])
    return got_ds


PREDICT_CASES = [("conv", "json_store", "right_hand", (12, 42)), ("tenc", "json_store", "right_hand", (12, 42)),
                 ("tpt", "json_store", "right_hand", (12, 42)), ("tpt", "h5_store", "right_hand", (8, 42)),
                 ("tpt", "json_store", "right_index", (29, 8)), ("tpt", "json_store", "right_3fingers", (21, 24))]


@pytest.mark.parametrize("kind,name,predict,geometry", PREDICT_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in PREDICT_CASES])
def test_predict_dataset_equals_the_hand_written_loop(cuda_device, kind, name, predict, geometry):
    ds = _dataset(name, cuda_device)
    model = _model(kind, cuda_device, geometry)
    pad = "frame0" if ds.n_body == 12 else "zeros"
    assert len(hps.window_plan(ds, T)[0]) == 8                          # B = 3 ends on a partial slice, 64 is larger than the plan
    for B, training in ((2, False), (3, True), (64, True)):
        loader = hps.DeviceLoader(ds, B, T, selection="randomcrop", predict=predict, pad=pad, shuffle=True)
        _check_predict_dataset(model, loader, 0.75, training)
    first = hps.predict_dataset(model, hps.DeviceLoader(ds, 2, T, predict=predict, pad=pad), coverage="first", conf=0.75)
    lo, hi = int(ds.offsets[-2]), int(ds.offsets[-1])                   # the 19-frame utterance: 7 rows predicted, 12 kept
    d = 3 * (ds.n_body + 42) - 21 + batch_ref.TARGET[predict].start     # a predicted joint's confidence
    assert torch.equal(first.rows[lo + T:hi], ds.rows[lo + T:hi]) and bool((first.rows[lo:lo + T, d] == 0.75).all())
    assert not torch.equal(first.rows[lo:lo + T], ds.rows[lo:lo + T])


def test_predict_dataset_takes_the_long_path_beyond_128_frames(cuda_device):
    """max_frames = 130 over utterances of 150 and 40 frames: windows (0, 0, 0), (0, 20, 110), (1, 0, 0) through forward_long."""
    g = torch.Generator().manual_seed(31)
    rows = (torch.rand((190, 3, 54), generator=g) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)).reshape(190, 162)
    ds = hps.DeviceDataset(rows, torch.tensor([0, 150, 190]), 12, tokens=torch.randint(0, 1000, (2, 5), generator=g), device=cuda_device)
    assert [t.tolist() for t in hps.window_plan(ds, 130)] == [[0, 0, 1], [0, 20, 0], [0, 110, 0]]
    model = _model("tpt", cuda_device)
    _check_predict_dataset(model, hps.DeviceLoader(ds, 2, 130, pad="frame0"), 1.0, False)


def test_predict_dataset_and_joint_error_refusals(cuda_device):
    js, h5 = _dataset("json_store", cuda_device), _dataset("h5_store", cuda_device)
    conv, tenc, tpt = (_model(k, "cpu") for k in ("conv", "tenc", "tpt"))
    bare = hps.DeviceDataset(js.rows, js.offsets, 12, device=cuda_device)
    cases = [(conv, hps.DeviceLoader(h5, 2, T), {}, "n_body = 12"), (tenc, hps.DeviceLoader(h5, 2, T), {}, "n_body = 12"),
             (conv, hps.DeviceLoader(js, 2, T, predict="right_index"), {}, "predict='right_hand'"),
             (tenc, hps.DeviceLoader(js, 2, 101), {}, "max_frames <= 100"),
             (tpt, hps.DeviceLoader(js, 2, 1025), {}, "max_frames <= 1024"),
             (tpt, hps.DeviceLoader(js, 2, T, predict="right_index"), {}, r"\(n_joints, nout\)"),
             (tpt, hps.DeviceLoader(h5, 2, T), {}, r"\(n_joints, nout\)"),
             (tpt, hps.DeviceLoader(bare, 2, T), {}, "tokens="),
             (conv, hps.DeviceLoader(js, 2, T), {"conf": float("nan")}, "finite"),
             (conv, hps.DeviceLoader(js, 2, T), {"conf": float("inf")}, "finite"),
             (torch.nn.Linear(2, 2), hps.DeviceLoader(js, 2, T), {}, "ConvModel, TransformerEnc and TextPoseTransformer"),
             (conv, js, {}, "DeviceLoader")]
    for model, loader, kw, message in cases:                            # the models live on the host: nothing may launch
        with pytest.raises(ValueError, match=message):
            hps.predict_dataset(model, loader, **kw)
    with pytest.raises(ValueError, match="coverage must be one of"):
        hps.predict_dataset(conv, hps.DeviceLoader(js, 2, T), coverage="last")
    with pytest.raises(ValueError, match="n_body"):
        hps.joint_pixel_error(js, h5)
    shorter = hps.DeviceDataset(js.rows[:-1], torch.cat([js.offsets[:-1], js.offsets[-1:] - 1]), 12, device=cuda_device)
    with pytest.raises(ValueError, match="row count"):
        hps.joint_pixel_error(shorter, js)
    moved = hps.DeviceDataset(js.rows, torch.cat([js.offsets[:1], js.offsets[1:2] + 1, js.offsets[2:]]), 12, device=cuda_device)
    with pytest.raises(ValueError, match="offsets"):
        hps.joint_pixel_error(moved, js)
    with pytest.raises(ValueError, match="shape"):
        js.with_rows(js.rows[:-1])
    with pytest.raises(ValueError, match="float32"):
        js.with_rows(js.rows.double())
    got = js.utterance_rows()
    assert [a.shape for a in got] == [(n, 162) for n in js.lengths.tolist()] and all(a.dtype == np.float32 for a in got)
    assert np.array_equal(np.concatenate(got), js.rows.cpu().numpy())
    again = hps.DeviceDataset.from_h5_rows(h5.utterance_rows(), tokens=h5.tokens, device=cuda_device)
    assert torch.equal(again.rows, h5.rows) and torch.equal(again.offsets, h5.offsets)   # the inverse of from_h5_rows


# ---- against the existing inference path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bar", [("conv", 1.2e-7 * 1280), ("tenc", 2e-5 * 1280), ("tpt", 2e-5 * 1280)])
def test_predict_dataset_agrees_with_predict_utterances(cuda_device, kind, bar):
    """The utterances of json_store that fit into T, staged by both paths: openpose.load_utterance + forward_fused against
    DeviceDataset.from_frames + predict_dataset.  The bar is the model's existing parity bar times the factor."""
    rec = batch_ref.load_fixture("json_store")
    lengths = _lengths(rec["store"][1].numpy())
    fit = [u for u, n in enumerate(lengths) if 0 < n <= T]
    assert [lengths[u] for u in fit] == [1, 3, 7]
    utterances = [rec["frames"][u] for u in fit]
    ids = [rec["store"][3][u].tolist() for u in fit] if kind == "tpt" else None
    model = _model(kind, cuda_device)
    want, n_frames = infer.predict_utterances(model, utterances, T, dif_encoding=False, normalize=True, tokens=ids)
    tokens = None if ids is None else torch.tensor([infer.pad_tokens(t) for t in ids], dtype=torch.int64)
    ds = hps.DeviceDataset.from_frames(utterances, tokens=tokens, device=cuda_device)
    out = hps.predict_dataset(model, hps.DeviceLoader(ds, 2, T, dif_encoding=False, normalize=True, pad="frame0"))
    worst = 0.0
    for u, got in enumerate(out.utterance_rows()):
        n = n_frames[u]
        assert got.shape[0] == n == lengths[fit[u]]
        xy = np.stack([got[:, 33:54], got[:, 54 + 33:108]], axis=2)
        worst = max(worst, float(np.abs(xy.astype(np.float64) - want[u, :n]).max()))
    print(f"{kind}: max |predict_dataset - predict_utterances| = {worst:.3e} px (bar {bar:.3e})")
    assert worst <= bar


# ---- the joint error ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _predicted(name):
    """(the fixture store on the device, predict_dataset's output over it), computed once."""
    ds = _dataset(name, torch.device(DEV))
    model = _model("conv", DEV) if name == "json_store" else _model("tpt", DEV, (8, 42))
    pad = "frame0" if ds.n_body == 12 else "zeros"
    return ds, hps.predict_dataset(model, hps.DeviceLoader(ds, 3, T, pad=pad))


def _sequential_f64(values):
    total = np.zeros(values.shape[1], np.float64)
    for row in values:
        total = total + row.astype(np.float64)
    return total


@pytest.mark.parametrize("name", ["h5_store", "json_store"])
def test_joint_error_equals_the_restatement(cuda_device, name):
    ds, out = _predicted(name)
    rows_pred, rows_true, offsets = out.rows.cpu().numpy(), ds.rows.cpu().numpy(), ds.offsets.cpu().numpy()
    want_sum, want_count = rows_ref.joint_error(rows_pred, rows_true, offsets, ds.n_body)
    res = hps.joint_pixel_error(out, ds)
    assert rows_ref.same_bits(res.utt_sum, want_sum) and rows_ref.same_bits(res.utt_count, want_count)
    assert want_count.sum() > 0 and float(want_sum.max()) > 1.0                       # pixels apart, and counted
    total = _sequential_f64(want_sum)
    assert rows_ref.same_bits(res.total_sum, total) and res.total_sum.dtype == np.float64
    assert res.count.dtype == np.int64 and res.count.tolist() == want_count.astype(np.int64).sum(axis=0).tolist()
    with np.errstate(invalid="ignore", divide="ignore"):
        assert rows_ref.same_bits(res.per_joint, np.where(res.count > 0, total / res.count, np.nan))
    assert res.mean == float(total.sum() / res.count.sum())
    if name == "h5_store":                                                            # the empty utterance: 0 / 0
        assert _lengths(offsets)[0] == 0 and not res.utt_sum[0].any() and not res.utt_count[0].any()
        assert res.utt_sum[0].tobytes() == np.zeros(21, np.float32).tobytes()
    # identical stores: distance 0 on every confident joint
    same = hps.joint_pixel_error(ds, ds)
    J, h = ds.n_body + 42, ds.n_body + 21
    conf = rows_true[:, 2 * J + h:]
    assert not same.utt_sum.any() and same.mean == 0.0
    assert same.count.tolist() == (conf > 0).sum(axis=0).tolist() and same.utt_count.tolist() == want_count.tolist()
    # a joint the true store marks undetected is not counted: zero some confidences in a private copy
    private = rows_true.copy()
    lo = int(offsets[-2])
    dropped = int((private[lo:lo + 5, 2 * J + h + 3] > 0).sum())
    private[lo:lo + 5, 2 * J + h + 3] = 0.0
    private[:, 2 * J + h + 20] = 0.0
    masked = hps.joint_pixel_error(out, ds.with_rows(torch.from_numpy(private).to(cuda_device)))
    m_sum, m_count = rows_ref.joint_error(rows_pred, private, offsets, ds.n_body)
    assert rows_ref.same_bits(masked.utt_sum, m_sum) and rows_ref.same_bits(masked.utt_count, m_count)
    assert masked.utt_count[-1, 3] == want_count[-1, 3] - dropped and masked.count[20] == 0 and np.isnan(masked.per_joint[20])


def test_joint_error_is_the_same_on_every_run_and_stream(cuda_device):
    ds, out = _predicted("json_store")
    base = hps.joint_pixel_error(out, ds)
    for _ in range(2):
        s = torch.cuda.Stream(device=cuda_device)
        s.wait_stream(torch.cuda.current_stream(cuda_device))
        with torch.cuda.stream(s):
            res = hps.joint_pixel_error(out, ds)
        torch.cuda.current_stream(cuda_device).wait_stream(s)
        for k in ("utt_sum", "utt_count", "total_sum", "count", "per_joint"):
            assert rows_ref.same_bits(getattr(res, k), getattr(base, k)), k
        assert res.mean == base.mean


# ---- the weakest alignment each pointer is promised ------------------------------------------------------------------------
def test_scatter_rows_with_every_pointer_at_8_bytes(cuda_device):
    rows, offsets, n_body, _ = _np_store("h5_store")
    utt, start, skip = [5, 5, 3, 0], [0, 12, 0], [0, 2, 3]
    start, skip = start + [0], skip + [0]
    pred = _pred(4, 21, 3, 77)
    want, _ = rows_ref.scatter(rows, offsets, n_body, utt, start, skip, T, "right_hand", 3, FACTOR, pred, 1.0, rows)
    for shift in (0, 8):
        got = _scatter(cuda_device, rows, offsets, n_body, utt, start, skip, "right_hand", 3, pred, 1.0, shift=shift)
        assert rows_ref.same_bits(got, want), shift


def test_joint_error_with_every_pointer_at_its_weakest_alignment(cuda_device):
    """Rows, utt_sum and utt_count are promised 4 bytes (here +4 and +12), offsets and the totals 8 (+8)."""
    ds, out = _predicted("h5_store")
    rows_pred, rows_true, offsets = out.rows.cpu(), ds.rows.cpu(), ds.offsets.cpu()
    U = offsets.numel() - 1
    lib = _lib.load()

    def call(p):
        return lib.b2h_joint_error(p["rows_pred"], p["rows_true"], rows_true.shape[0], p["offsets"], U, ds.n_body, p["utt_sum"],
                                   p["utt_count"], p["total_sum"], p["total_count"], None)
    ins = {"rows_pred": rows_pred, "rows_true": rows_true, "offsets": offsets}
    outs = {"utt_sum": (U, 21), "utt_count": (U, 21), "total_sum": (21, 2), "total_count": (21, 2)}   # 8-byte words count twice
    shifts = {"rows_pred": 4, "rows_true": 12, "offsets": 8, "utt_sum": 12, "utt_count": 4, "total_sum": 8, "total_count": 8}
    runs = []
    for sh in ({}, shifts):
        def placed(p, sh=sh):
            assert all(p[k].value % 16 == sh.get(k, 0) for k in list(ins) + list(outs))
            return call(p)
        runs.append(poison.launch(placed, ins, outs, cuda_device, shifts=sh))
    for k in outs:
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), k
    want_sum, want_count = rows_ref.joint_error(rows_pred.numpy(), rows_true.numpy(), offsets.numpy(), ds.n_body)
    assert rows_ref.same_bits(runs[1]["utt_sum"].cpu().numpy(), want_sum)
    assert rows_ref.same_bits(runs[1]["utt_count"].cpu().view(torch.int32).numpy(), want_count)
    assert rows_ref.same_bits(runs[1]["total_sum"].cpu().view(torch.float64).numpy().reshape(21), _sequential_f64(want_sum))
    assert runs[1]["total_count"].cpu().view(torch.int64).reshape(21).tolist() == want_count.astype(np.int64).sum(axis=0).tolist()


# ---- the CLI -------------------------------------------------------------------------------------------------------------
def test_infer_all_frames_writes_every_frame(cuda_device, tmp_path):
    rec = batch_ref.load_fixture("json_store")
    frames = rec["frames"][4]
    assert len(frames) == 19
    data = tmp_path / "utt"
    data.mkdir()
    for i, fr in enumerate(frames):
        (data / f"{i:04d}_keypoints.json").write_text(json.dumps(fr))
    model = _model("conv", cuda_device)
    ckpt = tmp_path / "model.pth"
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, ckpt)
    common = ["--data", str(data), "--model-checkpoint", str(ckpt), "--max-frames", str(T)]

    def hands(folder):
        files = sorted(glob.glob(os.path.join(folder, "*.json")))
        return np.array([json.load(open(f))["people"][0]["hand_right_keypoints_2d"] for f in files]).reshape(len(files), 21, 3)
    for extra, dif in (([], False), (["--dif-encoding"], True)):
        out = tmp_path / ("all_dif" if dif else "all")
        infer.main(common + ["--output-folder", str(out), "--all-frames"] + extra)
        got = hands(str(out))
        assert got.shape[0] == 19
        ds = hps.DeviceDataset.from_frames([frames], device=cuda_device)
        want = hps.predict_dataset(model, hps.DeviceLoader(ds, 128, T, dif_encoding=dif, normalize=True, pad="frame0")).rows.cpu().numpy()
        assert np.array_equal(got[:, :, 0].astype(np.float32), want[:, 33:54]) and np.array_equal(got[:, :, 1].astype(np.float32), want[:, 87:108])
        assert (got[:, :, 2] == 1.0).all()
        assert not np.array_equal(want[:, 33:54], ds.rows.cpu().numpy()[:, 33:54])
    infer.main(common + ["--output-folder", str(tmp_path / "first")])                    # without the flag: 7 files, as before
    assert hands(str(tmp_path / "first")).shape[0] == T
