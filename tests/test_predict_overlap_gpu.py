"""Overlapping inference windows on the MI355X: b2h_scatter_rows_blend (kernel_scatter_rows.h) against the numpy
restatement tests/blend_ref.py, bit for bit, into a poisoned store between poisoned guard bands, for both blends, every
`--predict` choice and transform, in batches of 1, 3 and the whole plan and in either launch order; a plan without
overlap against b2h_scatter_rows; CENTRE as a pure select; `predict_dataset(overlap=K)` against a hand-written loop for
the three models and on the long path; overlap 0 against the call without it; runs and streams; the halo property of
ConvModel that is the point of the feature; the weakest pointer alignment; `infer --all-frames --overlap`."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import batch_ref
import blend_ref
import hand_pose_sl_amd as hps
import poison
import rows_ref
from hand_pose_sl_amd import _lib, infer

pytestmark = pytest.mark.gpu
FACTOR = 1280.0
SHAPES = [(8, 4), (13, 5)]                                            # (T, K): an even overlap of T / 2, an odd one below it


def _lengths(T, K):
    return [0, 1, T, T + 1, 2 * T - K, 2 * T - K + 1, 5 * T + 3]


def _store(T, K, seed=0):
    """(rows, offsets) numpy of a 12-joint store in pixel units with the utterance lengths the plan branches on."""
    lengths = _lengths(T, K)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    g = np.random.default_rng(1000 * T + K + seed)
    rows = (g.random((int(offsets[-1]), 3, 54)) * np.array([1280.0, 720.0, 1.0]).reshape(1, 3, 1)).astype(np.float32)
    return rows.reshape(-1, 162), offsets


def _plan_with_strangers(T, K):
    """The plan of the store, with two entries of utterances the store does not have: one between two utterances, one at
    the end.  They write nothing and are nobody's predecessor or successor."""
    utt, start, skip = blend_ref.plan(_lengths(T, K), T, K)
    at = utt.index(4)
    for pos, stranger in ((at, len(_lengths(T, K)) + 2), (len(utt) + 1, -1)):
        utt.insert(pos, stranger), start.insert(pos, 3), skip.insert(pos, 1)
    return utt, start, skip


def _pred(n, T, nt, flags, seed):
    g = np.random.default_rng(seed)
    if flags & rows_ref.NORMALIZE:
        return g.standard_normal((n, T, nt, 2)).astype(np.float32)
    return (g.random((n, T, nt, 2)) * np.array([1280.0, 720.0])).astype(np.float32)      # pixel scale


def _blend_run(dev, store, plan, T, predict, flags, preds, blend, conf, batch, shift=0, reverse=False):
    """The plan written back by b2h_scatter_rows_blend in batches of `batch` entries, on guarded operands (all `shift` bytes
    past the 16-byte grid), into a store that holds POISON everywhere; returns rows_out as numpy after checking every guard
    band and that no input changed."""
    rows, offsets = store
    ins = {"rows": torch.from_numpy(rows), "offsets": torch.from_numpy(offsets), "utt": torch.tensor(plan[0], dtype=torch.int64),
           "start": torch.tensor(plan[1], dtype=torch.int64), "skip": torch.tensor(plan[2], dtype=torch.int64)}
    g = {k: poison.guarded_input(v, True, dev, shift) for k, v in ins.items()}
    out = poison.guarded_output(rows.size * 4, True, dev, shift)
    n_plan, lib = len(plan[0]), _lib.load()
    firsts = list(range(0, n_plan, batch))
    for i in (firsts[::-1] if reverse else firsts):
        B = min(batch, n_plan - i)
        gp = poison.guarded_input(torch.from_numpy(preds[i:i + B]), True, dev, shift)
        gb = poison.guarded_input(torch.from_numpy(preds[i - 1]), True, dev, shift) if i else None
        assert all(b.ptr.value % 16 == shift for b in list(g.values()) + [out, gp] + ([gb] if gb else []))
        rc = lib.b2h_scatter_rows_blend(g["rows"].ptr, rows.shape[0], g["offsets"].ptr, offsets.size - 1, 12, g["utt"].ptr,
                                        g["start"].ptr, g["skip"].ptr, n_plan, i, B, T, _lib.PREDICT[predict], flags, FACTOR,
                                        gp.ptr, gb.ptr if gb else None, blend, conf, out.ptr, None)
        torch.cuda.synchronize(dev)
        assert rc == 0, _lib.last_error()
        assert gp.guards_intact() and (gb is None or gb.guards_intact())
        assert torch.equal(gp.body, torch.from_numpy(preds[i:i + B]).reshape(-1).to(dev).view(torch.int32)), "pred modified"
    assert out.guards_intact() and all(b.guards_intact() for b in g.values())
    for k, v in ins.items():
        assert torch.equal(g[k].body, v.contiguous().reshape(-1).to(dev).view(torch.int32)), f"{k}: input modified"
    return out.view(torch.float32, rows.shape).cpu().numpy()


def _poisoned(rows):
    return np.full(rows.shape, poison.POISON, np.uint32).view(np.float32)          # as bits: no conversion touches the NaN


# ---- the kernel against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("predict", batch_ref.PREDICTS)
def test_blend_write_back_equals_the_restatement(cuda_device, predict, flags):
    nt = batch_ref.joints(predict, 12)[1]
    for T, K in SHAPES:
        rows, offsets = store = _store(T, K)
        plan = _plan_with_strangers(T, K)
        n_plan = len(plan[0])
        preds = _pred(n_plan, T, nt, flags, 100 * T + flags)
        for blend in (blend_ref.LINEAR, blend_ref.CENTRE):
            want, hit, mixed = blend_ref.scatter(rows, offsets, 12, *plan, T, predict, flags, FACTOR, preds, blend, 0.625,
                                                 _poisoned(rows))
            assert hit.any(axis=1).all() and hit.sum() == rows.shape[0] * nt * 3       # every row owned, by the target joints
            assert mixed.sum() == K * (n_plan - 2 - 6)                                 # K rows per boundary: 6 utterances, 2 strangers
            for batch, reverse in ((1, False), (3, False), (n_plan, False), (3, True)):
                got = _blend_run(cuda_device, store, plan, T, predict, flags, preds, blend, 0.625, batch, reverse=reverse)
                assert rows_ref.same_bits(got, want), (T, K, blend, batch, reverse)
                written = got.view(np.uint32) != poison.POISON
                assert np.array_equal(written, hit) and int(written.sum()) == int(hit.sum())


def test_blend_changes_only_the_blend_regions(cuda_device):
    """Outside the K rows behind each window boundary both blends write what a window alone predicts; inside them LINEAR
    mixes the two windows and CENTRE takes one, so the three differ there."""
    T, K = SHAPES[1]
    rows, offsets = store = _store(T, K)
    plan = blend_ref.plan(_lengths(T, K), T, K)
    preds = _pred(len(plan[0]), T, 21, 3, 5)
    lin, cen = (_blend_run(cuda_device, store, plan, T, "right_hand", 3, preds, b, 1.0, 4) for b in (0, 1))
    _, _, mixed = blend_ref.scatter(rows, offsets, 12, *plan, T, "right_hand", 3, FACTOR, preds, 0, 1.0, rows)
    assert rows_ref.same_bits(lin[~mixed], cen[~mixed]) and mixed.sum() > 0
    assert all(not rows_ref.same_bits(lin[r], cen[r]) for r in np.flatnonzero(mixed))


@pytest.mark.parametrize("T", [7, 8])
def test_plan_without_overlap_gives_the_bits_of_scatter_rows(cuda_device, T):
    rows, offsets = _store(T, 0, seed=1)
    ds = hps.DeviceDataset(torch.from_numpy(rows), torch.from_numpy(offsets), 12, device=cuda_device)
    plan = hps.window_plan(ds, T)
    assert [t.tolist() for t in plan] == [t.tolist() for t in hps.window_plan(ds, T, overlap=0)]
    n_plan = plan[0].numel()
    for predict, flags in (("right_hand", (True, True)), ("right_3fingers", (False, True)), ("right_index", (True, False))):
        loader = hps.DeviceLoader(ds, 3, T, predict=predict, dif_encoding=flags[0], normalize=flags[1])
        pred = torch.from_numpy(_pred(n_plan, T, loader.joints[1], loader.flags, T)).to(cuda_device)
        want = torch.full_like(ds.rows, float("nan"))
        for i in range(0, n_plan, 3):
            loader.write_back(pred[i:i + 3], plan[0][i:i + 3], plan[1][i:i + 3], plan[2][i:i + 3], want, conf=0.5)
        for blend in ("linear", "centre"):
            got = torch.full_like(ds.rows, float("nan"))
            for i in range(0, n_plan, 3):
                assert loader.write_back_blend(pred[i:i + 3], plan, i, got, pred[i - 1] if i else None, blend, conf=0.5) is got
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (predict, blend)
        assert not torch.isnan(want[:, 3 * 54 - 21 + batch_ref.TARGET[predict].start]).any()


@pytest.mark.parametrize("T,K", SHAPES)
def test_centre_picks_one_window(cuda_device, T, K):
    """Every written value is fl(fl(p * f) + w) of ONE window's prediction: the predecessor's for the first ceil(K / 2)
    frames of a blend region (2 p < K), the window's own elsewhere."""
    rows, offsets = store = _store(T, K)
    utt, start, skip = plan = blend_ref.plan(_lengths(T, K), T, K)
    preds = _pred(len(utt), T, 21, 3, 9)
    got = _blend_run(cuda_device, store, plan, T, "right_hand", 3, preds, blend_ref.CENTRE, 1.0, 3)
    f = np.float32(FACTOR)
    taken = {"own": 0, "before": 0}
    for e, t, row, region in blend_ref.owned(offsets, utt, start, skip, T, rows.shape[0]):
        own, before = preds[e, t], None if region is None else preds[e - 1, region[0]]
        assert region is None or (start[e] + t == start[e - 1] + region[0] and utt[e] == utt[e - 1])    # the same row of the store
        pick = "before" if region is not None and 2 * region[1] < region[2] else "own"
        p = before if pick == "before" else own
        assert rows_ref.same_bits(got[row, 33:54], p[:, 0] * f + rows[row, 4]), (e, t, pick)
        assert rows_ref.same_bits(got[row, 87:108], p[:, 1] * f + rows[row, 58]), (e, t, pick)
        if region is not None:
            other = own if pick == "before" else before
            assert not rows_ref.same_bits(got[row, 33:54], other[:, 0] * f + rows[row, 4])
        taken[pick] += region is not None
    boundaries = len(utt) - 6
    assert taken == {"own": boundaries * (K // 2), "before": boundaries * (K - K // 2)}


def test_every_pointer_at_8_bytes(cuda_device):
    """pred and pred_before are read as float2 and the plan as int64: 8 bytes is what each is promised."""
    T, K = SHAPES[1]
    rows, offsets = store = _store(T, K)
    plan = _plan_with_strangers(T, K)
    preds = _pred(len(plan[0]), T, 21, 3, 77)
    want, _, _ = blend_ref.scatter(rows, offsets, 12, *plan, T, "right_hand", 3, FACTOR, preds, 0, 1.0, _poisoned(rows))
    for shift in (0, 8):
        got = _blend_run(cuda_device, store, plan, T, "right_hand", 3, preds, 0, 1.0, 3, shift=shift)
        assert rows_ref.same_bits(got, want), shift


# ---- predict_dataset against the hand-written loop -------------------------------------------------------------------------
def _dataset(dev, lengths, S=9, seed=31):
    g = torch.Generator().manual_seed(seed)
    n = sum(lengths)
    rows = (torch.rand((n, 3, 54), generator=g) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)).reshape(n, 162)
    offsets = torch.tensor([0] + np.cumsum(lengths).tolist())
    return hps.DeviceDataset(rows, offsets, 12, tokens=torch.randint(0, 1000, (len(lengths), S), generator=g), device=dev)


def _model(kind, dev, seed=5):
    torch.manual_seed(seed)
    if kind == "conv":
        m = hps.ConvModel(30, "ReLU", False)
    elif kind == "tenc":
        m = hps.TransformerEnc(24, 4, 128, 42, 1)
    else:
        m = hps.TextPoseTransformer(n_tokens=1000, n_joints=12, joints_dim=2, nhead=4, nhid=128, nout=42, n_enc_layers=1,
                                    n_dec_layers=1)
    return m.to(dev).eval()


def _forward(model, loader, batch):
    if not isinstance(model, hps.TextPoseTransformer):
        return model(batch["body_kp"])
    if loader.max_frames > 128:
        return model.forward_long(batch["text_tokens"], batch["input_kp"])
    return model(batch["text_tokens"], batch["input_kp"])


def _loop(model, loader, K, blend, conf):
    """window_plan(overlap=K) -> build -> model, slice by slice as predict_dataset cuts them, then the numpy blend."""
    ds, B, T = loader.ds, loader.batch_size, loader.max_frames
    rows, offsets = ds.rows.cpu().numpy(), ds.offsets.cpu().numpy()
    utt, start, skip = (t.tolist() for t in hps.window_plan(ds, T, overlap=K))
    assert (utt, start, skip) == blend_ref.plan(ds.lengths.tolist(), T, K)
    preds = []
    for i in range(0, len(utt), B):
        with torch.no_grad():
            preds.append(_forward(model, loader, loader.build(utt[i:i + B], start[i:i + B])).cpu().numpy())
    return blend_ref.scatter(rows, offsets, ds.n_body, utt, start, skip, T, loader.predict, loader.flags, loader.factor,
                             np.concatenate(preds), _lib.BLEND[blend], conf, rows)


def _check_predict_dataset(model, loader, K, blend, conf=0.75, training=False):
    ds = loader.ds
    model.train(training)
    got_ds = hps.predict_dataset(model, loader, conf=conf, overlap=K, blend=blend)
    assert model.training is training                                      # the mode is put back
    model.eval()
    want, hit, mixed = _loop(model, loader, K, blend, conf)
    got, rows = got_ds.rows.cpu().numpy(), ds.rows.cpu().numpy()
    assert rows_ref.same_bits(got, want) and mixed.sum() > 0
    assert rows_ref.same_bits(got[~hit], rows[~hit]) and hit.any(axis=1).all()
    assert got_ds.offsets is ds.offsets and got_ds.tokens is ds.tokens and got_ds.rows.data_ptr() != ds.rows.data_ptr()
    assert (got[:, 3 * 54 - 21:] == np.float32(conf)).all()
    return got_ds, mixed


@pytest.mark.parametrize("kind", ["conv", "tenc", "tpt"])
def test_predict_dataset_with_overlap_equals_the_hand_written_loop(cuda_device, kind):
    T, K = 16, 6
    ds = _dataset(cuda_device, [0, 1, T, T + 1, 2 * T - K, 2 * T - K + 1, 5 * T + 3])
    assert hps.window_plan(ds, T, overlap=K)[0].numel() == 17 and ds.tokens.shape[1] == 9
    model = _model(kind, cuda_device)
    for B, blend in ((2, "linear"), (3, "centre"), (64, "linear")):        # predecessors in the batch, before it, one batch
        loader = hps.DeviceLoader(ds, B, T, selection="randomcrop", pad="frame0", shuffle=True)
        _check_predict_dataset(model, loader, K, blend, training=B == 3)


def test_predict_dataset_with_overlap_on_the_long_path(cuda_device):
    """max_frames = 136, overlap 40 over utterances of 300 and 40 frames: windows at 0, 96 and (164, skip 28), and (1, 0, 0),
    through forward_long in batches of 2: the second boundary's predecessor comes from the batch before."""
    ds = _dataset(cuda_device, [300, 40], S=5)
    assert [t.tolist() for t in hps.window_plan(ds, 136, overlap=40)] == [[0, 0, 0, 1], [0, 96, 164, 0], [0, 0, 28, 0]]
    _, mixed = _check_predict_dataset(_model("tpt", cuda_device), hps.DeviceLoader(ds, 2, 136, pad="frame0"), 40, "linear", 1.0)
    assert np.flatnonzero(mixed).tolist() == list(range(96, 136)) + list(range(192, 232))


def test_overlap_zero_runs_and_streams_give_the_same_bits(cuda_device):
    T = 16
    ds = _dataset(cuda_device, [0, 1, T, T + 1, 26, 27, 83])
    model = _model("conv", cuda_device)
    loader = hps.DeviceLoader(ds, 3, T, pad="frame0")
    plain = hps.predict_dataset(model, loader, conf=0.75)
    for blend in ("linear", "centre"):
        assert torch.equal(hps.predict_dataset(model, loader, conf=0.75, overlap=0, blend=blend).rows.view(torch.int32),
                           plain.rows.view(torch.int32))
    for blend in ("linear", "centre"):
        base = hps.predict_dataset(model, loader, conf=0.75, overlap=6, blend=blend)
        assert not torch.equal(base.rows, plain.rows)
        again = hps.predict_dataset(model, loader, conf=0.75, overlap=6, blend=blend)
        s = torch.cuda.Stream(device=cuda_device)
        s.wait_stream(torch.cuda.current_stream(cuda_device))
        with torch.cuda.stream(s):
            aside = hps.predict_dataset(model, loader, conf=0.75, overlap=6, blend=blend)
        torch.cuda.current_stream(cuda_device).wait_stream(s)
        assert torch.equal(again.rows.view(torch.int32), base.rows.view(torch.int32))
        assert torch.equal(aside.rows.view(torch.int32), base.rows.view(torch.int32))


def test_refusals_of_the_python_surface(cuda_device):
    T = 16
    ds = _dataset(cuda_device, [1, 40])
    conv = _model("conv", "cpu")                                           # on the host: nothing may launch
    loader = hps.DeviceLoader(ds, 2, T)
    for kw, message in ((dict(overlap=9), r"overlap must be in 0 \.\. max_frames // 2 = 8"), (dict(overlap=-1), "overlap must be in"),
                        (dict(overlap=2, blend="cubic"), "blend must be one of"),
                        (dict(overlap=2, coverage="first"), "needs coverage='all'")):
        with pytest.raises(ValueError, match=message):
            hps.predict_dataset(conv, loader, **kw)
    plan = hps.window_plan(ds, T, overlap=4)
    assert plan[0].numel() == 4
    pred = torch.zeros((2, T, 21, 2), device=cuda_device)
    out = ds.rows.clone()
    for args, kw, message in (((pred, plan, 2, out), {}, "prediction_before"), ((pred, plan, 3, out), {}, "not in a plan of 4"),
                              ((pred, plan, -1, out), {}, "not in a plan of 4"), ((pred, plan[:2], 0, out), {}, "utt, start, skip"),
                              ((pred, plan, 0, out), {"blend": "cubic"}, "blend must be one of"),
                              ((pred[:, :8], plan, 0, out), {}, "prediction must be"),
                              ((pred, plan, 2, out, pred), {}, "prediction_before must be"),
                              ((pred, plan, 0, out[:-1]), {}, "rows_out must be")):
        with pytest.raises(ValueError, match=message):
            loader.write_back_blend(*args, **kw)
    assert torch.equal(out, ds.rows)


# ---- the property that shows the point ------------------------------------------------------------------------------------
def test_conv_model_with_enough_halo_equals_the_whole_utterance(cuda_device):
    """ConvModel sees 8 frames to either side (four kernel-5 layers).  Windows of 32 frames that overlap by 16 and keep,
    of every frame predicted twice, the prediction nearer to its window's centre (blend="centre") leave every kept frame
    at least 8 frames inside its window, so the result is the prediction of the whole 70-frame utterance at once: the
    same fp32 convolution of the same inputs, different at most in summation order, held to the project's fp32 parity bar
    of 2e-5 on the unit-scale store the bar is stated for.  Windows that only touch differ from it next to every boundary
    (the CPU oracle shows 5e-2 for this seed, tests/test_predict_overlap_cpu.py).  Measured on one MI355X: max|B - A| = 0,
    max|C - A| = 5.33e-2 within 8 frames of a boundary and 0 elsewhere, at max|A| = 0.113."""
    rows = blend_ref.halo_rows()
    ds = hps.DeviceDataset(torch.from_numpy(rows), torch.tensor(blend_ref.HALO_OFFSETS), 12, device=cuda_device)
    torch.manual_seed(blend_ref.HALO_SEED)
    model = hps.ConvModel(30, "ReLU", False).to(cuda_device).eval()
    loader = lambda T: hps.DeviceLoader(ds, 8, T, dif_encoding=False, normalize=False)
    hand = lambda d: np.concatenate([d.rows.cpu().numpy()[:, 33:54], d.rows.cpu().numpy()[:, 87:108]], axis=1).astype(np.float64)
    A = hand(hps.predict_dataset(model, loader(70)))
    B = hand(hps.predict_dataset(model, loader(32), overlap=16, blend="centre"))
    C = hand(hps.predict_dataset(model, loader(32), overlap=0))
    near = blend_ref.near_seams(32)
    halo, seam, away = np.abs(B - A).max(), np.abs(C - A)[near].max(), np.abs(C - A)[~near].max()
    print(f"halo: max|B - A| = {halo:.3e} (bar 2e-5); touching windows: max|C - A| = {seam:.3e} within 8 frames of a "
          f"boundary, {away:.3e} elsewhere; max|A| = {np.abs(A).max():.3e}")
    assert halo <= 2e-5
    assert seam > 1e-3
    assert away <= 2e-5


# ---- the CLI -------------------------------------------------------------------------------------------------------------
def test_infer_all_frames_with_overlap_writes_every_frame(cuda_device, tmp_path):
    T, K = 16, 6
    frames = batch_ref.load_fixture("json_store")["frames"][4]
    assert len(frames) == 19
    data = tmp_path / "utt"
    data.mkdir()
    for i, fr in enumerate(frames):
        (data / f"{i:04d}_keypoints.json").write_text(json.dumps(fr))
    model = _model("conv", cuda_device)
    ckpt = tmp_path / "model.pth"
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, ckpt)
    common = ["--data", str(data), "--model-checkpoint", str(ckpt), "--max-frames", str(T), "--all-frames"]

    def hands(folder):
        files = sorted(glob.glob(os.path.join(folder, "*.json")))
        return np.array([json.load(open(f))["people"][0]["hand_right_keypoints_2d"] for f in files]).reshape(len(files), 21, 3)
    infer.main(common + ["--output-folder", str(tmp_path / "touch"), "--overlap", "0"])
    touch = hands(str(tmp_path / "touch"))
    ds = hps.DeviceDataset.from_frames([frames], device=cuda_device)
    plan = blend_ref.plan([19], T, K)
    assert plan == ([0, 0], [0, 3], [0, 7])
    mixed = np.zeros(19, bool)
    mixed[[row for _, _, row, region in blend_ref.owned([0, 19], *plan, T) if region is not None]] = True
    assert np.flatnonzero(mixed).tolist() == list(range(10, 16))
    for blend in ("linear", "centre"):
        out = tmp_path / blend
        infer.main(common + ["--output-folder", str(out), "--overlap", str(K), "--blend", blend])
        got = hands(str(out))
        assert got.shape[0] == 19 and (got[:, :, 2] == 1.0).all()
        loader = hps.DeviceLoader(ds, 128, T, dif_encoding=False, normalize=True, pad="frame0")
        want = hps.predict_dataset(model, loader, overlap=K, blend=blend).rows.cpu().numpy()
        assert np.array_equal(got[:, :, 0].astype(np.float32), want[:, 33:54]) and np.array_equal(got[:, :, 1].astype(np.float32), want[:, 87:108])
        differs = (got[:, :, :2] != touch[:, :, :2]).any(axis=(1, 2))
        assert differs.any() and not differs[~mixed].any()                 # only blended rows differ from touching windows
