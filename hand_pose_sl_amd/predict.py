"""A trained model over a whole keypoint store: the counterpart of the reference's `infer_utterance_h5.py` ->
steps/traintest.py:332-391, which runs the model over the store in batches and writes the predictions out as store rows.

  window_plan(...)       windows of `max_frames` frames that cover every frame of every utterance exactly once
                         (b2h_window_plan, a host function)
  predict_dataset(...)   plan -> DeviceLoader.build -> model -> DeviceLoader.write_back (b2h_scatter_rows), slice by
                         slice of the plan; returns a new DeviceDataset.  overlap=K: windows that overlap by K frames
                         (b2h_window_plan_overlap), blended in the write-back (b2h_scatter_rows_blend)
  joint_pixel_error(...) per-utterance, per-joint Euclidean pixel error of one store's right hands against another's
                         (b2h_joint_error), deterministic

The write-back undoes the loader's target transforms: * factor, and + the raw wrist under `dif_encoding`, which the
reference leaves as a TODO (traintest.py:275-279), so a model trained with `--dif-encoding` lands in the image.
"""
import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .conv_model import ConvModel
from .dataset import DeviceDataset, DeviceLoader, _ptr
from .padding import check_mask_padding, padding_lengths
from .text_pose_transformer import TextPoseTransformer
from .transformer_enc import TransformerEnc


def window_plan(offsets_or_dataset, max_frames, coverage="all", overlap=0):
    """(utt, start, skip) host int64 tensors: the windows of `max_frames` frames that predict a store.  "all": every row
    is addressed by exactly one (entry, frame >= skip) -- an utterance longer than max_frames gets ceil(len / max_frames)
    windows, the last a full one ending with the utterance whose first `skip` frames the one before it covers;
    "first": one window at 0 per utterance (the reference's `--frames-selection first`).  Empty utterances get none.
    `overlap` K > 0 ("all" only, K <= max_frames // 2; b2h_window_plan_overlap): the windows of a long utterance lie
    max_frames - K apart, so each begins its used frames K rows before the one before it ends -- the rows that
    `DeviceLoader.write_back_blend` blends.  `offsets_or_dataset`: a DeviceDataset, or its (U + 1) ascending int64
    offsets."""
    if coverage not in _lib.COVERAGE:
        raise ValueError(f"coverage must be one of {sorted(_lib.COVERAGE)}, got {coverage!r}")
    overlap = int(overlap)
    if overlap and coverage != "all":
        raise ValueError(f"overlap={overlap} needs coverage='all': with coverage={coverage!r} an utterance has one window")
    src = offsets_or_dataset.offsets if isinstance(offsets_or_dataset, DeviceDataset) else offsets_or_dataset
    off = torch.as_tensor(src).detach().cpu().contiguous()
    if off.dtype != torch.int64 or off.dim() != 1 or off.numel() < 1:
        raise ValueError(f"offsets must be (U + 1,) int64, got {tuple(off.shape)} {off.dtype}")
    i64p = ctypes.POINTER(ctypes.c_int64)
    lib, n_utt = _lib.load(), off.numel() - 1
    host = lambda t: ctypes.cast(t.data_ptr(), i64p) if t.numel() else None
    if overlap:
        fill = lambda *out: lib.b2h_window_plan_overlap(host(off), n_utt, int(max_frames), overlap, *out)
    else:
        fill = lambda *out: lib.b2h_window_plan(host(off), n_utt, int(max_frames), _lib.COVERAGE[coverage], *out)
    count = fill(None, None, None, 0)
    if count < 0:
        raise ValueError(_lib.last_error())
    plan = [torch.empty(count, dtype=torch.int64) for _ in range(3)]
    if fill(*[host(t) for t in plan], count) != count:
        raise RuntimeError(f"libb2h: {_lib.last_error()}")
    return tuple(plan)


def _check(model, loader, conf):
    """The refusals of predict_dataset, before any GPU work.  Returns whether the model takes tokens."""
    if not isinstance(loader, DeviceLoader):
        raise ValueError("predict_dataset() reads the store through a DeviceLoader: wrap the DeviceDataset in "
                         "DeviceLoader(ds, batch_size, max_frames, ...) with the trainer's transforms")
    if loader.augment is not None:
        raise ValueError("predict_dataset() writes predictions back into store coordinates, which a scaled, rotated or "
                         "mirrored window no longer has: use a DeviceLoader with augment=None")
    if not math.isfinite(conf):
        raise ValueError(f"conf must be a finite confidence for the predicted joints, got {conf!r}")
    ds, T = loader.ds, loader.max_frames
    if isinstance(model, TextPoseTransformer):
        if T > 1024:
            raise ValueError(f"TextPoseTransformer runs at most 1024 frames per window: use a DeviceLoader with max_frames <= 1024, got {T}")
        want = (loader.joints[0], 2 * loader.joints[1])
        if (model.ninp // 2, model.nout) != want:
            raise ValueError(f"the model's (n_joints, nout) = {(model.ninp // 2, model.nout)} but the loader builds {want} "
                             f"for predict={loader.predict!r} over a {ds.n_body}-joint body: use the matching model or loader")
        if ds.tokens is None:
            raise ValueError("a TextPoseTransformer needs the store's tokens: build the DeviceDataset with tokens=")
        return True
    if not isinstance(model, (ConvModel, TransformerEnc)):
        raise ValueError(f"predict_dataset() runs ConvModel, TransformerEnc and TextPoseTransformer, not {type(model).__name__}")
    if ds.n_body != 12 or loader.predict != "right_hand":
        raise ValueError(f"{type(model).__name__} takes 12 body joints and predicts the right hand: use a store from "
                         f"OpenPose JSON (n_body = 12) and a loader with predict='right_hand', or a TextPoseTransformer")
    if isinstance(model, TransformerEnc) and T > model.pos_encoder.pe.shape[0]:
        raise ValueError(f"TransformerEnc has {model.pos_encoder.pe.shape[0]} positional rows: use a DeviceLoader with "
                         f"max_frames <= {model.pos_encoder.pe.shape[0]}, got {T}")
    return False


def predict_dataset(model, loader, coverage="all", conf=1.0, mask_padding=False, overlap=0, blend="linear"):
    """Run `model` over the whole store of `loader` (a DeviceLoader: it supplies the store, batch_size, max_frames,
    predict, the transforms, the factor and the pad; its selection and shuffle are not used) and return a DeviceDataset
    with the same offsets, tokens and n_body whose predicted right-hand joints hold the predictions in store units --
    * factor, + the raw wrist under dif_encoding -- with confidence `conf`; every other word is the input store's.
    coverage "all" predicts every frame (`window_plan`), "first" the first max_frames of each utterance.  The model
    runs in eval mode under no_grad in the precision it is set to (its mode is restored), dispatched as validate()
    dispatches; the loop does no host synchronisation.  mask_padding (TextPoseTransformer only, else ValueError):
    every window runs with its key-padding masks, text_lengths = token_lengths(tokens) and frame_lengths = the window's
    n_frames, as train_epoch(mask_padding=True) trains; a model trained with masks must be run with them.
    overlap K (0 .. max_frames // 2, coverage "all"): the windows of an utterance longer than max_frames overlap by K
    frames (`window_plan(..., overlap=K)`) and `DeviceLoader.write_back_blend` blends the two predictions of those
    frames -- blend "linear": a cross-fade, "centre": each frame from the window whose centre is nearer --, so no frame
    next to a window boundary is predicted with context on one side only.  With K = 0 the calls and the result are
    exactly those of a call without it."""
    mask_padding = check_mask_padding("predict_dataset()", model, mask_padding)
    text = _check(model, loader, conf)
    overlap = int(overlap)
    if not 0 <= overlap <= loader.max_frames // 2:
        raise ValueError(f"overlap must be in 0 .. max_frames // 2 = {loader.max_frames // 2} (a frame is predicted by at "
                         f"most two windows), got {overlap}")
    if blend not in _lib.BLEND:
        raise ValueError(f"blend must be one of {sorted(_lib.BLEND)}, got {blend!r}")
    ds, B = loader.ds, loader.batch_size
    plan = utt, start, skip = [t.to(ds.device) for t in window_plan(ds, loader.max_frames, coverage, overlap)]
    before = None    # overlap > 0: the prediction of the plan entry before the batch, a view that keeps its batch alive
    rows_out = ds.rows.clone()
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            batch = None
            for i in range(0, utt.numel(), B):
                u, s, k = utt[i:i + B], start[i:i + B], skip[i:i + B]
                if batch is None or batch["n_frames"].shape[0] != u.numel():
                    batch = loader.empty_batch(u.numel())
                loader.build(u, s, out=batch)
                if not text:
                    prediction = model(batch["body_kp"])
                elif loader.max_frames > 128:   # model(tokens, pose) keeps its 128-frame limit: the long path
                    lengths = padding_lengths(batch, ds.device) if mask_padding else {}
                    prediction = model.forward_long(batch["text_tokens"], batch["input_kp"], **lengths)
                else:
                    lengths = padding_lengths(batch, ds.device) if mask_padding else {}
                    prediction = model(batch["text_tokens"], batch["input_kp"], **lengths)
                prediction = prediction.contiguous()
                if overlap:
                    loader.write_back_blend(prediction, plan, i, rows_out, before, blend, conf)
                    before = prediction[-1]
                else:
                    loader.write_back(prediction, u, s, k, rows_out, conf)
    finally:
        model.train(was_training)
    return ds.with_rows(rows_out)


@dataclass
class JointError:
    """joint_pixel_error's result.  utt_sum (U, 21) float32 and utt_count (U, 21) int32: per utterance and right-hand
    joint, the sum of the Euclidean pixel distances over the frames whose true confidence is > 0, and their number;
    total_sum / count (21): their float64 / int64 sums over the utterances; per_joint (21) float64 = total_sum / count,
    NaN where the count is 0; mean: over all counted joints."""
    utt_sum: np.ndarray
    utt_count: np.ndarray
    total_sum: np.ndarray
    count: np.ndarray
    per_joint: np.ndarray
    mean: float


def joint_pixel_error(pred_ds, true_ds):
    """Per-utterance, per-joint Euclidean pixel error of the right hands of `pred_ds` against `true_ds` (two
    DeviceDatasets with the same n_body, offsets and row count, e.g. predict_dataset's output and its input).  A frame
    counts for a joint iff `true_ds` holds a confidence > 0 for it.  Fixed summation orders and no atomics: the same
    bits on every run.  Returns a JointError."""
    if not isinstance(pred_ds, DeviceDataset) or not isinstance(true_ds, DeviceDataset):
        raise ValueError("joint_pixel_error() compares two DeviceDatasets")
    if pred_ds.n_body != true_ds.n_body or pred_ds.rows.shape != true_ds.rows.shape or pred_ds.device != true_ds.device:
        raise ValueError(f"the two stores must share n_body, the row count and the device: got n_body {pred_ds.n_body} / "
                         f"{true_ds.n_body}, rows {tuple(pred_ds.rows.shape)} / {tuple(true_ds.rows.shape)}")
    if pred_ds.offsets is not true_ds.offsets and not torch.equal(pred_ds.offsets, true_ds.offsets):
        raise ValueError("the two stores must share their offsets: compare a store with a prediction over the same store")
    dev, n_utt = true_ds.device, len(true_ds)
    utt_sum = torch.empty((n_utt, 21), dtype=torch.float32, device=dev)
    utt_count = torch.empty((n_utt, 21), dtype=torch.int32, device=dev)
    total_sum = torch.empty(21, dtype=torch.float64, device=dev)
    total_count = torch.empty(21, dtype=torch.int64, device=dev)
    with _lib.on_device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().b2h_joint_error(
            _ptr(pred_ds.rows), _ptr(true_ds.rows), true_ds.rows.shape[0], _ptr(true_ds.offsets), n_utt, true_ds.n_body,
            _ptr(utt_sum), _ptr(utt_count), _ptr(total_sum), _ptr(total_count), st))
    total, count = total_sum.cpu().numpy(), total_count.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        per_joint = np.where(count > 0, total / count, np.nan)
    n = int(count.sum())
    return JointError(utt_sum.cpu().numpy(), utt_count.cpu().numpy(), total, count, per_joint,
                      float(total.sum() / n) if n else float("nan"))
