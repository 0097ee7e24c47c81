"""The reference's evaluation loop around the three models (SURVEY.md 8f N4 + the callers of
the hot path): `validate(model, val_loader, criterion, device, args)`, body2hand/src/steps/traintest.py:168-213.

Per batch the reference computes  prediction = model(batch["body_kp"])  (traintest.py:183,194) or, for its
TextPoseTransformer,  model(batch["text_tokens"], batch["input_kp"])  (:193-195; batches of more than 128 frames
run through TextPoseTransformer.forward_long, the same forward on the long-attention path),
mask_output(prediction, n_frames)  (:203, steps/utils.py:309-312),  loss = criterion(prediction,
batch["target_kp"], n_frames[, batch["target_conf"]])  (:207-210)  and averages `loss.item()` over the
batches with AverageMeter (steps/utils.py:11-25).  Here the forward is the HIP model, the criterion one
of the two HIP reductions of `metrics.py`; the tail mask is skipped because neither criterion reads a
frame at or beyond `n_frames[i]` (it could not change the value).  One host synchronisation per call,
not per batch: the per-batch losses stay on the device until the end.

`train_epoch(model, train_loader, criterion, optimizer, args)` is the training counterpart, the loop body of
traintest.py:87-128 under the same dispatch and the same single synchronisation; with a `DeviceLoader` (dataset.py) as
the loader an epoch does no host work per batch.
"""
import torch

from .metrics import l1_to_pixels, masked_pose_l1, weighted_pose_l1
from .padding import check_mask_padding, padding_lengths
from .text_pose_transformer import TextPoseTransformer

LOSSES = ("L1", "confL1")  # the two `--loss` choices validate() can evaluate (traintest.py:207-210)


def _loss_name(criterion, args, loss):
    """Which of the reference's two evaluation losses is meant.  The reference's loop dispatches on
    `args.loss` (traintest.py:207-210), so that wins; then an explicit name; then the criterion's class."""
    if args is not None and getattr(args, "loss", None) is not None:
        return args.loss
    if loss is not None:
        return loss
    if isinstance(criterion, str):
        return criterion
    if criterion is None:
        return "L1"
    name = type(criterion).__name__
    return {"maskedPoseL1": "L1", "poderatedPoseL1": "confL1"}.get(name, name)


def _check_model_name(what, model, args):
    """traintest.py:93-109 / :183-200 dispatch on args.model; here the model's class does, and a name that is given
    must agree with it.  Returns whether the model is the text-conditioned one."""
    text = isinstance(model, TextPoseTransformer)
    name = getattr(args, "model", None) if args is not None else None
    if name is not None and (name == "TextPoseTransformer") != text or name not in (None, "Conv", "TransformerEnc",
                                                                                   "TextPoseTransformer"):
        raise ValueError(f"{what} runs Conv, TransformerEnc and TextPoseTransformer, each with a model of its "
                         f"class; got args.model={name!r} with a {type(model).__name__}")
    return text


def train_epoch(model, train_loader, criterion=None, optimizer=None, args=None, *, loss=None, mask_padding=False):
    """One epoch of the reference's training loop (steps/traintest.py:80,87-128) for its three models: per batch the
    forward -- model(batch["body_kp"]) or, for a TextPoseTransformer, model(batch["text_tokens"], batch["input_kp"]) --,
    the criterion, optimizer.zero_grad(), loss.backward(), optimizer.step().  `criterion`, `args.loss` and `args.model`
    are read exactly as validate() reads them; mask_output (:111) is skipped for validate()'s reason: neither criterion
    reads a frame at or beyond n_frames[i], so it changes neither the loss nor a gradient.  `train_loader`: a
    DeviceLoader, or any iterable of the reference's batch dicts.  Returns the mean of the batch losses as AverageMeter
    accumulates it (steps/utils.py:11-25: the sum of the `loss.item()` floats over their count), with one host
    synchronisation per epoch: the per-batch losses stay on the device until the end.

    mask_padding (not in the reference; TextPoseTransformer only, else ValueError): the model gets the key-padding
    masks of the batch, text_lengths = token_lengths(batch["text_tokens"]) (one more tiny launch per step) and
    frame_lengths = batch["n_frames"], so padded token ids and padded frames are not attended.  A model trained
    with masks must be validated and run with masks."""
    mask_padding = check_mask_padding("train_epoch()", model, mask_padding)
    loss = _loss_name(criterion, args, loss)
    if loss not in LOSSES:
        raise ValueError(f"train_epoch() trains with --loss L1 or confL1, not {loss!r}")
    if optimizer is None:
        raise ValueError("train_epoch() needs the optimizer")
    text = _check_model_name("train_epoch()", model, args)
    dev = next(model.parameters()).device
    model.train()
    losses = []
    for batch in train_loader:
        if text:   # traintest.py:105-107
            pose = batch["input_kp"] if "input_kp" in batch else batch["body_kp"]
            lengths = padding_lengths(batch, dev) if mask_padding else {}
            prediction = model(batch["text_tokens"].to(dev), pose.to(dev), **lengths)
        else:
            prediction = model(batch["body_kp"].to(dev))
        target = batch["target_kp"].to(dev)
        if loss == "L1":
            value = masked_pose_l1(prediction, target, batch["n_frames"])
        else:
            value = weighted_pose_l1(prediction, target, batch["n_frames"], batch["target_conf"])
        optimizer.zero_grad()
        value.backward()
        optimizer.step()
        losses.append(value.detach())
    if not losses:
        raise ZeroDivisionError("empty loader")  # AverageMeter.get_average() divides by its count
    values = torch.stack(losses).cpu().tolist()
    return sum(values) / len(values)


def validate(model, val_loader, criterion=None, device=None, args=None, *, loss=None, return_pixels=False,
             mask_padding=False):
    """`validate(model, val_loader, criterion, device, args)` exactly as steps/traintest.py:136,168 calls it
    -- `criterion` a maskedPoseL1 / poderatedPoseL1 instance (the reference's or `hand_pose_sl_amd`'s: only
    its class name is read, the HIP reduction of that name computes it), `device` ignored (the model's device
    is used; the reference moves the batch there itself), `args.loss` in {"L1", "confL1"} and, when present,
    `args.model` in {"Conv", "TransformerEnc", "TextPoseTransformer"} matching the model's class (anything else
    raises ValueError as traintest.py:199-200 does)
    -- or the short keyword form `validate(model, val_loader, loss="confL1")` / `validate(model, loader, "L1")`.

    model: hand_pose_sl_amd.ConvModel, TransformerEnc or TextPoseTransformer on a GPU; val_loader: iterable of
    batches (dicts with "body_kp" (B,T,12,2) -- for a TextPoseTransformer "text_tokens" (B,S) and "input_kp" or
    "body_kp" --, "target_kp" (B,T,21,2), "n_frames", and "target_conf" (B,T,21)
    for confL1), tensors on the host or the device as the reference's loader yields them.
    Returns the mean over batches of the batch losses (a float), like the reference; with
    return_pixels also L12Pixels(J, 1280) of it with J the prediction's joint count -- 21, or 4 / 12 for a model of
    `--predict right_index` / `right_3fingers` (traintest.py:21-28,139).  mask_padding: as for train_epoch()."""
    mask_padding = check_mask_padding("validate()", model, mask_padding)
    loss = _loss_name(criterion, args, loss)
    if loss not in LOSSES:
        # MSE / huber make the reference's validate() fail with an unbound `loss` (traintest.py:207-211)
        raise ValueError(f"validate() evaluates --loss L1 or confL1, not {loss!r}")
    text = _check_model_name("validate()", model, args)
    dev = next(model.parameters()).device
    model.eval()
    losses = []
    with torch.no_grad():
        for batch in val_loader:
            if text:   # traintest.py:193-195
                pose = batch["input_kp"] if "input_kp" in batch else batch["body_kp"]
                lengths = padding_lengths(batch, dev) if mask_padding else {}
                if pose.shape[1] > 128:   # model(tokens, pose) keeps its 128-frame limit: the long path, no transforms
                    prediction = model.forward_long(batch["text_tokens"], pose, **lengths)
                else:
                    prediction = model(batch["text_tokens"], pose, **lengths)
            else:
                prediction = model(batch["body_kp"])
            target = batch["target_kp"].to(dev)
            joints = prediction.shape[2]
            if loss == "L1":
                losses.append(masked_pose_l1(prediction, target, batch["n_frames"]))
            else:
                losses.append(weighted_pose_l1(prediction, target, batch["n_frames"], batch["target_conf"]))
    if not losses:
        raise ZeroDivisionError("empty loader")  # AverageMeter.get_average() divides by its count
    value = float(torch.stack(losses).double().mean())
    return (value, l1_to_pixels(value, joints)) if return_pixels else value
