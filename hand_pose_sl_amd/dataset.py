"""The training set on the GPU: `DeviceDataset` holds every frame of every utterance in device memory and
`DeviceLoader` turns "these utterances, these crop offsets" into the reference's batch dict with one HIP kernel
(b2h_build_batch, kernel_build_batch.h), so an epoch needs no host work per batch.

The reference builds a batch per utterance on the host -- FastTextPoseDataset.__getitem__ / TextPoseH5Dataset.__getitem__
(dataloaders/text_pose_dataset.py:430-476, 652-688: frame selection, padding, clipping, torch.tensor(list).float()),
WristDifference, ChestDifference, NormalizeFixedFactor and one Build*Item (steps/utils.py:180-277, run.py:83-104) --
under a DataLoader without workers (run.py:135-136), then copies it to the device (traintest.py:89-90,106).

Store layout (include/b2h.h): `rows` (N, 3 J) float32, J = n_body + 42, a row = [x * J | y * J | c * J] with the joints
n_body body, 21 left hand, 21 right hand; `offsets` (U + 1) int64 ascending; `tokens` (U, S) int64 or None.  n_body = 8
is the reference's HDF5 row (n_frames, 150); n_body = 12 the same rule for utterances read from OpenPose JSON.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, openpose

SELECTIONS = ("randomcrop", "first")
PADS = ("zeros", "frame0")
PLAN_SOURCES = ("torch", "native")
# (input joints, target joints) of each `--predict` choice (run.py:91-102), the input of right_hand being the body
_JOINTS = {"right_index": (29, 4), "right_3fingers": (21, 12)}


def frames_to_rows(frames):
    """One utterance's frames (OpenPose frame paths, parsed dicts or merged-JSON entries) -> its (n, 162) float32
    store rows: 12 body (BODY_HEAD_KEYPOINTS), 21 left-hand, 21 right-hand joints as [x * 54 | y * 54 | c * 54], the
    12-joint counterpart of openpose.item_to_h5_row.  Values are rounded to float32 as torch.tensor(list).float()
    rounds them (text_pose_dataset.py:536-544)."""
    out = np.empty((len(frames), 3, 54), np.float32)
    for i, fr in enumerate(frames):
        r_kp, r_conf, l_kp, l_conf, b_kp, b_conf = openpose.load_keypoints(fr)
        kp = np.asarray(b_kp + l_kp + r_kp, dtype=np.float64)
        if kp.shape != (54, 2):
            raise ValueError(f"frame {i}: expected 12 + 21 + 21 joints, got {kp.shape[0]}")
        out[i, 0], out[i, 1], out[i, 2] = kp[:, 0], kp[:, 1], np.asarray(b_conf + l_conf + r_conf, dtype=np.float64)
    return out.reshape(len(frames), 162)


class DeviceDataset:
    """`DeviceDataset(rows, offsets, n_body, tokens=None, device="cuda")`: validates the store once on the host and
    moves it to the GPU.  `len(ds)` is the number of utterances, `ds.lengths` their row counts (a host tensor)."""

    def __init__(self, rows, offsets, n_body, tokens=None, device="cuda"):
        if n_body not in (8, 12):
            raise ValueError(f"n_body must be 8 (HDF5 rows) or 12 (OpenPose JSON), got {n_body!r}")
        rows, offsets = torch.as_tensor(rows), torch.as_tensor(offsets)
        width = 3 * (n_body + 42)
        if rows.dtype != torch.float32 or offsets.dtype != torch.int64:
            raise ValueError(f"rows must be float32 and offsets int64, got {rows.dtype} and {offsets.dtype}")
        if rows.dim() != 2 or rows.shape[1] != width:
            raise ValueError(f"rows must be (N, {width}) for n_body = {n_body}, got {tuple(rows.shape)}")
        if offsets.dim() != 1 or offsets.numel() < 1:
            raise ValueError(f"offsets must be (U + 1,), got {tuple(offsets.shape)}")
        host = offsets.cpu()
        if int(host[0]) != 0 or int(host[-1]) != rows.shape[0] or bool((host[1:] < host[:-1]).any()):
            raise ValueError(f"offsets must ascend from 0 to the row count {rows.shape[0]}")
        n_utt = offsets.numel() - 1
        if tokens is not None:
            tokens = torch.as_tensor(tokens)
            if tokens.dtype != torch.int64:
                raise ValueError(f"tokens must be int64, got {tokens.dtype}")
            if tokens.dim() != 2 or tokens.shape[0] != n_utt or not 1 <= tokens.shape[1] <= 128:
                raise ValueError(f"tokens must be ({n_utt}, S) with 1 <= S <= 128, got {tuple(tokens.shape)}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceDataset lives on the GPU (an MI355X); there is no host fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_body = n_body
        self.rows = rows.to(self.device).contiguous()
        self.offsets = offsets.to(self.device).contiguous()
        self.tokens = None if tokens is None else tokens.to(self.device).contiguous()
        self.lengths = host[1:] - host[:-1]

    def __len__(self):
        return self.offsets.numel() - 1

    @classmethod
    def _from_utterances(cls, utterances, n_body, tokens, device):
        width = 3 * (n_body + 42)
        arrays = [np.ascontiguousarray(u, dtype=np.float32).reshape(-1, width) if np.size(u) else
                  np.zeros((0, width), np.float32) for u in utterances]
        offsets = np.zeros(len(arrays) + 1, np.int64)
        np.cumsum([a.shape[0] for a in arrays], out=offsets[1:])
        rows = np.concatenate(arrays, axis=0) if arrays else np.zeros((0, width), np.float32)
        return cls(torch.from_numpy(rows), torch.from_numpy(offsets), n_body, tokens, device)

    @classmethod
    def from_h5_rows(cls, utterances, tokens=None, device="cuda"):
        """A list of (n_i, 150) arrays, the datasets of the reference's keypoints HDF5 file (one per utterance)."""
        for i, u in enumerate(utterances):
            if np.ndim(u) != 2 or np.shape(u)[1] != 150:
                raise ValueError(f"utterance {i}: expected an (n_frames, 150) row array, got {np.shape(u)}")
        return cls._from_utterances(utterances, 8, tokens, device)

    @classmethod
    def from_frames(cls, utterances, tokens=None, device="cuda"):
        """A list of utterances, each a list of OpenPose frame dicts, merged-JSON entries or paths in time order."""
        return cls._from_utterances([frames_to_rows(list(u)) for u in utterances], 12, tokens, device)

    def with_rows(self, rows):
        """A store with this one's offsets, tokens and n_body (shared, not copied) around other `rows`: a contiguous
        float32 tensor of this store's shape on its device, taken as it is -- no copy, nothing validated again."""
        if (not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.shape != self.rows.shape or
                rows.device != self.device or not rows.is_contiguous()):
            raise ValueError(f"rows must be a contiguous float32 tensor of shape {tuple(self.rows.shape)} on {self.device}")
        other = object.__new__(type(self))
        other.__dict__.update(self.__dict__)
        other.rows = rows
        return other

    def utterance_rows(self):
        """The store as a list of (n_i, 3 J) float32 numpy arrays, one per utterance: the inverse of `from_h5_rows`
        (for n_body 8 the datasets of the reference's keypoints HDF5 file)."""
        rows, off = self.rows.cpu().numpy(), self.offsets.cpu().tolist()
        return [rows[off[u]:off[u + 1]].copy() for u in range(len(self))]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Augment:
    """`Augment(scale=0.0, rotate_deg=0.0, mirror=0.0, jitter=0.0)`: what `DeviceLoader(..., augment=)` draws per
    sequence and applies inside the batch build (b2h_build_batch_aug, kernel_build_batch_aug.h), a frozen value.

      scale       the sequence is scaled about its chest by a factor uniform in [1 - scale, 1 + scale]; 0 <= scale < 1
      rotate_deg  and rotated about it by an angle within +-rotate_deg degrees, 0 <= rotate_deg <= 90: tan(angle / 2) is
                  drawn uniformly, so `rotate_tan` = tan(radians(rotate_deg) / 2), computed in double and rounded once
      mirror      the probability of a left/right mirror (hands and body sides swapped), 0 <= mirror <= 1
      jitter      uniform noise of +-jitter pixels on every input joint, finite and >= 0

    The fields hold the float32 values the kernel receives.  A parameter of 0 switches its stage off; all four 0 build
    the plain batch, bit for bit."""
    __slots__ = ("scale", "rotate_deg", "mirror", "jitter", "rotate_tan")

    def __init__(self, scale=0.0, rotate_deg=0.0, mirror=0.0, jitter=0.0):
        given = {"scale": scale, "rotate_deg": rotate_deg, "mirror": mirror, "jitter": jitter}
        for name, v in given.items():
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        with np.errstate(over="ignore"):      # a value past float32's range becomes inf and is refused below
            f32 = {name: float(np.float32(v)) for name, v in given.items()}
        if not 0.0 <= f32["scale"] < 1.0:
            raise ValueError(f"scale must be in [0, 1), got {scale!r}")
        if not 0.0 <= float(rotate_deg) <= 90.0:
            raise ValueError(f"rotate_deg must be in [0, 90], got {rotate_deg!r}")
        if not 0.0 <= f32["mirror"] <= 1.0:
            raise ValueError(f"mirror must be a probability in [0, 1], got {mirror!r}")
        if not 0.0 <= f32["jitter"] < math.inf:
            raise ValueError(f"jitter must be finite and >= 0, got {jitter!r}")
        f32["rotate_deg"] = float(rotate_deg)
        f32["rotate_tan"] = float(np.float32(math.tan(math.radians(float(rotate_deg)) / 2.0)))
        for name, v in f32.items():
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value=None):
        raise AttributeError("Augment is frozen: make another one")

    __delattr__ = __setattr__

    def _fields(self):
        return (self.scale, self.rotate_tan, self.mirror, self.jitter)

    def __eq__(self, other):
        return isinstance(other, Augment) and self._fields() == other._fields()

    def __hash__(self):
        return hash(self._fields())

    def __repr__(self):
        return f"Augment(scale={self.scale!r}, rotate_deg={self.rotate_deg!r}, mirror={self.mirror!r}, jitter={self.jitter!r})"


class DeviceLoader:
    """Iterable over the batches of a DeviceDataset, `len()` of them, each the reference's batch dict on the device:
    "input_kp" (B, T, J_in, 2), "target_kp" (B, T, J_out, 2), "target_conf" (B, T, J_out), "n_frames" (B) int64,
    "text_tokens" (B, S) when the store has tokens, and for `right_hand` "body_kp", the same tensor as "input_kp".

    The order is sequential like run.py's loaders (`shuffle` draws a torch.randperm, with `generator` if given);
    "randomcrop" draws the crop starts with torch on the device, so they follow torch.manual_seed; "first" crops at 0.
    `pad`: "zeros" as TextPoseH5Dataset pads, "frame0" as the JSON datasets do.  `build(utt, start, out)` is the
    explicit form.

    `plan_epoch()` returns the order and the crop starts of a whole epoch as two device tensors, and
    `build_planned(plan, step_word, out)` builds the batch a device step word selects from them: the two halves of an
    epoch of captured steps (`GraphTrainer`).  `plan_source` "torch" (the default) draws the plan as `__iter__` draws,
    "native" with b2h_epoch_plan (kernel_epoch_plan.h) from (`seed`, epoch number) alone, and `__iter__` then iterates
    that plan too; torch's generators are not touched.

    `augment`: None (every call is the plain build's), or an `Augment`: `build`, `build_planned` and `__iter__` then go
    through b2h_build_batch_aug, keyed by two device words {seed, epoch} the loader owns.  The epoch word is the number
    of the epoch's plan -- for "native" the number b2h_epoch_plan receives, for "torch" a count kept the same way --,
    stored in place by `plan_epoch()` and `__iter__`; the draw index of a sequence is its position in the epoch
    (`build(..., entry0=)` names the first one of an explicit batch), so `train_epoch()` and `GraphTrainer.epoch()` see
    the same batches.

    `write_back(prediction, utt, start, skip, rows_out)` is the inverse of `build` for the target: a batch of
    predictions back into store rows (b2h_scatter_rows), what `predict_dataset` (predict.py) runs per slice;
    `write_back_blend` is the same for a plan of overlapping windows (b2h_scatter_rows_blend)."""

    def __init__(self, ds, batch_size, max_frames, selection="randomcrop", predict="right_hand", dif_encoding=True,
                 normalize=True, factor=1280, pad="zeros", shuffle=False, drop_last=False, generator=None,
                 plan_source="torch", seed=0, augment=None):
        if not isinstance(ds, DeviceDataset):
            raise TypeError("ds must be a DeviceDataset")
        if plan_source not in PLAN_SOURCES:
            raise ValueError(f"plan_source must be one of {PLAN_SOURCES}, got {plan_source!r}")
        if batch_size < 1 or max_frames < 1:
            raise ValueError("batch_size and max_frames must be >= 1")
        if selection not in SELECTIONS:
            raise ValueError(f"selection must be one of {SELECTIONS}, got {selection!r}")
        if pad not in PADS:
            raise ValueError(f"pad must be one of {PADS}, got {pad!r}")
        if predict not in _lib.PREDICT:
            raise ValueError(f"predict must be one of {sorted(_lib.PREDICT)}, got {predict!r}")
        if predict != "right_hand" and ds.n_body != 12:
            raise ValueError(f"--predict {predict} needs a 12-joint body (a store from OpenPose JSON)")
        if normalize and not factor > 0:
            raise ValueError("factor must be > 0")
        self.ds, self.batch_size, self.max_frames = ds, int(batch_size), int(max_frames)
        self.selection, self.predict, self.shuffle, self.drop_last, self.generator = selection, predict, shuffle, drop_last, generator
        self.plan_source, self.seed = plan_source, int(seed) & 0xFFFFFFFFFFFFFFFF
        self.epochs_planned = 0   # the epoch number of the next native plan (with `augment`: of the next plan)
        self._aug_key = None
        self.augment = augment
        self.factor = float(factor)
        self.flags =((_lib.BATCH_DIF_ENCODING if dif_encoding else 0) | (_lib.BATCH_NORMALIZE if normalize else 0) |
                      (_lib.BATCH_PAD_FRAME0 if pad == "frame0" else 0))
        self.joints = (ds.n_body, 21) if predict == "right_hand" else _JOINTS[predict]
        # the largest start a random crop may draw, per utterance (select_jsons: random.randint(0, len - n))
        self._room = (ds.lengths - self.max_frames).clamp_(min=0).to(ds.device)

    @property
    def augment(self):
        return self._augment

    @augment.setter
    def augment(self, augment):
        if augment is not None and not isinstance(augment, Augment):
            raise TypeError("augment must be None or a hand_pose_sl_amd.Augment")
        self._augment = augment
        if augment is None:
            return
        self._aug = _lib.AugmentStruct(augment.scale, augment.rotate_tan, augment.mirror, augment.jitter)
        if self._aug_key is None:     # {seed, epoch} as uint64 words; the epoch word is stored by _epoch_number
            signed = self.seed - (1 << 64) if self.seed >> 63 else self.seed
            self._aug_key = torch.tensor([signed, 0], dtype=torch.int64, device=self.ds.device)

    def __len__(self):
        n = len(self.ds)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _spec(self, B):
        """name -> (shape, dtype) of the tensors `build` writes for B sequences."""
        T, (ji, jt) = self.max_frames, self.joints
        spec = {"input_kp": ((B, T, ji, 2), torch.float32), "target_kp": ((B, T, jt, 2), torch.float32),
                "target_conf": ((B, T, jt), torch.float32), "n_frames": ((B,), torch.int64)}
        if self.ds.tokens is not None:
            spec["text_tokens"] = ((B, self.ds.tokens.shape[1]), torch.int64)
        return spec

    def empty_batch(self, B):
        """Unwritten tensors of one batch of B sequences: what `build` fills and returns."""
        out = {k: torch.empty(shape, dtype=dtype, device=self.ds.device) for k, (shape, dtype) in self._spec(B).items()}
        if self.predict == "right_hand":
            out["body_kp"] = out["input_kp"]
        return out

    def _epoch_number(self, epoch):
        """The number of the plan being made (None: the loader's own count, advanced), stored into the augmentation's
        epoch word in place."""
        if epoch is None:
            epoch, self.epochs_planned = self.epochs_planned, self.epochs_planned + 1
        epoch = int(epoch) & 0xFFFFFFFFFFFFFFFF
        if self.augment is not None:
            self._aug_key[1:].fill_(epoch - (1 << 64) if epoch >> 63 else epoch)
        return epoch

    def _launch(self, utt, start, n_plan, step_word, entry0, B, out):
        """One kernel: b2h_build_batch (no step word) or b2h_build_batch_planned, with `augment` b2h_build_batch_aug."""
        ds, dev, tok, lib = self.ds, self.ds.device, self.ds.tokens, _lib.load()
        store = (_ptr(ds.rows), ds.rows.shape[0], _ptr(ds.offsets), len(ds), ds.n_body, _ptr(tok),
                 0 if tok is None else tok.shape[1], _ptr(utt), _ptr(start))
        with _lib.on_device(dev):
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            batch = (B, self.max_frames, _lib.PREDICT[self.predict], self.flags, self.factor, _ptr(out["input_kp"]),
                     _ptr(out["target_kp"]), _ptr(out["target_conf"]),
                     _ptr(out.get("text_tokens")) if tok is not None else None, _ptr(out["n_frames"]), st)
            if self.augment is not None:
                rc = lib.b2h_build_batch_aug(*store, n_plan, _ptr(step_word), int(entry0), ctypes.byref(self._aug),
                                             _ptr(self._aug_key), *batch)
            elif step_word is None:
                rc = lib.b2h_build_batch(*store, *batch)
            else:
                rc = lib.b2h_build_batch_planned(*store, n_plan, _ptr(step_word), *batch)
            _lib.check(rc)
        return out

    def build(self, utt, start=None, out=None, entry0=0):
        """The batch of utterances `utt` ((B) int64 on the device; a list or host tensor is copied there) cropped at
        `start` ((B) int64, None = 0; read only for utterances longer than max_frames, clamped into them).  `out`: a
        batch returned earlier, written again in place -- with `utt` and `start` device tensors this launches one
        kernel and nothing else, so a captured graph replays it after the caller refreshes `utt` and `start` in place.
        `entry0` (read only with `augment`): the position in the epoch of the batch's first sequence, which keys its
        draws; `__iter__` passes i * batch_size for batch i."""
        ds, dev = self.ds, self.ds.device
        utt = torch.as_tensor(utt, dtype=torch.int64).to(dev).contiguous()
        if utt.dim() != 1:
            raise ValueError(f"utt must be (B,), got {tuple(utt.shape)}")
        B = utt.shape[0]
        if start is not None:
            start = torch.as_tensor(start, dtype=torch.int64).to(dev).contiguous()
            if start.shape != utt.shape:
                raise ValueError(f"start must be ({B},), got {tuple(start.shape)}")
        if out is None:
            out = self.empty_batch(B)
        for k, (shape, dtype) in self._spec(B).items():
            t = out.get(k)
            if t is None or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out[{k!r}] must be a contiguous {dtype} tensor of shape {shape} on {dev}")
        return self._launch(utt, start, 0, None, entry0, B, out)

    def write_back(self, prediction, utt, start, skip, rows_out, conf=1.0):
        """The inverse of `build` for the target: `prediction` ((B, max_frames, J_out, 2) float32 on the device, in the
        units of "target_kp") written into the store rows `rows_out` (a float32 tensor of the store's shape, normally a
        clone of `ds.rows`) with one kernel (b2h_scatter_rows): * factor and + the raw wrist as the loader's transforms
        ask, into the joints `predict` predicts, their confidences set to `conf`.  `utt`, `start` as `build` takes
        them; `skip` ((B) int64 or None = 0): the leading frames of each window that are left alone.  Frames at or past
        the utterance's end are never written.  Returns `rows_out`."""
        ds, dev = self.ds, self.ds.device
        utt = torch.as_tensor(utt, dtype=torch.int64).to(dev).contiguous()
        if utt.dim() != 1:
            raise ValueError(f"utt must be (B,), got {tuple(utt.shape)}")
        B = utt.shape[0]
        opt = {}
        for name, t in (("start", start), ("skip", skip)):
            if t is not None:
                t = torch.as_tensor(t, dtype=torch.int64).to(dev).contiguous()
                if t.shape != utt.shape:
                    raise ValueError(f"{name} must be ({B},), got {tuple(t.shape)}")
            opt[name] = t
        shape = (B, self.max_frames, self.joints[1], 2)
        for name, t, want in (("prediction", prediction, shape), ("rows_out", rows_out, tuple(ds.rows.shape))):
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != want or t.dtype != torch.float32 or t.device != dev or
                    not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float32 tensor of shape {want} on {dev}")
        with _lib.on_device(dev):
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_lib.load().b2h_scatter_rows(
                _ptr(ds.rows), ds.rows.shape[0], _ptr(ds.offsets), len(ds), ds.n_body, _ptr(utt), _ptr(opt["start"]),
                _ptr(opt["skip"]), B, self.max_frames, _lib.PREDICT[self.predict], self.flags, self.factor, _ptr(prediction),
                float(conf), _ptr(rows_out), st))
        return rows_out

    def write_back_blend(self, prediction, plan, entry0, rows_out, prediction_before=None, blend="linear", conf=1.0):
        """`write_back` for a plan of overlapping windows (`window_plan(..., overlap=K)`), one kernel
        (b2h_scatter_rows_blend).  `plan`: the WHOLE plan (utt, start, skip) as device int64 tensors (host tensors or
        lists are copied there); `prediction` ((B, max_frames, J_out, 2)) holds entries entry0 .. entry0 + B - 1 of
        it and `prediction_before` ((max_frames, J_out, 2), required when entry0 > 0) entry entry0 - 1, the last block
        of the batch before.  A window writes its used frames up to where the next window of the utterance begins
        its own, and the first K of them are blended with the window before: "linear" weights (p + 1) / (K + 1) for
        the later window, "centre" takes each frame from the window whose centre is nearer.  Every row is written by
        one call over the plan, so the calls may come in any order.  Returns `rows_out`."""
        ds, dev = self.ds, self.ds.device
        if blend not in _lib.BLEND:
            raise ValueError(f"blend must be one of {sorted(_lib.BLEND)}, got {blend!r}")
        if len(plan) != 3:
            raise ValueError("plan must be (utt, start, skip), as window_plan returns it")
        plan = [torch.as_tensor(t, dtype=torch.int64).to(dev).contiguous() for t in plan]
        if plan[0].dim() != 1 or any(t.shape != plan[0].shape for t in plan):
            raise ValueError(f"plan must be three (n_plan,) tensors, got {[tuple(t.shape) for t in plan]}")
        n_plan, entry0 = plan[0].shape[0], int(entry0)
        block = (self.max_frames, self.joints[1], 2)
        if not isinstance(prediction, torch.Tensor) or prediction.dim() != 4:
            raise ValueError(f"prediction must be a contiguous float32 tensor of shape (B, {', '.join(map(str, block))}) on {dev}")
        B = prediction.shape[0]
        if entry0 < 0 or entry0 + B > n_plan:
            raise ValueError(f"entries {entry0} .. {entry0 + B - 1} are not in a plan of {n_plan}")
        if entry0 > 0 and prediction_before is None:
            raise ValueError("prediction_before (the prediction of plan entry entry0 - 1) is needed when entry0 > 0")
        for name, t, want in (("prediction", prediction, (B,) + block), ("prediction_before", prediction_before, block),
                              ("rows_out", rows_out, tuple(ds.rows.shape))):
            if t is None and name == "prediction_before":
                continue
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != want or t.dtype != torch.float32 or t.device != dev or
                    not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float32 tensor of shape {want} on {dev}")
        with _lib.on_device(dev):
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_lib.load().b2h_scatter_rows_blend(
                _ptr(ds.rows), ds.rows.shape[0], _ptr(ds.offsets), len(ds), ds.n_body, *[_ptr(t) for t in plan], n_plan,
                entry0, B, self.max_frames, _lib.PREDICT[self.predict], self.flags, self.factor, _ptr(prediction),
                _ptr(prediction_before), _lib.BLEND[blend], float(conf), _ptr(rows_out), st))
        return rows_out

    def draw_starts(self, utt):
        """Random crop offsets for the utterances `utt` (device int64): uniform in [0, len - max_frames], 0 for an
        utterance that fits; drawn on the device from torch's generator, without a host synchronisation."""
        room = self._room[utt]
        u = torch.rand(room.shape, dtype=torch.float64, device=room.device)
        return torch.minimum((u * (room + 1).to(torch.float64)).to(torch.int64), room)

    def plan_epoch(self, epoch=None):
        """(utt_plan, start_plan) of one epoch: device int64 tensors of len(ds) entries, the utterance and the crop
        start of every sequence in the order the batches take them; start_plan is None unless the selection is
        "randomcrop".  "torch": exactly what `__iter__` draws, in its order -- the randperm, then `draw_starts` batch
        by batch (the entries of a dropped last batch start at 0, undrawn) --, so from one generator state an eager
        epoch and a planned one see the same batches.  "native": one b2h_epoch_plan launch keyed by (seed, epoch);
        `epoch` None takes the loader's own count and advances it.  With `augment` both sources store that number into
        the augmentation's epoch word."""
        n, dev, B = len(self.ds), self.ds.device, self.batch_size
        crop = self.selection == "randomcrop"
        if self.plan_source == "native":
            epoch = self._epoch_number(epoch)
            utt = torch.empty(n, dtype=torch.int64, device=dev)
            start = torch.empty(n, dtype=torch.int64, device=dev) if crop else None
            with _lib.on_device(dev):
                st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                _lib.check(_lib.load().b2h_epoch_plan(_ptr(self.ds.offsets), n, self.max_frames, int(bool(self.shuffle)),
                                                      int(crop), self.seed, epoch, _ptr(utt), _ptr(start), st))
            return utt, start
        if self.augment is not None:
            self._epoch_number(epoch)
        order = (torch.randperm(n, generator=self.generator).to(dev) if self.shuffle else
                 torch.arange(n, dtype=torch.int64, device=dev))
        if not crop:
            return order, None
        drawn = [self.draw_starts(order[i * B:(i + 1) * B]) for i in range(len(self))]
        drawn.append(torch.zeros(n - sum(d.shape[0] for d in drawn), dtype=torch.int64, device=dev))
        return order, torch.cat(drawn)

    def build_planned(self, plan, step_word, out):
        """The planned counterpart of `build`: the batch of `out`'s B sequences, entries *step_word * B .. + B - 1 of
        `plan` = (utt_plan, start_plan or None) (b2h_build_batch_planned); `step_word` is a one-element int64 tensor on
        the device.  One kernel launch and nothing else, so a captured graph replays it with whatever the step word
        holds by then; entries past the plan's end come out as unknown utterances (NaN, -1, 0).  Returns `out`."""
        ds, dev = self.ds, self.ds.device
        utt, start = plan
        for name, t in (("utt_plan", utt), ("step_word", step_word)) + ((("start_plan", start),) if start is not None else ()):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.device != dev or t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous 1-d int64 tensor on {dev}")
        if start is not None and start.shape != utt.shape:
            raise ValueError(f"start_plan must be ({utt.shape[0]},), got {tuple(start.shape)}")
        if step_word.numel() != 1:
            raise ValueError("step_word must hold one element")
        nf = out.get("n_frames") if isinstance(out, dict) else None
        if nf is None or nf.dim() != 1:
            raise ValueError("out must be a batch from empty_batch() or build()")
        B = nf.shape[0]
        for k, (shape, dtype) in self._spec(B).items():
            t = out.get(k)
            if t is None or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out[{k!r}] must be a contiguous {dtype} tensor of shape {shape} on {dev}")
        return self._launch(utt, start, utt.shape[0], step_word, 0, B, out)

    def __iter__(self):
        if self.plan_source == "native":
            utt, start = self.plan_epoch()
            for i in range(len(self)):
                sl = slice(i * self.batch_size, (i + 1) * self.batch_size)
                yield self.build(utt[sl], None if start is None else start[sl], entry0=i * self.batch_size)
            return
        n, dev = len(self.ds), self.ds.device
        if self.augment is not None:
            self._epoch_number(None)
        order =(torch.randperm(n, generator=self.generator).to(dev) if self.shuffle else
                 torch.arange(n, dtype=torch.int64, device=dev))
        for i in range(len(self)):
            utt = order[i * self.batch_size:(i + 1) * self.batch_size]
            yield self.build(utt, self.draw_starts(utt) if self.selection == "randomcrop" else None, entry0=i * self.batch_size)
