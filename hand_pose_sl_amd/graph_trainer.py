"""`GraphTrainer`: `train_epoch()` with the step captured into a HIP graph.

    trainer = hand_pose_sl_amd.GraphTrainer(model, loader, optimizer, criterion)
    for epoch in range(args.epochs):
        adjust_learning_rate(args.lr, args.lr_decay, optimizer, epoch)     # steps/utils.py:301-307, as the reference does
        train_loss = trainer.epoch()

One step is  build the batch -> forward -> loss -> backward -> Adam -> record  (the loop body of steps/traintest.py:87-128).
Everything a step reads that changes from step to step lives in device words: the plan entry it builds from (the epoch's
plan of `DeviceLoader.plan_epoch` and a step word, b2h_build_batch_planned), the dropout masks' counter
(`set_dropout_source("native")`), Adam's step count and learning rate (`hand_pose_sl_amd.Adam`).  b2h_epoch_record ends
the step: it stores the loss into the epoch's loss array and advances the step word.  So the first step ever runs eagerly
(the warm-up that allocates the optimizer state, and a real step), the step is then captured once on one stream without
parallel branches, and every later full step of this and of every later epoch is a `graph.replay()` with no host work in
between.  A final partial batch runs eagerly through the ordinary `build` on the plan's tail.  One device-to-host copy
per epoch, of the losses.

The graph is captured again (after one more eager step) when something baked into it changes: the models' train-kernel,
train-linear and dropout switches, Adam's betas, eps, weight_decay and its four step-control options (max_grad_norm,
skip_nonfinite, warmup_steps, schedule; the warmup's progress is the step word and is not), the batch geometry or the store, the
loader's `Augment` fields or its key words' storage (the epoch word's value is not: `plan_epoch()` rewrites it in place), or the
storage of a parameter, or `mask_padding`.  The learning rate is not baked in: `epoch()` calls `optimizer.sync_hyper()`.

`mask_padding=True` (TextPoseTransformer only) is train_epoch()'s: the step hands the model the batch's key-padding masks.
The b2h_token_lengths launch that makes text_lengths is part of the captured step and reads the capture's own batch
buffers, as the forward reads n_frames from them.
"""
import ctypes

import torch

from . import _lib
from .dataset import DeviceLoader
from .evaluate import LOSSES, _loss_name
from .metrics import masked_pose_l1, weighted_pose_l1
from .optim import Adam
from .padding import check_mask_padding, padding_lengths
from .text_pose_transformer import TextPoseTransformer


def _dropout_p(model):
    """The dropout probability of a training forward: TextPoseTransformer's, TransformerEnc's; ConvModel has none."""
    if hasattr(model, "_dropout_p"):
        return float(model._dropout_p)
    enc = getattr(model, "pos_encoder", None)
    return float(enc.dropout.p) if enc is not None else 0.0


class GraphTrainer:
    """`epoch() -> float` does what `train_epoch(model, loader, criterion, optimizer)` does, for ConvModel,
    TransformerEnc and TextPoseTransformer, and returns the same AverageMeter mean of the batch losses.  `captures`
    and `replays` count the graph captures and replays made so far.  Refuses at construction, before any GPU work,
    what a captured step cannot contain; each message names the remedy."""

    def __init__(self, model, loader, optimizer, criterion=None, *, loss=None, mask_padding=False):
        self.mask_padding = check_mask_padding("GraphTrainer", model, mask_padding)
        if not isinstance(loader, DeviceLoader):
            raise ValueError("GraphTrainer replays steps that build their batch on the device: put the training set into a "
                             "hand_pose_sl_amd.DeviceDataset and pass a hand_pose_sl_amd.DeviceLoader over it (or use "
                             "train_epoch() with this loader)")
        if not isinstance(optimizer, Adam):
            raise ValueError("GraphTrainer captures optimizer.step(): use hand_pose_sl_amd.Adam, whose step count and "
                             f"learning rate are device words, not {type(optimizer).__name__} (or use train_epoch())")
        p = _dropout_p(model)
        if p > 0.0 and getattr(model, "dropout_source", "torch") == "torch":
            raise ValueError(f"GraphTrainer cannot capture torch-drawn dropout masks (dropout = {p}): call "
                             "model.set_dropout_source(\"native\", seed) first (or use train_epoch())")
        name = _loss_name(criterion, None, loss)
        if name not in LOSSES:
            raise ValueError(f"GraphTrainer trains with --loss L1 or confL1, not {name!r}: pass a maskedPoseL1 or "
                             "poderatedPoseL1 criterion, or loss=\"L1\" / \"confL1\"")
        text = isinstance(model, TextPoseTransformer)
        if text and loader.ds.tokens is None:
            raise ValueError("a TextPoseTransformer trains on text: give the DeviceDataset its tokens")
        if not text and loader.predict != "right_hand":
            raise ValueError(f"{type(model).__name__} reads batch[\"body_kp\"]: use a DeviceLoader with predict=\"right_hand\"")
        self.model, self.loader, self.optimizer, self.loss = model, loader, optimizer, name
        self._text = text
        self.captures = self.replays = 0
        self._key = None       # what the graph and its buffers were made for
        self._graph = None
        self._warm = False     # an eager step ran under _key
        self._keep = None      # the captured step's loss tensor

    # ---- what a capture bakes in -----------------------------------------------------------------------------------
    def _graph_key(self):
        m, ld, ds = self.model, self.loader, self.loader.ds
        g = self.optimizer.param_groups[0]
        drop = m.__dict__.get("_drop_step")
        return (getattr(m, "train_kernels", None), getattr(m, "train_linear", None), getattr(m, "train_whole", None),
                getattr(m, "dropout_source", None), bool(self.mask_padding),
                getattr(m, "_drop_seed", None), _dropout_p(m), None if drop is None else drop.data_ptr(),
                float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                self.optimizer.max_grad_norm, self.optimizer.skip_nonfinite, self.optimizer.warmup_steps, self.optimizer.schedule,
                ld.batch_size, ld.max_frames, ld.predict, ld.flags, ld.factor, ld.drop_last, ld.selection, len(ds), ds.n_body,
                ds.rows.data_ptr(), ds.offsets.data_ptr(), None if ds.tokens is None else ds.tokens.data_ptr(),
                None if ld.augment is None else ld.augment._fields() + (ld._aug_key.data_ptr(),),
                tuple(p.data_ptr() for grp in self.optimizer.param_groups for p in grp["params"]))

    def _reset(self, key):
        ld, dev, n = self.loader, self.loader.ds.device, len(self.loader.ds)
        self._graph = self._keep = None
        self._warm = False
        self._key = key
        self._batch = ld.empty_batch(ld.batch_size)
        self._utt_plan = torch.empty(n, dtype=torch.int64, device=dev)
        self._start_plan = torch.empty(n, dtype=torch.int64, device=dev) if ld.selection == "randomcrop" else None
        self._step_word = torch.zeros(1, dtype=torch.int64, device=dev)
        self._losses = torch.empty(-(-n // ld.batch_size), dtype=torch.float32, device=dev)

    # ---- one step --------------------------------------------------------------------------------------------------
    def _train_on(self, batch):
        """forward, loss, backward, Adam and the record of one batch, in train_epoch()'s order; returns the loss."""
        m, opt, dev = self.model, self.optimizer, self.loader.ds.device
        if self._text:
            lengths = padding_lengths(batch, dev) if self.mask_padding else {}
            prediction = m(batch["text_tokens"], batch["input_kp"], **lengths)
        else:
            prediction = m(batch["body_kp"])
        if self.loss == "L1":
            value = masked_pose_l1(prediction, batch["target_kp"], batch["n_frames"])
        else:
            value = weighted_pose_l1(prediction, batch["target_kp"], batch["n_frames"], batch["target_conf"])
        opt.zero_grad()
        value.backward()
        opt.step()
        value = value.detach()
        with _lib.on_device(dev):
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_lib.load().b2h_epoch_record(ctypes.c_void_p(value.data_ptr()), ctypes.c_void_p(self._losses.data_ptr()),
                                                    self._losses.numel(), ctypes.c_void_p(self._step_word.data_ptr()), st))
        return value

    def _planned_step(self):
        plan = (self._utt_plan, self._start_plan)
        return self._train_on(self.loader.build_planned(plan, self._step_word, self._batch))

    def _capture(self):
        graph = torch.cuda.CUDAGraph()
        self.optimizer.zero_grad(set_to_none=True)      # the captured backward allocates the gradients in the graph's pool
        with torch.cuda.graph(graph):                   # one stream: no parallel branches; nothing runs
            self._keep = self._planned_step()
        self._graph = graph
        self.captures += 1

    # ---- the epoch -------------------------------------------------------------------------------------------------
    def epoch(self):
        ld, opt = self.loader, self.optimizer
        n, B = len(ld.ds), ld.batch_size
        full = n // B
        tail = 0 if ld.drop_last else n - full * B
        count = full + (1 if tail else 0)
        if count == 0:
            raise ZeroDivisionError("empty loader")  # AverageMeter.get_average() divides by its count
        self.model.train()
        if getattr(self.model, "dropout_source", None) == "native":
            self.model._drop_step_on(self.model._device())   # the word a captured draw reads exists before it is keyed
        key = self._graph_key()
        if key != self._key:
            self._reset(key)
        utt, start = ld.plan_epoch()
        self._utt_plan.copy_(utt)
        if self._start_plan is not None:
            self._start_plan.copy_(start)
        self._step_word.zero_()
        opt.sync_hyper()
        for _ in range(full):
            if self._graph is None and not self._warm:
                self._planned_step()
                self._warm = True
                continue
            if self._graph is None:
                self._capture()
            self._graph.replay()
            self.replays += 1
        if tail:
            sl = slice(full * B, n)
            self._train_on(ld.build(self._utt_plan[sl], None if self._start_plan is None else self._start_plan[sl],
                                    entry0=full * B))
        values = self._losses[:count].cpu().tolist()
        if full:   # replays wrote through raw pointers: tell autograd and the models' packed-weights key
            torch.autograd.graph.increment_version([p for grp in opt.param_groups for p in grp["params"]])
        return sum(values) / len(values)
