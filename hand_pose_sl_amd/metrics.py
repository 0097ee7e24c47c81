"""Evaluation metrics of the reference on the GPU.

`masked_pose_l1` mirrors `maskedPoseL1.forward(prediction, target, lengths)`
(body2hand/src/steps/utils.py:413-428): per utterance the mean absolute error over its first
`lengths[i]` frames, averaged over the batch.  `weighted_pose_l1` mirrors `poderatedPoseL1`
(`--loss confL1`, steps/utils.py:431-452): the same with prediction and target multiplied by the
target joints' confidences, SUMMED over the batch (the class does not divide).  `l1_to_pixels`
mirrors `L12Pixels(4 | 12 | 21, 1280)` (steps/utils.py:291-299; the joint count follows `--predict`,
traintest.py:21-28), the "pixel distance" the training loop
prints (traintest.py:27-28,139).

Both losses are differentiable in the prediction (the training loop's `loss.backward()`,
traintest.py:111-121): when `prediction` requires a gradient and autograd is on, the same forward
kernels run inside an autograd Function whose backward is a HIP kernel.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._native import _aligned


def _l1(prediction, target, lengths, scores, return_per_sequence, what):
    if prediction.shape != target.shape or prediction.dim() != 4 or prediction.shape[2] < 1 or prediction.shape[3] != 2:
        raise RuntimeError("expected two (B, T, J, 2) tensors of one shape with J >= 1 joints (21 for the whole hand, 4 and "
                           f"12 for the finger targets), got {tuple(prediction.shape)} and {tuple(target.shape)}")
    if scores is not None and tuple(scores.shape) != tuple(prediction.shape[:3]):
        raise RuntimeError(f"scores must have shape {tuple(prediction.shape[:3])}, got {tuple(scores.shape)}")
    if prediction.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the GPU only")
    p = prediction.to(torch.float32).contiguous()
    t = target.to(device=p.device, dtype=torch.float32).contiguous()
    B, T = p.shape[0], p.shape[1]
    nf = None
    if lengths is not None:
        nf = torch.as_tensor(lengths).to(device=p.device, dtype=torch.int64).contiguous()
        if nf.shape != (B,):
            raise RuntimeError(f"lengths must have shape ({B},)")
    sc = None
    if scores is not None:
        sc = scores.to(device=p.device, dtype=torch.float32).contiguous()   # the reference moves them too (utils.py:439)
    if p.requires_grad and torch.is_grad_enabled():
        # the gradient kernels take pred and target on the 16-byte grid (the metric kernels read dwords)
        loss, per_seq = _L1Fn.apply(_aligned(p), _aligned(t.detach()), nf, None if sc is None else sc.detach())
    else:
        loss, per_seq = _l1_forward(p.detach(), t, nf, sc)
    return (loss, per_seq) if return_per_sequence else loss


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None


def _l1_forward(p, t, nf, sc):
    B, T, J = p.shape[0], p.shape[1], p.shape[2]
    per_seq = torch.empty((B,), dtype=torch.float32, device=p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    lib = _lib.load()
    with _lib.on_device(p.device):
        st = ctypes.c_void_p(torch.cuda.current_stream(p.device).cuda_stream)
        if sc is None:
            _lib.check(lib.b2h_masked_l1_joints(_ptr(p), _ptr(t), _ptr(nf), B, T, J, _ptr(per_seq), _ptr(loss), st))
        else:
            _lib.check(lib.b2h_weighted_l1_joints(_ptr(p), _ptr(t), _ptr(sc), _ptr(nf), B, T, J, _ptr(per_seq), _ptr(loss), st))
    return loss, per_seq


class _L1Fn(torch.autograd.Function):
    """The two L1 losses, differentiable in the prediction: the forward kernels above, and
    b2h_masked_l1_joints_backward / b2h_weighted_l1_joints_backward, which read dL/dloss from device memory (no host read).
    The per-sequence means are not differentiable."""

    @staticmethod
    def forward(ctx, p, t, nf, sc):
        loss, per_seq = _l1_forward(p, t, nf, sc)
        ctx.mark_non_differentiable(per_seq)
        ctx.save_for_backward(p, t, nf, sc)
        return loss, per_seq

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss, _gper):
        p, t, nf, sc = ctx.saved_tensors
        B, T, J = p.shape[0], p.shape[1], p.shape[2]
        g = (gloss if gloss is not None else torch.zeros((), device=p.device)).to(device=p.device, dtype=torch.float32).contiguous()
        dp = torch.empty_like(p)
        lib = _lib.load()
        with _lib.on_device(p.device):
            st = ctypes.c_void_p(torch.cuda.current_stream(p.device).cuda_stream)
            if sc is None:
                _lib.check(lib.b2h_masked_l1_joints_backward(_ptr(p), _ptr(t), _ptr(nf), B, T, J, _ptr(g), _ptr(dp), st))
            else:
                _lib.check(lib.b2h_weighted_l1_joints_backward(_ptr(p), _ptr(t), _ptr(sc), _ptr(nf), B, T, J, _ptr(g), _ptr(dp),
                                                               st))
        return dp, None, None, None


def masked_pose_l1(prediction, target, lengths=None, return_per_sequence=False):
    """prediction, target: (B, T, J, 2) float32 CUDA tensors, J >= 1 (21, or the 4 / 12 joints of the finger targets); lengths: (B,) ints or None (= T).
    Returns a 0-dim CUDA tensor (and the (B,) per-utterance means when asked)."""
    return _l1(prediction, target, lengths, None, return_per_sequence, "masked_pose_l1")


def weighted_pose_l1(prediction, target, lengths, scores, return_per_sequence=False):
    """poderatedPoseL1.forward(prediction, target, lengths, scores) (steps/utils.py:437-452): scores
    (B, T, J) = confidences of the target joints.  Returns the SUM over the batch of the per-utterance
    means, as the reference does."""
    if scores is None:
        raise RuntimeError("weighted_pose_l1 needs the (B, T, J) scores")
    return _l1(prediction, target, lengths, scores, return_per_sequence, "weighted_pose_l1")


def l1_to_pixels(loss, num_joints=21, upsample=1280):
    """L12Pixels (steps/utils.py:291-299): loss / num_joints * upsample."""
    return loss / num_joints * upsample


class maskedPoseL1(nn.Module):  # noqa: N801 -- the reference's class name (steps/utils.py:413-428)
    """`criterion = maskedPoseL1()` as traintest.py:36-38 builds it; `criterion(prediction, target, lengths)`
    runs the HIP reduction; differentiable in `prediction` when it requires a gradient (training)."""

    def forward(self, prediction, target, lengths):
        return masked_pose_l1(prediction, target, lengths)


class poderatedPoseL1(nn.Module):  # noqa: N801 -- the reference's class name (steps/utils.py:431-452)
    """`criterion = poderatedPoseL1()` (`--loss confL1`, traintest.py:39-40);
    `criterion(prediction, target, lengths, scores)`."""

    def forward(self, prediction, target, lengths, scores):
        return weighted_pose_l1(prediction, target, lengths, scores)
