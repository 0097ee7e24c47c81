"""Key-padding masks as key lengths: the lengths of padded token rows, and what the loops'
`mask_padding=True` hands to a TextPoseTransformer.

The reference pads every sentence to 40 ids with 0 and every utterance to `--max-frames` with zero rows, and calls
nn.Transformer without a mask.  Padding is always a suffix, so torch's three boolean key-padding masks are two lengths
per sequence: `text_lengths` (src_key_padding_mask and memory_key_padding_mask) and `frame_lengths`
(tgt_key_padding_mask).  `token_lengths` gives the first from the padded ids; the second is the loader's `n_frames`.
"""
import ctypes

import torch

from . import _lib
from .text_pose_transformer import TextPoseTransformer


def token_lengths(tokens, pad_id=0):
    """int64 (B,) on the tokens' device: 1 + the position of the last id that differs from `pad_id`, 1 for a row of
    pads only (a sequence attends to at least one key).  A `pad_id` inside the sentence counts as a token; id 0 is both
    the pad and `<unk>` in the reference's tokenizer, so a sentence that really ends in `<unk>` loses those tokens.
    tokens: int64 (B, S) on a GPU; one b2h_token_lengths launch on the current stream, capturable."""
    if not torch.is_tensor(tokens) or tokens.dim() != 2 or tokens.dtype != torch.int64:
        raise RuntimeError("expected int64 token ids of shape (B, S), got "
                           f"{tuple(tokens.shape) if torch.is_tensor(tokens) else type(tokens).__name__}"
                           f"{' ' + str(tokens.dtype) if torch.is_tensor(tokens) else ''}")
    if tokens.shape[1] < 1:
        raise RuntimeError("expected at least one token id per row (S >= 1)")
    if tokens.device.type != "cuda":
        raise RuntimeError("hand_pose_sl_amd.token_lengths runs on an MI355X only: call tokens.to('cuda') first (there is "
                           "no CPU path in the product)")
    tok = tokens.contiguous()
    out = torch.empty(tok.shape[0], dtype=torch.int64, device=tok.device)
    lib = _lib.load()
    with _lib.on_device(tok.device):
        st = torch.cuda.current_stream(tok.device).cuda_stream
        _lib.check(lib.b2h_token_lengths(ctypes.c_void_p(tok.data_ptr()), tok.shape[0], tok.shape[1], int(pad_id),
                                         ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(st)))
    return out


def check_mask_padding(what, model, mask_padding):
    """`mask_padding=True` is for the model that takes masks; returns bool(mask_padding)."""
    if mask_padding and not isinstance(model, TextPoseTransformer):
        raise ValueError(f"{what}: mask_padding=True hands key-padding masks to a TextPoseTransformer, the only model here "
                         f"that attends over padded text and frames; got a {type(model).__name__}")
    return bool(mask_padding)


def padding_lengths(batch, dev):
    """The two keywords of a masked TextPoseTransformer call for one batch: the token rows' lengths (one extra launch)
    and the loader's n_frames."""
    return {"text_lengths": token_lengths(batch["text_tokens"].to(device=dev, dtype=torch.int64)),
            "frame_lengths": batch["n_frames"]}
