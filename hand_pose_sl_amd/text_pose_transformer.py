"""Drop-in mirror of the reference's `TextPoseTransformer` (body2hand/src/models/HandPoseModels.py:181-230),
the text-conditioned body->hand model and the default of the reference's CLIs (run.py:32-36,148-151;
infer_utterance.py:27-28,102-103), on libb2h's gfx950 kernels.

Same constructor `TextPoseTransformer(n_tokens, n_joints, joints_dim, nhead, nhid, nout, n_enc_layers,
n_dec_layers, dropout=0.5)` and the same `state_dict`: the torch.nn containers are built in the reference's order,
so a seeded default init is identical and its checkpoints load as they are.  `model(input_tokens, input_pose)`
with int64 token ids (B, S) and float32 pose (B, T, 12, 2) -> float32 (B, T, 21, 2); tokenisation stays with the
caller, as in the reference (traintest.py:105-107).  The torch containers only hold parameters: the forward runs
through the C ABI (`b2h_tpt_forward`).  Like the reference, the model passes no mask (padded token id 0 is attended
like any other id) and never applies its two positional encodings, which exist only as `pe` buffers.

Inference only, exact fp32, S <= 128 and T <= 128.  No path ever falls back to PyTorch ops.
"""
import ctypes
import warnings

import torch
import torch.nn as nn

from . import _lib
from ._native import NativeModule
from .transformer_enc import PositionalEncoding


class TextPoseTransformer(NativeModule, nn.Module):
    """`precision` (not in the reference; keyword only): only "fp32" = fp32 operands on the matrix cores."""

    def __init__(self, n_tokens, n_joints, joints_dim, nhead, nhid, nout, n_enc_layers, n_dec_layers, dropout=0.5, *,
                 precision="fp32"):
        super().__init__()
        if precision != "fp32":
            raise ValueError(f"precision must be 'fp32', got {precision!r}")
        self.precision = precision
        self.model_type = "Transformer"
        self.src_mask = None
        self.token_pos_encoder = PositionalEncoding(nhid, dropout, max_len=40)
        self.pose_pos_encoder = PositionalEncoding(nhid, dropout, max_len=100)
        with warnings.catch_warnings():  # torch notes that seq-first layers skip its nested-tensor path
            warnings.simplefilter("ignore", UserWarning)
            self.transformer = nn.Transformer(nhid, nhead, n_enc_layers, n_dec_layers, nhid, dropout=dropout)
        self.token_embedding = nn.Embedding(n_tokens, nhid)
        self.hidden2pose_projection = nn.Linear(nhid, nout)
        self.pose2hidden_projection = nn.Linear(n_joints * joints_dim, nhid)
        self.n_tokens = int(n_tokens)
        self.ninp = int(n_joints * joints_dim)
        self._dropout_p = float(dropout)
        self._geom = (self.n_tokens, self.ninp, int(nhead), int(nhid), int(nout), int(n_enc_layers), int(n_dec_layers))

    _NAME, _CREATE, _LOAD, _DESTROY = "TextPoseTransformer", "b2h_tpt_create", "b2h_tpt_load_weights", "b2h_tpt_destroy"

    def _tensors(self):
        """The parameters in state_dict order, i.e. the order of b2h_tpt_load_weights (the two pe buffers, which the
        forward never uses, are not among them)."""
        return list(self.parameters())

    def _device(self):
        return self._modules["pose2hidden_projection"]._parameters["weight"].device

    def _create_args(self):
        return self._geom

    def _ensure_handle(self):
        """(library, device): this model's callers have always unpacked the pair."""
        return super()._ensure_handle(), self._device()

    def forward(self, input_tokens, input_pose):
        if self.training and self._dropout_p > 0.0:
            raise RuntimeError("hand_pose_sl_amd.TextPoseTransformer is inference-only: in training mode the reference "
                               f"applies dropout (p = {self._dropout_p}) and this path has none; call model.eval()")
        if input_pose.dim() != 4 or input_pose.shape[2] * input_pose.shape[3] != self.ninp:
            raise RuntimeError(f"expected input_pose of shape (B, T, {self.ninp // 2}, 2), got {tuple(input_pose.shape)}")
        if input_tokens.dim() != 2:
            raise RuntimeError(f"expected input_tokens of shape (B, S), got {tuple(input_tokens.shape)}")
        if input_tokens.shape[0] != input_pose.shape[0]:
            raise RuntimeError(f"input_tokens has batch size {input_tokens.shape[0]}, input_pose {input_pose.shape[0]}")
        if input_tokens.dtype not in (torch.int64, torch.int32):
            raise RuntimeError(f"expected integer token ids (int64, like nn.Embedding), got {input_tokens.dtype}")
        if input_tokens.device.type == "cpu" and input_tokens.numel():
            # where the ids are host memory the range check costs no synchronisation; ids already on the device
            # are checked by the kernel, which turns their sequence's output into NaN (include/b2h.h)
            lo, hi = int(input_tokens.min()), int(input_tokens.max())
            if lo < 0 or hi >= self.n_tokens:
                raise IndexError("index out of range in self")  # nn.Embedding's message
        lib, dev = self._ensure_handle()
        tok = input_tokens.to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
        x = input_pose.detach().to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
        B, S, T = tok.shape[0], tok.shape[1], x.shape[1]
        y = torch.empty((B, T, 21, 2), dtype=torch.float32, device=dev)
        need = lib.b2h_tpt_workspace_bytes(self._handle, B, S, T)
        ws = self._grown_workspace(need, dev)
        with _lib.on_device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.b2h_tpt_forward(self._handle, ctypes.c_void_p(tok.data_ptr()), ctypes.c_void_p(x.data_ptr()),
                                           ctypes.c_void_p(y.data_ptr()), B, S, T, ctypes.c_void_p(ws.data_ptr()),
                                           ws.numel(), ctypes.c_void_p(st)))
        return y
