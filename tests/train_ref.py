"""Helpers of the training tests (tests/test_train_*.py): the fixtures under tests/golden/train/, float64 /
float32 autograd through the oracle's torch port, and the gradient accuracy bar.  A helper module, not a
conftest.py: the tests import it by name.

The bar (per tensor): max|g - g64| <= 4 * max|g32_ref - g64| + 1e-6 * max|g64|, i.e. as accurate as the
reference's own fp32 training, with a floor for tensors whose fp32 error happens to be ~0."""
import glob
import os

import numpy as np
import torch

from conftest import GOLDEN

KEYS = ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias",
        "conv4.weight", "conv4.bias"]
TRAIN = os.path.join(GOLDEN, "train")


def train_cases(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(TRAIN, prefix + "*.npz")))


def load_train(name):
    d = np.load(os.path.join(TRAIN, name + ".npz"))
    rec = {k: d[k] for k in d.files}
    B, T, C, pe, seed = [int(v) for v in rec["meta"]]
    rec.update(B=B, T=T, C=C, pos_emb=bool(pe), seed=seed)
    rec["state"] = {k: rec[k.replace(".", "_")] for k in KEYS}
    return rec


def bar(err32, g64):
    return 4.0 * float(err32) + 1e-6 * float(np.abs(g64).max())


def assert_within_bar(got, g64, err32, what):
    got = np.asarray(got, np.float64)
    err = float(np.abs(got - g64).max()) if g64.size else 0.0
    lim = bar(err32, g64)
    assert np.isfinite(got).all() and err <= lim, f"{what}: max|g - g64| = {err:.3e} > bar {lim:.3e}"


def port_grads(x, state, dy, pos_emb, dtype):
    """Parameter gradients and dx of sum(y * dy), y = torch_port.torch_forward, in `dtype` on the CPU."""
    from oracle.torch_port import torch_forward
    st = {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    xx = torch.as_tensor(x).detach().to(dtype).clone().requires_grad_(True)
    if pos_emb and dtype != torch.float32:   # the port builds its t/100 channel in float32
        y = _port64(xx, st)
    else:
        y = torch_forward(xx, st, pos_emb)
    (y * torch.as_tensor(dy).to(dtype)).sum().backward()
    return y.detach(), [st[k].grad for k in KEYS], xx.grad


def _port64(x, st):
    import torch.nn.functional as F
    B, T = x.shape[0], x.shape[1]
    h = x.reshape(B, T, 24).transpose(1, 2)
    pe = (torch.arange(100, dtype=torch.float32) / 100).to(x.dtype).view(1, 1, 100).expand(B, 1, 100)
    h = torch.cat([pe, h], dim=1)
    for i in (1, 2, 3):
        h = F.relu(F.conv1d(h, st[f"conv{i}.weight"], st[f"conv{i}.bias"], padding=2))
    h = F.conv1d(h, st["conv4.weight"], st["conv4.bias"], padding=2)
    return h.view(B, 21, 2, T).permute(0, 3, 1, 2)


def reference_loss(pred, target, lengths, scores, kind):
    """maskedPoseL1 / poderatedPoseL1 restated with torch ops (steps/utils.py:413-452), after mask_output
    (utils.py:309-312) applied in place."""
    for i, n in enumerate(lengths):
        pred[i, int(n):] = 0
    loss = 0
    for i, n in enumerate(lengths):
        p, t = pred[i, :int(n)], target[i, :int(n)]
        if kind == "L1":
            loss = loss + torch.nn.functional.l1_loss(p, t)
        else:
            s = scores[i, :int(n)].unsqueeze(2)
            loss = loss + torch.nn.functional.l1_loss(p * s, t * s)
    return loss / len(lengths) if kind == "L1" else loss
