"""The one host-side overlap checker of the training entry points (check_overlap in b2h_api.hip): b2h_backward and
b2h_tenc_backward refuse an output that aliases an input or a parameter with B2H_ERR_INVALID and their own message,
before anything is launched -- every output still holds its poison afterwards."""
import ctypes
import warnings

import pytest
import torch

import hand_pose_sl_amd as hps
from hand_pose_sl_amd import _lib

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
POISON = 12345.0


def _ptrs(ts):
    return (vp * len(ts))(*[t.data_ptr() for t in ts])


def _poisoned_like(ts):
    return [torch.full_like(t, POISON) for t in ts]


def _refused(lib, rc, message, outputs, dev):
    assert rc == _lib.ERR_INVALID
    assert lib.b2h_last_error().decode() == message
    torch.cuda.synchronize(dev)
    for t in outputs:
        assert bool((t == POISON).all())


def test_conv_backward_dx_aliasing_dy(cuda_device):
    B, T = 2, 17
    m = hps.ConvModel(8, "ReLU", False).to(cuda_device).train()
    lib, _ = m._ensure_created()
    params = [p.detach() for p in m._params()]
    x = torch.rand((B, T, 12, 2), device=cuda_device)
    dy = torch.full((B, T, 21, 2), POISON, device=cuda_device)
    grads = _poisoned_like(params)
    nbytes = lib.b2h_backward_workspace_bytes(m._handle, B, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda_device)
    torch.cuda.synchronize(cuda_device)
    rc = lib.b2h_backward(m._handle, _ptrs(params), vp(x.data_ptr()), vp(dy.data_ptr()), vp(dy.data_ptr()), _ptrs(grads),
                          B, T, vp(ws.data_ptr()), nbytes, None)
    _refused(lib, rc, "an output overlaps x or dy", grads + [dy], cuda_device)


def test_tenc_backward_gradient_aliasing_a_parameter(cuda_device):
    B, T, L = 2, 17, 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        m = hps.TransformerEnc(24, 4, 128, 42, L, dropout=0.0).to(cuda_device).train()
    lib, _ = m._ensure_created()
    tensors = [t.detach() for t in m._tensors()]            # pe, then the parameters
    before = tensors[4].clone()
    dy = torch.rand((B, T, 21, 2), device=cuda_device)
    grads = _poisoned_like(tensors[1:])
    dx = torch.full((B, T, 12, 2), POISON, device=cuda_device)
    nsaved, nws = lib.b2h_tenc_train_bytes(m._handle, B, T, 0), lib.b2h_tenc_train_bytes(m._handle, B, T, 1)
    saved = torch.zeros(nsaved, dtype=torch.uint8, device=cuda_device)
    scratch = torch.empty(nws, dtype=torch.uint8, device=cuda_device)
    aliased = list(grads)
    aliased[3] = tensors[4]                                  # the gradient of parameter 4 IS parameter 4
    torch.cuda.synchronize(cuda_device)
    rc = lib.b2h_tenc_backward(m._handle, _ptrs(tensors), None, 0.0, vp(dy.data_ptr()), vp(saved.data_ptr()), nsaved,
                               vp(dx.data_ptr()), _ptrs(aliased), vp(scratch.data_ptr()), nws, B, T, None)
    _refused(lib, rc, "an output overlaps a parameter", grads + [dx], cuda_device)
    assert torch.equal(tensors[4], before)
