"""Inference attention over described rows (b2h_attn_f32<NK>: one fp32 kernel for self- and cross-attention, block =
64 * query tiles, NK = key tiles) at the shapes where its tile masks and staging rounds can go wrong and that the
existing sweeps do not pin in this form.

TransformerEnc fp32 against the float64 port (oracle/tenc_torch_port.py): one layer, a positional table of 128 rows,
B = 3, T in {1, 15, 16, 17, 33, 100, 127, 128} -- a single row, one short of a tile, a whole tile, one past it, three
tiles with a one-row tail, the reference's length, eight tiles with a 15-row tail, eight whole tiles.  At Tq = Tk the
staging loop makes exactly one round.  The bound is TOL = 2e-5 of tests/test_transformer_enc.py, restated here.  That
file's test_hip_batch_independence_lengths_and_errors runs T = 1, 15, 16, 17, 33, 100 (B = 3) and
test_hip_lengths_up_to_128_with_a_longer_positional_table T = 100, 127, 128 (B = 5) on the four-layer model against the
numpy oracle; they stay, this file adds the float64 checker on one layer.

TextPoseTransformer fp32 at unequal tile counts, (S, T) in {(17, 16), (16, 17), (128, 1), (1, 128)}: one encoder and
one decoder layer, B = 2, against tpt_ref.Checker in float64 with tests/test_tpt_gpu.py's bound (tpt_ref.BAR); the
first sequence's output is bit-equal alone and inside the batch.  With more key tiles than query tiles the staging
loop makes several rounds ((128, 1): eight key tiles staged by one wave), with fewer some threads stage nothing
((1, 128)).  tests/test_tpt_gpu.py::test_shape_sweep has the equal counts (3, 16, 16), (2, 128, 128) and the unequal
(2, 1, 17), (2, 17, 33), (3, 33, 128), (3, 128, 15)."""
import functools

import pytest
import torch

import hand_pose_sl_amd as hps
import oracle
from tpt_ref import BAR, Checker, inputs, recipe_model

pytestmark = pytest.mark.gpu

TOL = 2e-5                      # tests/test_transformer_enc.py: the fp32 bound of TransformerEnc
TENC_T = [1, 15, 16, 17, 33, 100, 127, 128]
TPT_ST = [(17, 16), (16, 17), (128, 1), (1, 128)]


@functools.lru_cache(maxsize=None)
def tenc_pair():
    """(one-layer TransformerEnc with a 128-row positional table and non-default biases, its float64 port)."""
    torch.manual_seed(3)
    m = hps.TransformerEnc(24, 4, 128, 42, 1, precision="fp32")
    m.pos_encoder = hps.PositionalEncoding(24, 0.5, max_len=128)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p += 0.05 * torch.randn(p.shape, generator=g)
    state = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    return m.to("cuda:0").eval(), oracle.TencTorchPort(state, nlayers=1).double()


@pytest.mark.parametrize("T", TENC_T)
def test_tenc_fp32_against_the_float64_port(cuda_device, T):
    m, port = tenc_pair()
    x = torch.rand((3, T, 12, 2), generator=torch.Generator().manual_seed(100 + T)) - 0.5
    with torch.no_grad():
        y = m(x.to(cuda_device))
    err = float((y.cpu().double() - port(x.double())).abs().max())
    print(f"TransformerEnc fp32, 1 layer, (3, {T}): max|y - y64| = {err:.3e}")
    assert y.shape == (3, T, 21, 2) and err <= TOL


@functools.lru_cache(maxsize=None)
def tpt_pair():
    cpu = recipe_model(23, 100, 1, 1)
    return recipe_model(23, 100, 1, 1).to("cuda:0"), Checker(cpu, torch.float64)


@pytest.mark.parametrize("S,T", TPT_ST, ids=lambda v: str(v))
def test_tpt_fp32_unequal_tile_counts(cuda_device, S, T):
    m, check = tpt_pair()
    tok, pose = inputs(2, S, T, 100, 1000 * S + T)
    tok_d, pose_d = tok.to(cuda_device), pose.to(cuda_device)
    y = m(tok_d, pose_d)
    err = float((y.cpu().double() - check(tok, pose)).abs().max())
    print(f"TextPoseTransformer fp32, 1 + 1 layers, (2, {S}, {T}): max|y - y64| = {err:.3e}")
    assert y.shape == (2, T, 21, 2) and err <= BAR
    assert torch.equal(m(tok_d[:1], pose_d[:1])[0], y[0])   # alone == inside the batch
