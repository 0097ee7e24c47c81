"""The persistent bf16/f16 kernel (kernel_mfma16.h) where its layer 1 and its tile loop can go wrong: layer 1 reads
the unpadded [time][24] image under weight fragments whose last eight k-slots are zero (so every byte under them
must be finite, stale LDS included), and the tile loops are peeled so that no fragment is read past the last tile
(tails of 0 to 3 tiles after the two-tile loop body).  Bounds are the ones tests/test_gpu_parity.py holds the same
kernels to, imported from there."""
import numpy as np
import pytest
import torch

import oracle
from conftest import golden_names, load_golden
from poison import POISON
from test_gpu_parity import ORACLE_MODE, TOL, TOL_MODEL, _model, _poisoned, _tol

pytestmark = pytest.mark.gpu

PRECS = ["bf16", "f16"]
LENGTHS = sorted({1, 2, 3, 5, 8, 15, 16, 17, 31, 32, 33, 95, 96, 97, 191, 192, 193, 200, 207, 208, 209, 385, 600,
                  63, 64, 65})   # (63..65: four tiles against five, the first length at which the loop body runs twice)


def _all_written(y):
    return not bool((y.view(torch.int32) == torch.tensor(POISON, dtype=torch.int32)).any())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("T", LENGTHS)
def test_lengths_into_poisoned_output(T, prec, cuda_device):
    """Lengths around the tile, the loop's tails and the chunk edges, B = 3, U[-.5,.5], into a poisoned buffer:
    every row written, and the oracle's bars."""
    rec = load_golden("cfg1_b1_t200")
    g = torch.Generator().manual_seed(1000 + T)
    x = torch.rand((3, T, 12, 2), generator=g) - 0.5
    m = _model(rec, prec, cuda_device)
    out = _poisoned(torch.empty((3, T, 21, 2), device=cuda_device))
    with torch.no_grad():
        y = m.forward_into(x.to(cuda_device), out)
    assert _all_written(y), (prec, T)
    y = y.cpu().numpy()
    err = np.abs(y - oracle.forward_from_state(x.numpy(), rec["state"])).max()
    errm = np.abs(y - oracle.forward_from_state(x.numpy(), rec["state"], mode=ORACLE_MODE[prec])).max()
    print(f"T={T} {prec}: vs fp32 {err:.3e} (bar {TOL[prec]:.1e}), vs operand model {errm:.3e} (bar {TOL_MODEL[prec]:.1e})")
    assert err <= TOL[prec]
    assert errm <= TOL_MODEL[prec]


def _poisoned_rows(pattern, B, g):
    """Which of B sequences are poisoned.  A static launch of B whole-sequence chunks on G = min(CUs, B) workgroups
    gives workgroup b the chunks b + G k, which its waves draw in order.  "odd": every odd sequence -- with an even G
    a workgroup then sees one parity only, so this pattern alone checks batch independence, not stale LDS.
    "random": a seeded random half, which mixes clean and poisoned chunks in every workgroup's list and so in
    every wave's LDS area, whatever G is."""
    if pattern == "odd":
        return torch.arange(B) % 2 == 1
    return torch.rand(B, generator=g) < 0.5


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pattern", ["odd", "random"])
@pytest.mark.parametrize("T", [5, 40, 200])
def test_poisoned_neighbours(T, pattern, prec, cuda_device):
    """8 192 sequences in a static launch (32 chunks per workgroup, four per wave, computed in turn in the wave's
    one LDS area), some of them all NaN and +-Inf: a clean sequence that came out differently from a launch of
    the clean ones alone has read a neighbour's row -- under a zero weight (0 x NaN) or past its own last tile."""
    rec = load_golden("cfg1_b1_t200")
    B = 8192
    g = torch.Generator().manual_seed(T)
    x = torch.rand((B, T, 12, 2), generator=g) - 0.5
    bad = _poisoned_rows(pattern, B, g)
    n_bad = int(bad.sum())
    assert 0 < n_bad < B
    x[bad] = torch.tensor([float("nan"), float("inf"), float("-inf")])[torch.randint(0, 3, (n_bad, T, 12, 2), generator=g)]
    if pattern == "random":   # the mixing the pattern is for: clean and poisoned chunks in one workgroup's list
        ncu = torch.cuda.get_device_properties(cuda_device).multi_processor_count
        mine = bad[0::min(ncu, B)]
        assert bool(mine.any()) and not bool(mine.all())
    x = x.to(cuda_device)
    clean = (~bad).to(cuda_device)
    m = _model(rec, prec, cuda_device)
    with torch.no_grad():
        y = m(x)
        alone = m(x[clean].contiguous())
    assert bool(torch.isfinite(alone).all())
    assert torch.equal(y[clean], alone), (prec, pattern, T)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("T", [3, 17, 81])
def test_pool_launch_equals_static_pieces(T, prec, cuda_device):
    """65 536 short sequences = 256 chunks per workgroup, the smallest DYNAMIC launch, against the same rows in
    static-sized pieces, bit for bit; a second pool launch then fills a poisoned buffer."""
    rec = load_golden("cfg2_b64_t200_u55")
    B = 65536
    g = torch.Generator(device=cuda_device).manual_seed(7 * T)
    x = torch.rand((B, T, 12, 2), generator=g, device=cuda_device) - 0.5
    m = _model(rec, prec, cuda_device)
    with torch.no_grad():
        y = m(x)
        pieces = torch.cat([m(x[a:a + 4096]) for a in range(0, B, 4096)])
        assert torch.equal(y, pieces), (prec, T)
        again = m.forward_into(x, _poisoned(y))
        assert _all_written(again) and torch.equal(again, y), (prec, T)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("T", [33, 200])
def test_all_fused_flags_equal_transform_launch_transform(T, prec, cuda_device):
    """Chest difference, normalise, de-normalise and the tail mask in one fused launch == the same IEEE fp32
    transforms around a plain launch, bit for bit."""
    rec = load_golden("cfg1_b1_t200")
    B, factor = 5, np.float32(1280.0)
    rng = np.random.default_rng(T)
    body = rng.random((B, T, 12, 2), dtype=np.float32) * np.array([1280.0, 720.0], np.float32)
    nf = np.array([T, 1, T // 2, T - 1, 17])
    m = _model(rec, prec, cuda_device)
    with torch.no_grad():
        fused = m.forward_fused(torch.from_numpy(body).to(cuda_device), n_frames=nf, dif_encoding=True, normalize=True,
                                denormalize=True, mask_tail=True, factor=float(factor)).cpu().numpy()
        inp = (body - body[:, :, 1:2]) / factor
        want = m(torch.from_numpy(inp).to(cuda_device)).cpu().numpy() * factor
    for b, n in enumerate(nf):
        want[b, n:] = 0
    assert np.array_equal(fused, want), (prec, T, np.abs(fused - want).max())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["posemb_b2_t100", "cfg1_b1_t1", "cfg1_b1_t200"] + golden_names("edge_b3_t"))
def test_pos_emb_and_plain_models(name, prec, cuda_device):
    """A pos_emb model (25 input channels: the padded layer 1) and plain ones (24: the unpadded image) against the
    reference's own outputs and the oracle's operand-rounding model."""
    rec = load_golden(name)
    m = _model(rec, prec, cuda_device)
    x = torch.from_numpy(rec["x"]).to(cuda_device)
    with torch.no_grad():
        y = m.forward_into(x, _poisoned(torch.empty((rec["B"], rec["T"], 21, 2), device=cuda_device)))
    assert _all_written(y)
    y = y.cpu().numpy()
    ys = y[rec["y_idx"]] if "y_idx" in rec else y
    err = np.abs(ys - rec["y"]).max()
    ym = oracle.forward_from_state(rec["x"], rec["state"], pos_emb=rec["pos_emb"], mode=ORACLE_MODE[prec])
    errm = np.abs(y - ym).max()
    print(f"{name} {prec}: vs reference {err:.3e} (bar {_tol(rec, prec):.1e}), vs operand model {errm:.3e}")
    assert err <= _tol(rec, prec)
    assert errm <= TOL_MODEL[prec]
