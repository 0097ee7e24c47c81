"""Captured training epochs with augmentation on the MI355X: `GraphTrainer.epoch()` against `train_epoch()` on a twin
model from the same seeds, over a `DeviceLoader(augment=Augment(...))` with a native plan -- losses equal as floats,
parameters and Adam state torch.equal, one capture --; a changed `Augment` field captures again; `augment=None` is the
loader without the argument."""
import functools

import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps

pytestmark = pytest.mark.gpu
LENGTHS = [3, 16, 17, 40, 9, 25, 16, 31, 12]            # 9 utterances at B = 4: two full steps and a partial one
AUGMENT = hps.Augment(scale=0.2, rotate_deg=15, mirror=0.5, jitter=3)


@functools.lru_cache(maxsize=None)
def _dataset():
    gen = torch.Generator().manual_seed(51)
    rows = torch.rand((sum(LENGTHS), 3, 54), generator=gen) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)
    offsets = torch.tensor([0] + np.cumsum(LENGTHS).tolist(), dtype=torch.int64)
    return hps.DeviceDataset(rows.reshape(-1, 162).contiguous(), offsets, 12)


def _conv(dev):
    torch.manual_seed(32)
    return hps.ConvModel(30, "ReLU", False).to(dev)


def _loader(**kw):
    return hps.DeviceLoader(_dataset(), 4, 16, selection="randomcrop", pad="frame0", shuffle=True, plan_source="native", seed=5, **kw)


def _run(dev, make_loader, graph, epochs=2, between=None):
    """`epochs` epochs of GraphTrainer.epoch() (graph) or train_epoch(); `between(loader)` runs before every epoch but the
    first.  Returns (losses, model, optimizer, trainer or None)."""
    model, loader = _conv(dev), make_loader()
    opt = hps.Adam(model.parameters(), lr=1e-3)
    trainer = hps.GraphTrainer(model, loader, opt, loss="L1") if graph else None
    losses = []
    for e in range(epochs):
        if e and between:
            between(loader)
        losses.append(trainer.epoch() if graph else hps.train_epoch(model, loader, None, opt, loss="L1"))
    return losses, model, opt, trainer


def _assert_equal_runs(a, b):
    (la, ma, oa, _), (lb, mb, ob, _) = a, b
    assert la == lb and all(np.isfinite(v) for v in la), (la, lb)
    for (k, p), q in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(p, q), k
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[p][key], ob.state[q][key]), (k, key)
    assert oa.steps_done() == ob.steps_done()


def test_trainer_equals_train_epoch_with_augmentation(cuda_device):
    graph = _run(cuda_device, lambda: _loader(augment=AUGMENT), True)
    eager = _run(cuda_device, lambda: _loader(augment=AUGMENT), False)
    _assert_equal_runs(graph, eager)
    trainer = graph[3]
    assert trainer.captures == 1 and trainer.replays == 2 * 2 - 1       # 2 epochs x 2 full steps, the first one eager
    assert graph[2].steps_done() == 2 * 3
    assert graph[0][0] != graph[0][1]
    plain = _run(cuda_device, _loader, False)                           # and the augmentation did reach the model
    assert plain[0] != eager[0]
    assert any(not torch.equal(p, q) for p, q in zip(plain[1].parameters(), eager[1].parameters()))


def test_trainer_captures_again_when_an_augment_field_changes(cuda_device):
    def change(loader):
        loader.augment = hps.Augment(scale=0.2, rotate_deg=15, mirror=0.5, jitter=4)
    graph = _run(cuda_device, lambda: _loader(augment=AUGMENT), True, epochs=3, between=change)
    eager = _run(cuda_device, lambda: _loader(augment=AUGMENT), False, epochs=3, between=change)
    _assert_equal_runs(graph, eager)
    trainer = graph[3]
    assert trainer.captures == 2 and trainer.replays == 6 - 2           # 6 full steps: one eager and one capture per Augment
    same = _run(cuda_device, lambda: _loader(augment=AUGMENT), True, epochs=3,
                between=lambda loader: setattr(loader, "augment", hps.Augment(0.2, 15, 0.5, 3)))
    assert same[3].captures == 1 and same[3].replays == 6 - 1                                       # an equal value: no capture
    assert same[0][0] == graph[0][0] and same[0][1] != graph[0][1]                                  # the new jitter was used


def test_augment_none_is_the_loader_without_the_argument(cuda_device):
    without = _run(cuda_device, _loader, True)
    with_none = _run(cuda_device, lambda: _loader(augment=None), True)
    _assert_equal_runs(with_none, without)
    for run in (without, with_none):
        assert run[3].captures == 1 and run[3].replays == 3
    _assert_equal_runs(with_none, _run(cuda_device, lambda: _loader(augment=None), False))
    zero = _run(cuda_device, lambda: _loader(augment=hps.Augment()), True)      # all four 0: the plain batches, bit for bit
    _assert_equal_runs(zero, without)
