"""`mask_padding=True` through the loops on the MI355X: train_epoch() against GraphTrainer on a twin
from the same seeds, validate() and predict_dataset() against the per-batch computation done by hand, on a store of five
short utterances with padded token rows, batch_size 2, max_frames 20 and native dropout."""
import functools

import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
from hand_pose_sl_amd.predict import window_plan

pytestmark = pytest.mark.gpu
LENGTHS = [3, 20, 11, 7, 25]                 # around max_frames = 20: shorter, equal, longer (two windows)
TOKENS = [[5, 9, 2, 0, 0, 0], [7, 0, 0, 0, 0, 0], [3, 0, 4, 8, 1, 6], [0, 0, 0, 0, 0, 0], [2, 2, 0, 0, 0, 0]]
TOKEN_LENGTHS = [3, 1, 6, 1, 2]
B, T = 2, 20


@functools.lru_cache(maxsize=None)
def _store():
    gen = torch.Generator().manual_seed(51)
    rows = torch.rand((sum(LENGTHS), 3, 50), generator=gen) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)
    offsets = torch.tensor([0] + np.cumsum(LENGTHS).tolist(), dtype=torch.int64)
    return hps.DeviceDataset(rows.reshape(-1, 150).contiguous(), offsets, 8, torch.tensor(TOKENS, dtype=torch.int64))


def _loader(**kw):
    return hps.DeviceLoader(_store(), B, T, selection="first", **kw)


def _model(dev, dropout=0.1):
    torch.manual_seed(52)
    m = hps.TextPoseTransformer(10, 8, 2, 4, 128, 42, 1, 1, dropout=dropout).to(dev)
    return m.set_dropout_source("native", 19) if dropout else m


def test_store_token_lengths(cuda_device):
    assert hps.token_lengths(_store().tokens).cpu().tolist() == TOKEN_LENGTHS


def test_train_epoch_equals_graph_trainer_and_the_flag_is_part_of_the_capture(cuda_device):
    eager_model, eager_opt = _model(cuda_device), None
    eager_opt = hps.Adam(eager_model.parameters(), lr=1e-3)
    eager = [hps.train_epoch(eager_model, _loader(), None, eager_opt, loss="L1", mask_padding=True) for _ in range(2)]
    model = _model(cuda_device)
    opt = hps.Adam(model.parameters(), lr=1e-3)
    trainer = hps.GraphTrainer(model, _loader(), opt, loss="L1", mask_padding=True)
    got = [trainer.epoch() for _ in range(2)]
    assert got == eager and all(np.isfinite(v) for v in got), (got, eager)
    for (k, a), b in zip(model.named_parameters(), eager_model.parameters()):
        assert torch.equal(a, b), k
    assert trainer.captures == 1 and trainer.replays == 3          # 2 epochs x 2 full steps, the first one eager
    # the masks change the training: a twin without the flag ends elsewhere
    plain_model = _model(cuda_device)
    plain_opt = hps.Adam(plain_model.parameters(), lr=1e-3)
    plain = [hps.train_epoch(plain_model, _loader(), None, plain_opt, loss="L1") for _ in range(2)]
    assert plain != eager
    # toggling the flag captures again, and the unmasked epochs are then train_epoch()'s own
    trainer.mask_padding = False
    key = trainer._graph_key()
    assert key != trainer._key
    trainer.epoch()
    assert trainer.captures == 2
    trainer.mask_padding = True
    trainer.epoch()
    assert trainer.captures == 3
    twin = _model(cuda_device)
    off = hps.GraphTrainer(twin, _loader(), hps.Adam(twin.parameters(), lr=1e-3), loss="L1")
    assert [off.epoch() for _ in range(2)] == plain
    for a, b in zip(twin.parameters(), plain_model.parameters()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("loss", ["L1", "confL1"])
def test_validate_equals_the_batches_done_by_hand(loss, cuda_device):
    model = _model(cuda_device).eval()
    got = hps.validate(model, _loader(), loss=loss, mask_padding=True)
    values = []
    with torch.no_grad():
        for batch in _loader():
            pred = model(batch["text_tokens"], batch["input_kp"], text_lengths=hps.token_lengths(batch["text_tokens"]),
                         frame_lengths=batch["n_frames"])
            if loss == "L1":
                values.append(hps.masked_pose_l1(pred, batch["target_kp"], batch["n_frames"]))
            else:
                values.append(hps.weighted_pose_l1(pred, batch["target_kp"], batch["n_frames"], batch["target_conf"]))
    assert len(values) == 3
    assert got == float(torch.stack(values).double().mean())
    assert got != hps.validate(model, _loader(), loss=loss)


def test_predict_dataset_equals_forward_fused_per_window(cuda_device):
    model = _model(cuda_device, dropout=0.0).eval()
    loader = _loader(pad="frame0")
    ds = loader.ds
    got = hps.predict_dataset(model, loader, mask_padding=True)
    utt, start, skip = (t.to(ds.device) for t in window_plan(ds, T, "all"))
    assert utt.numel() == 6                                        # the 25-frame utterance has two windows
    rows = ds.rows.clone()
    with torch.no_grad():
        for i in range(0, utt.numel(), B):
            u, s, k = utt[i:i + B], start[i:i + B], skip[i:i + B]
            batch = loader.build(u, s)
            pred = model.forward_fused(batch["text_tokens"], batch["input_kp"], dif_encoding=False, normalize=False,
                                       denormalize=False, text_lengths=hps.token_lengths(batch["text_tokens"]),
                                       frame_lengths=batch["n_frames"])
            loader.write_back(pred.contiguous(), u, s, k, rows, 1.0)
    assert torch.equal(got.rows, rows)
    assert not torch.equal(got.rows, hps.predict_dataset(model, loader).rows)
    assert model.training is False
