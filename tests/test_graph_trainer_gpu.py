"""Captured training epochs on the MI355X: b2h_epoch_plan against its restatement tests/plan_ref.py, bit for bit;
b2h_build_batch_planned against tests/batch_ref.py on the plan's slice, at every step of a ragged plan and beyond both of
its ends, between poisoned guard bands; b2h_epoch_record in and out of range; `GraphTrainer.epoch()` against
`train_epoch()` on a twin model from the same seeds -- losses equal as floats, parameters and Adam state torch.equal --
for the three models, both losses, native dropout, a partial last batch, shuffled random crops, the blocked MFMA
attention under replay, a recapture, a learning-rate edit and the native plan; every refusal of the constructor."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import batch_ref
import hand_pose_sl_amd as hps
import plan_ref
import poison
from hand_pose_sl_amd import _lib

pytestmark = pytest.mark.gpu
FLOATS = ("input_kp", "target_kp", "target_conf")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- 1. the epoch plan -------------------------------------------------------------------------------------------------
def _offsets(lengths):
    return torch.tensor([0] + np.cumsum(lengths).tolist(), dtype=torch.int64)


def _plan_cases():
    h5 = batch_ref.load_fixture("h5_store")["store"][1]
    gen = np.random.default_rng(5)
    return {"n1": _offsets([19]), "n2": _offsets([3, 40]), "n5": _offsets([0, 7, 8, 19, 500]), "fixture": h5,
            "n1000": _offsets(gen.integers(0, 60, 1000).tolist())}                     # four blocks, h = 5


@pytest.mark.parametrize("case", ["n1", "n2", "n5", "fixture", "n1000"])
def test_epoch_plan_equals_the_restatement(cuda_device, case):
    offsets = _plan_cases()[case]
    n, T, lib = offsets.numel() - 1, 7, _lib.load()
    doff = offsets.to(cuda_device)
    for shuffle in (0, 1):
        for crop in (0, 1):
            for seed, epoch in ((0, 0), (3, 1), (0xFEDCBA9876543210, (1 << 40) + 2)):
                utt = torch.full((n,), -7, dtype=torch.int64, device=cuda_device)
                start = torch.full((n,), -7, dtype=torch.int64, device=cuda_device)
                _lib.check(lib.b2h_epoch_plan(_p(doff), n, T, shuffle, crop, seed, epoch, _p(utt), _p(start), _stream(cuda_device)))
                want_utt, want_start = plan_ref.plan(offsets.tolist(), n, T, shuffle, crop, seed, epoch)
                assert utt.tolist() == want_utt, (shuffle, crop, seed, epoch)
                assert start.tolist() == want_start, (shuffle, crop, seed, epoch)
                if not crop:                                          # start_plan may be left out, offsets too
                    alone = torch.full((n,), -7, dtype=torch.int64, device=cuda_device)
                    _lib.check(lib.b2h_epoch_plan(None, n, T, shuffle, 0, seed, epoch, _p(alone), None, _stream(cuda_device)))
                    assert alone.tolist() == want_utt


def test_epoch_plan_between_poisoned_guard_bands(cuda_device):
    offsets = _plan_cases()["n1000"]
    lib, st = _lib.load(), _stream(cuda_device)
    out = poison.launch(lambda p: lib.b2h_epoch_plan(p["offsets"], 1000, 7, 1, 1, 11, 4, p["utt_plan"], p["start_plan"], st),
                        {"offsets": offsets}, {"utt_plan": (1000, 2), "start_plan": (1000, 2)}, cuda_device)
    want_utt, want_start = plan_ref.plan(offsets.tolist(), 1000, 7, True, True, 11, 4)
    assert out["utt_plan"].view(torch.int64).view(-1).tolist() == want_utt
    assert out["start_plan"].view(torch.int64).view(-1).tolist() == want_start


# ---- 2. the planned build ----------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 6, 7, 8, 21]


@functools.lru_cache(maxsize=None)
def _store(n_body=8, S=5, seed=3):
    gen = torch.Generator().manual_seed(seed)
    J = n_body + 42
    rows = torch.rand((sum(LENGTHS), 3, J), generator=gen) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)
    tokens = torch.randint(0, 1000, (len(LENGTHS), S), generator=gen)
    return rows.reshape(-1, 3 * J).contiguous(), _offsets(LENGTHS), n_body, tokens


UTT_PLAN = [5, 3, 4, 1, 2, 5, 0]           # 7 entries at B = 2: three full steps and a ragged one
START_PLAN = [3, 0, 1, 0, 5, 14, 0]


@pytest.mark.parametrize("step", [0, 1, 2, 3, -1, 4, 1 << 62, -(1 << 62)])
@pytest.mark.parametrize("with_start", [True, False])
def test_planned_build_equals_the_restatement_on_the_plans_slice(cuda_device, step, with_start):
    rows, offsets, n_body, tokens = _store()
    B, T, S, n_plan = 2, 7, 5, len(UTT_PLAN)
    lib, st = _lib.load(), _stream(cuda_device)
    ins = {"rows": rows, "offsets": offsets, "tokens": tokens, "utt_plan": torch.tensor(UTT_PLAN), "step": torch.tensor([step])}
    if with_start:
        ins["start_plan"] = torch.tensor(START_PLAN)
    out = poison.launch(
        lambda p: lib.b2h_build_batch_planned(p["rows"], rows.shape[0], p["offsets"], len(LENGTHS), n_body, p["tokens"], S,
                                              p["utt_plan"], p.get("start_plan"), n_plan, p["step"], B, T, 0, 3, 1280.0,
                                              p["input_kp"], p["target_kp"], p["target_conf"], p["text_tokens"], p["n_frames"], st),
        ins, {"input_kp": (B, T, n_body, 2), "target_kp": (B, T, 21, 2), "target_conf": (B, T, 21), "text_tokens": (B, S, 2),
              "n_frames": (B, 2)}, cuda_device)                   # an int64 output counts as two words: all overwritten
    got = {k: out[k].cpu() for k in FLOATS}
    got["text_tokens"] = out["text_tokens"].view(torch.int64).view(B, S).cpu()
    got["n_frames"] = out["n_frames"].view(torch.int64).view(B).cpu()
    entries = [step * B + b for b in range(B)] if 0 <= step <= n_plan else [-1] * B
    have = [b for b, e in enumerate(entries) if 0 <= e < n_plan]
    assert len(have) == {0: 2, 1: 2, 2: 2, 3: 1}.get(step, 0)
    if have:
        sl = [entries[b] for b in have]
        want = batch_ref.batch(rows, offsets, n_body, tokens, [UTT_PLAN[e] for e in sl],
                               [START_PLAN[e] for e in sl] if with_start else None, T)
        for k, w in want.items():
            assert torch.equal(got[k][have], w) and batch_ref.same_bits(got[k][have], w), (k, step)
    for b in set(range(B)) - set(have):                           # no entry: an unknown utterance, loud
        for k in FLOATS:
            assert bool((got[k][b].view(torch.int32) == 0x7FC00000).all()), (k, step)
        assert got["text_tokens"][b].tolist() == [-1] * S and int(got["n_frames"][b]) == 0


def test_loader_build_planned_walks_the_plan_with_the_step_word(cuda_device):
    rows, offsets, n_body, tokens = _store()
    ds = hps.DeviceDataset(rows, offsets, n_body, tokens)
    loader = hps.DeviceLoader(ds, 2, 7, selection="randomcrop")
    plan = (torch.tensor(UTT_PLAN[:6], device=cuda_device), torch.tensor(START_PLAN[:6], device=cuda_device))
    word = torch.zeros(1, dtype=torch.int64, device=cuda_device)
    out = loader.empty_batch(2)
    for s in range(3):
        assert loader.build_planned(plan, word, out) is out
        want = loader.build(plan[0][2 * s:2 * s + 2], plan[1][2 * s:2 * s + 2])
        for k in want:
            assert batch_ref.same_bits(out[k].cpu(), want[k].cpu()), (k, s)
        word.add_(1)
    assert bool(torch.isnan(loader.build_planned(plan, word, out)["input_kp"]).all())      # past the end
    with pytest.raises(ValueError, match="step_word"):
        loader.build_planned(plan, torch.zeros(1, dtype=torch.int64), out)                 # a host word
    with pytest.raises(ValueError, match="start_plan"):
        loader.build_planned((plan[0], plan[1][:3]), word, out)
    with pytest.raises(ValueError, match="plan_source"):
        hps.DeviceLoader(ds, 2, 7, plan_source="numpy")


def test_torch_plan_is_what_iter_draws(cuda_device):
    rows, offsets, n_body, tokens = _store()
    ds = hps.DeviceDataset(rows, offsets, n_body, tokens)
    for drop_last in (False, True):
        loader = hps.DeviceLoader(ds, 4, 7, selection="randomcrop", shuffle=True, drop_last=drop_last)
        torch.manual_seed(5)
        eager = list(loader)
        torch.manual_seed(5)
        utt, start = loader.plan_epoch()
        assert sorted(utt.tolist()) == list(range(6)) and start.shape == utt.shape and len(eager) == (1 if drop_last else 2)
        for i, want in enumerate(eager):
            got = loader.build(utt[4 * i:4 * i + 4], start[4 * i:4 * i + 4])
            for k in want:
                assert batch_ref.same_bits(got[k].cpu(), want[k].cpu()), (k, i, drop_last)
        assert not drop_last or start[4:].tolist() == [0, 0]
    first = hps.DeviceLoader(ds, 4, 7, selection="first")
    utt, start = first.plan_epoch()
    assert utt.tolist() == list(range(6)) and start is None


def test_native_plan_of_the_loader_is_the_restatement(cuda_device):
    rows, offsets, n_body, tokens = _store()
    ds = hps.DeviceDataset(rows, offsets, n_body, tokens)
    loader = hps.DeviceLoader(ds, 4, 7, selection="randomcrop", shuffle=True, plan_source="native", seed=9)
    for epoch in (0, 1):                                             # the loader counts the epochs itself
        utt, start = loader.plan_epoch()
        want = plan_ref.plan(offsets.tolist(), 6, 7, True, True, 9, epoch)
        assert (utt.tolist(), start.tolist()) == want
    utt, start = loader.plan_epoch(epoch=7)
    assert (utt.tolist(), start.tolist()) == plan_ref.plan(offsets.tolist(), 6, 7, True, True, 9, 7) and loader.epochs_planned == 2
    batches = list(loader)                                           # __iter__ iterates the plan of epoch 2
    want = plan_ref.plan(offsets.tolist(), 6, 7, True, True, 9, 2)
    ref = batch_ref.batch(rows, offsets, n_body, tokens, want[0][4:], want[1][4:], 7)
    assert len(batches) == 2 and all(batch_ref.same_bits(batches[1][k].cpu(), ref[k]) for k in ref)
    other = hps.DeviceLoader(ds, 4, 7, selection="randomcrop", shuffle=True, plan_source="native", seed=10).plan_epoch()
    mine = loader.plan_epoch(epoch=0)
    assert not (torch.equal(other[0], mine[0]) and torch.equal(other[1], mine[1]))       # two seeds differ


# ---- 3. the record -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step,slot", [(0, 0), (2, 2), (3, None), (-1, None), (1 << 40, None)])
def test_epoch_record_in_and_out_of_range(cuda_device, step, slot):
    lib, st = _lib.load(), _stream(cuda_device)
    loss = torch.tensor([1.25], device=cuda_device)
    losses = torch.tensor([7.0, 8.0, 9.0, 10.0], device=cuda_device)       # the fourth is past n_losses = 3
    word = torch.tensor([step], device=cuda_device)
    _lib.check(lib.b2h_epoch_record(_p(loss), _p(losses), 3, _p(word), st))
    want = [7.0, 8.0, 9.0, 10.0]
    if slot is not None:
        want[slot] = 1.25
    assert losses.tolist() == want and word.tolist() == [step + 1] and loss.tolist() == [1.25]
    _lib.check(lib.b2h_epoch_record(_p(loss), None, 0, _p(word), st))     # no array: the word still advances
    assert word.tolist() == [step + 2]


# ---- 4. GraphTrainer ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _h5():
    """The HDF5 fixture's utterances of 1, 3, 7, 8 and 19 frames (the empty one's loss is 0 / 0 = NaN, in the reference
    as here, which no equality of floats survives): 5 utterances, so B = 2 leaves a partial last batch."""
    rows, offsets, n_body, tokens = batch_ref.load_fixture("h5_store")["store"]
    assert offsets[:2].tolist() == [0, 0]
    return hps.DeviceDataset(rows, offsets[1:].clone(), n_body, tokens[1:].clone())


@functools.lru_cache(maxsize=None)
def _json():
    rec = batch_ref.load_fixture("json_store")
    return hps.DeviceDataset.from_frames(rec["frames"], rec["store"][3])


@functools.lru_cache(maxsize=None)
def _long():
    """Five 8-joint utterances around 130 frames, two of them longer: random crops at max_frames = 130."""
    gen = torch.Generator().manual_seed(41)
    lengths = [150, 131, 40, 130, 200]
    rows = torch.rand((sum(lengths), 3, 50), generator=gen) * torch.tensor([1280.0, 720.0, 1.0]).view(1, 3, 1)
    return hps.DeviceDataset(rows.reshape(-1, 150).contiguous(), _offsets(lengths), 8, torch.randint(0, 1000, (5, 5), generator=gen))


def _tpt(dev, dropout=0.0):
    torch.manual_seed(31)
    m = hps.TextPoseTransformer(1000, 8, 2, 4, 128, 42, 1, 1, dropout=dropout).to(dev)
    return m.set_dropout_source("native", 17) if dropout else m


def _conv(dev):
    torch.manual_seed(32)
    return hps.ConvModel(30, "ReLU", False).to(dev)


def _tenc(dev):
    torch.manual_seed(33)
    return hps.TransformerEnc(24, 4, 128, 42, 1, dropout=0.0).to(dev)


def _compare(dev, make_model, make_loader, loss="L1", epochs=2, between=None, captures=1):
    """`epochs` GraphTrainer epochs against as many train_epoch() calls on a twin from the same seeds; `between(model,
    optimizer)` runs on both sides before every epoch but the first.  Returns the trainer and its model."""
    eager_model, eager_loader = make_model(dev), make_loader()
    eager_opt = hps.Adam(eager_model.parameters(), lr=1e-3)
    torch.manual_seed(77)
    eager = []
    for e in range(epochs):
        if e and between:
            between(eager_model, eager_opt)
        eager.append(hps.train_epoch(eager_model, eager_loader, None, eager_opt, loss=loss))
    model, loader = make_model(dev), make_loader()
    opt = hps.Adam(model.parameters(), lr=1e-3)
    trainer = hps.GraphTrainer(model, loader, opt, loss=loss)
    torch.manual_seed(77)
    got = []
    for e in range(epochs):
        if e and between:
            between(model, opt)
        got.append(trainer.epoch())
    assert got == eager and all(np.isfinite(v) for v in got), (got, eager)
    for (k, a), b in zip(model.named_parameters(), eager_model.parameters()):
        assert torch.equal(a, b), k
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[a][key], eager_opt.state[b][key]), (k, key)
    full = len(loader.ds) // loader.batch_size
    steps = epochs * (full + (0 if loader.drop_last or len(loader.ds) % loader.batch_size == 0 else 1))
    assert opt.steps_done() == eager_opt.steps_done() == steps
    assert trainer.captures == captures and trainer.replays == epochs * full - captures
    return trainer, model


@pytest.mark.parametrize("loss,dropout", [("L1", 0.0), ("confL1", 0.0), ("L1", 0.1)])
def test_trainer_equals_train_epoch_with_a_partial_last_batch(cuda_device, loss, dropout):
    trainer, model = _compare(cuda_device, lambda d: _tpt(d, dropout), lambda: hps.DeviceLoader(_h5(), 2, 7, selection="first"), loss)
    assert trainer.replays == 3                                        # 2 epochs x 2 full steps, the first one eager
    fresh = _tpt(cuda_device, dropout)
    assert any(not torch.equal(a, b) for a, b in zip(model.parameters(), fresh.parameters()))      # it did train
    model.eval()                                                       # and inference sees the trained weights
    tok, pose = torch.randint(0, 1000, (1, 5), device=cuda_device), torch.rand((1, 7, 8, 2), device=cuda_device)
    with torch.no_grad():
        assert not torch.equal(model(tok, pose), fresh.eval()(tok, pose))


def test_trainer_equals_train_epoch_shuffled_with_random_crops(cuda_device):
    _compare(cuda_device, _tpt, lambda: hps.DeviceLoader(_h5(), 2, 7, selection="randomcrop", shuffle=True))


def test_trainer_drops_the_last_batch_when_the_loader_does(cuda_device):
    _compare(cuda_device, _tpt, lambda: hps.DeviceLoader(_h5(), 2, 7, selection="randomcrop", shuffle=True, drop_last=True))


def test_trainer_convmodel(cuda_device):
    _compare(cuda_device, _conv, lambda: hps.DeviceLoader(_json(), 2, 7, selection="randomcrop", pad="frame0", shuffle=True))


def test_trainer_transformer_enc(cuda_device):
    _compare(cuda_device, _tenc, lambda: hps.DeviceLoader(_json(), 2, 7, selection="randomcrop", pad="frame0", shuffle=True))


def test_trainer_blocked_mfma_attention_under_replay(cuda_device):
    def model(dev):
        return _tpt(dev).set_train_kernels("mfma").set_train_linear("mfma")
    _, m = _compare(cuda_device, model, lambda: hps.DeviceLoader(_long(), 2, 130, selection="randomcrop", shuffle=True))
    assert _lib.load().b2h_tpt_train_attn_name(m._handle, 130) == b"b2h_mt_sdpa"


def test_trainer_recaptures_when_the_linear_route_changes(cuda_device):
    def switch(model, opt):
        model.set_train_linear("mfma")
    trainer, _ = _compare(cuda_device, _tpt, lambda: hps.DeviceLoader(_h5(), 2, 7, selection="first"), between=switch,
                          epochs=3, captures=2)
    assert trainer.replays == 4                  # 6 full steps: one eager and one capture per route


def test_trainer_honours_a_learning_rate_edit_between_epochs(cuda_device):
    def decay(model, opt):
        opt.param_groups[0]["lr"] = 1e-2         # adjust_learning_rate, steps/utils.py:301-307
    trainer, _ = _compare(cuda_device, _tpt, lambda: hps.DeviceLoader(_h5(), 2, 7, selection="first"), between=decay)
    assert trainer.optimizer._lr_word.item() == np.float32(1e-2)       # no recapture: the rate is a device word


def test_trainer_native_plan_equals_an_eager_epoch_over_the_same_loader(cuda_device):
    def loader():
        return hps.DeviceLoader(_h5(), 2, 7, selection="randomcrop", shuffle=True, plan_source="native", seed=3)
    _compare(cuda_device, _tpt, loader)
    a, b = loader().plan_epoch(), hps.DeviceLoader(_h5(), 2, 7, selection="randomcrop", shuffle=True, plan_source="native",
                                                   seed=4).plan_epoch()
    assert not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))


def test_trainer_refusals_name_the_remedy(cuda_device):
    loader = hps.DeviceLoader(_h5(), 2, 7, selection="first")
    m = _tpt(cuda_device)
    opt = hps.Adam(m.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="DeviceLoader"):
        hps.GraphTrainer(m, list(loader), opt)
    with pytest.raises(ValueError, match="hand_pose_sl_amd.Adam"):
        hps.GraphTrainer(m, loader, torch.optim.Adam(m.parameters(), lr=1e-3))
    torch.manual_seed(31)
    dropping = hps.TextPoseTransformer(1000, 8, 2, 4, 128, 42, 1, 1, dropout=0.1).to(cuda_device)
    with pytest.raises(ValueError, match="set_dropout_source"):
        hps.GraphTrainer(dropping, loader, hps.Adam(dropping.parameters()))
    hps.GraphTrainer(dropping.set_dropout_source("native", 1), loader, hps.Adam(dropping.parameters()))
    torch.manual_seed(33)
    enc = hps.TransformerEnc(24, 4, 128, 42, 1, dropout=0.2).to(cuda_device)
    with pytest.raises(ValueError, match="set_dropout_source"):
        hps.GraphTrainer(enc, hps.DeviceLoader(_json(), 2, 7, pad="frame0"), hps.Adam(enc.parameters()))
    for bad in ("MSE", "huber"):
        with pytest.raises(ValueError, match="L1 or confL1"):
            hps.GraphTrainer(m, loader, opt, loss=bad)
    with pytest.raises(ValueError, match="L1 or confL1"):
        hps.GraphTrainer(m, loader, opt, torch.nn.MSELoss())
    with pytest.raises(ValueError, match="right_hand"):
        hps.GraphTrainer(_conv(cuda_device), hps.DeviceLoader(_json(), 2, 7, predict="right_index"), opt)
    assert opt.steps_done() == 0                                       # nothing ran
