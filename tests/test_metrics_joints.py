"""The two L1 losses over (B, T, J, 2) for the finger targets of `--predict right_index` (J = 4) and `right_3fingers`
(J = 12): forward and backward against the reference's classes (fixtures tests/golden/metric_j*_b5_t60.npz, written
by tests/golden/make_golden_tpt_geom.py) and against torch autograd of the reference formula, under the bars
tests/test_metrics.py and tests/test_train_gpu.py apply at J = 21; the shape rules; L12Pixels(J, 1280)."""
import numpy as np
import pytest
import torch

import hand_pose_sl_amd as hps
from tpt_geom_ref import load_metric
from train_ref import assert_within_bar, reference_loss


def test_shape_rules():
    p = torch.zeros((2, 5, 4, 2))
    for bad in (torch.zeros((2, 5, 4, 3)), torch.zeros((2, 5, 8)), torch.zeros((2, 5, 0, 2))):
        with pytest.raises(RuntimeError, match=r"\(B, T, J, 2\)"):
            hps.masked_pose_l1(bad, bad)
    with pytest.raises(RuntimeError, match=r"\(B, T, J, 2\)"):
        hps.masked_pose_l1(p, torch.zeros((2, 5, 12, 2)))            # prediction and target of different joint counts
    with pytest.raises(RuntimeError, match=r"scores must have shape \(2, 5, 4\)"):
        hps.weighted_pose_l1(p, p, [5, 5], torch.zeros((2, 5, 21)))
    with pytest.raises(RuntimeError, match=r"\(B, T, J\) scores"):
        hps.weighted_pose_l1(p, p, [5, 5], None)
    for J in (1, 4, 12, 21):                                         # right shapes get as far as the device check
        q = torch.zeros((2, 5, J, 2))
        with pytest.raises(RuntimeError, match="GPU only"):
            hps.masked_pose_l1(q, q)
        with pytest.raises(RuntimeError, match="GPU only"):
            hps.poderatedPoseL1()(q, q, [5, 5], torch.zeros((2, 5, J)))
    assert hps.l1_to_pixels(0.5, 4) == 0.5 / 4 * 1280 and hps.l1_to_pixels(0.5, 12) == 0.5 / 12 * 1280


@pytest.mark.gpu
@pytest.mark.parametrize("J", [4, 12])
def test_forward_matches_the_reference(J, cuda_device):
    r = load_metric(J)
    p, t, s = (torch.from_numpy(r[k]).to(cuda_device) for k in ("pred", "target", "scores"))
    lengths, valid = r["lengths"].tolist(), r["valid"].tolist()
    assert lengths == [60, 0, 33, 59, 17] and p.shape == (5, 60, J, 2)
    loss, per = hps.masked_pose_l1(p, t, lengths, return_per_sequence=True)
    wloss, wper = hps.weighted_pose_l1(p, t, lengths, s, return_per_sequence=True)
    for got, want in ((per, r["per_seq"]), (wper, r["wper_seq"])):
        got = got.cpu().numpy()
        assert np.isnan(got[1]) and np.isnan(want[1])               # the empty sequence: NaN, like torch's empty mean
        np.testing.assert_allclose(got[valid], want[valid], rtol=3e-6)
    assert np.isnan(float(loss)) and np.isnan(float(wloss)) and np.isnan(r["loss"]) and np.isnan(r["wloss"])
    vl = [lengths[i] for i in valid]
    loss = hps.maskedPoseL1()(p[valid], t[valid], vl)
    wloss = hps.poderatedPoseL1()(p[valid], t[valid], vl, s[valid])
    print(f"J={J}: L1 {float(loss):.8f} vs {float(r['loss_valid']):.8f}, confL1 {float(wloss):.8f} vs {float(r['wloss_valid']):.8f}")
    assert abs(float(loss) - float(r["loss_valid"])) <= 2e-6         # tests/test_metrics.py's bars at J = 21
    assert abs(float(wloss) - float(r["wloss_valid"])) <= 3e-6
    assert abs(float(hps.l1_to_pixels(loss, J)) - float(r["pixels_valid"])) <= 2e-3
    full = hps.masked_pose_l1(p, t)                                  # lengths None == all T frames
    assert abs(float(full) - float((p - t).abs().mean())) <= 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("J", [4, 12])
@pytest.mark.parametrize("kind", ["L1", "confL1"])
def test_gradients_match_autograd_of_the_reference_formula(kind, J, cuda_device):
    """tests/test_train_gpu.py::test_loss_gradients_match_reference_criteria at J joints, on the fixture's data."""
    r = load_metric(J)
    lengths = r["lengths"].tolist()
    pred, tgt, scores = (torch.from_numpy(r[k]).double() for k in ("pred", "target", "scores"))
    pred[0, 3, J - 1, 1] = tgt[0, 3, J - 1, 1] = 0.25              # a tie: sign(0) = 0
    want = {}
    for dt in (torch.float64, torch.float32):
        p = pred.detach().to(dt).clone().requires_grad_(True)
        (reference_loss(p.clone(), tgt.to(dt), lengths, scores.to(dt), kind) * 3.0).backward()
        want[dt] = p.grad.double()
    p = pred.float().to(cuda_device).requires_grad_(True)
    t, s = tgt.float().to(cuda_device), scores.float().to(cuda_device)
    loss = hps.masked_pose_l1(p, t, lengths) if kind == "L1" else hps.weighted_pose_l1(p, t, lengths, s)
    assert np.isnan(loss.item())                                    # lengths[1] == 0
    (loss * 3.0).backward()
    got = p.grad.cpu().double()
    assert got.shape == pred.shape
    assert not got[1].any() and not got[2, 33:].any() and not got[4, 17:].any() and got[0, 3, J - 1, 1] == 0
    assert got[0, :, :J - 1].abs().min() > 0                        # every counted element has a gradient
    assert_within_bar(got.numpy(), want[torch.float64].numpy(), (want[torch.float32] - want[torch.float64]).abs().max(), kind)


@pytest.mark.gpu
def test_validate_pixels_follow_the_joint_count(cuda_device):
    """validate(..., return_pixels=True) divides by the prediction's joints: L12Pixels(4, 1280) for (29, 8)."""
    import tpt_geom_ref as G
    model = G.recipe_model(5, 60, 29, 8, 1, 1).to(cuda_device)
    tok, pose = G.inputs(2, 9, 17, 60, 29, 3)
    g = torch.Generator().manual_seed(4)
    batch = {"text_tokens": tok, "input_kp": pose, "target_kp": torch.rand((2, 17, 4, 2), generator=g) - 0.5,
             "n_frames": torch.tensor([17, 9])}
    value, pixels = hps.validate(model, [batch], loss="L1", return_pixels=True)
    assert pixels == value / 4 * 1280
    pred = G.Checker(model)(tok, pose)
    want = np.mean([float((pred[b, :n] - batch["target_kp"][b, :n].double()).abs().mean()) for b, n in enumerate((17, 9))])
    assert abs(value - want) <= G.tol(pred)
