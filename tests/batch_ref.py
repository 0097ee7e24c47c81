"""A torch restatement, on the host, of the batch the reference's datasets and transforms build -- written for the tests
of b2h_build_batch (and timed as "the host path" by tools/bench_loader.py), from the store layout of include/b2h.h:

  item(...)   one utterance: the window (select_jsons, text_pose_dataset.py:52-68, with the start given), padding with
              zeros before any transform (TextPoseH5Dataset.pad, :614-624) or with the window's first frame (the JSON
              datasets' pad, :511-519), clipping, then WristDifference, ChestDifference, NormalizeFixedFactor and one
              Build*Item in run.py:83-104's order (steps/utils.py:180-277)
  batch(...)  the items of a batch stacked as torch's default collate stacks them

Plain tensor expressions in the reference's operation order, so every element is the same IEEE subtraction and
division; tests/test_build_batch_cpu.py holds it to the fixtures made from the reference's own methods, bit for bit.
A helper module, not a conftest.py: the tests import it by name.
"""
import glob
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = os.path.join(ROOT, "tests", "golden", "batches")
PREDICTS = ("right_hand", "right_index", "right_3fingers")
TARGET = {"right_hand": slice(0, 21), "right_index": slice(5, 9), "right_3fingers": slice(1, 13)}
JOINTS = {"right_hand": None, "right_index": (29, 4), "right_3fingers": (21, 12)}


def joints(predict, n_body):
    return (n_body, 21) if predict == "right_hand" else JOINTS[predict]


def item(rows, n_body, T, start, predict, dif, norm, factor, frame0):
    """rows: (len, 3 J) float32 tensor of ONE utterance -> (input_kp, target_kp, target_conf, n_frames)."""
    J = n_body + 42
    n = rows.shape[0]
    if n > T:
        s = min(max(int(start), 0), n - T)
        rows = rows[s:s + T]
    elif n < T:
        if frame0 and n > 0:
            rows = torch.cat([rows, rows[:1].expand(T - n, 3 * J)], dim=0)
        else:
            rows = torch.cat([rows, torch.zeros((T - n, 3 * J), dtype=rows.dtype)], dim=0)
    a = rows.reshape(T, 3, J).permute(0, 2, 1)
    kp, conf = a[:, :, :2], a[:, :, 2]
    body, hand, hand_conf = kp[:, :n_body], kp[:, n_body + 21:], conf[:, n_body + 21:]
    if dif:
        hand = hand - body[:, 4].unsqueeze(1)       # WristDifference: the raw body wrist
        body = body - body[:, 1].unsqueeze(1)       # ChestDifference
    if norm:
        body, hand = body / factor, hand / factor
    if predict == "right_hand":
        inp = body
    elif predict == "right_index":
        inp = torch.cat([body, hand[:, 0:5], hand[:, 9:]], dim=1)
    elif predict == "right_3fingers":
        inp = torch.cat([hand[:, 13:], hand[:, 0].unsqueeze(1), body], dim=1)
    else:
        raise ValueError(predict)
    return inp.contiguous(), hand[:, TARGET[predict]].contiguous(), hand_conf[:, TARGET[predict]].contiguous(), min(n, T)


def batch(rows, offsets, n_body, tokens, utt, start, T, predict="right_hand", dif=True, norm=True, factor=1280,
          frame0=False):
    """The batch dict of the utterances `utt` cropped at `start` (None = 0) from a host store (torch tensors)."""
    items = []
    for b, u in enumerate(int(v) for v in utt):
        r = rows[int(offsets[u]):int(offsets[u + 1])]
        items.append(item(r, n_body, T, 0 if start is None else int(start[b]), predict, dif, norm, factor, frame0))
    out = {"input_kp": torch.stack([i[0] for i in items]), "target_kp": torch.stack([i[1] for i in items]),
           "target_conf": torch.stack([i[2] for i in items]), "n_frames": torch.tensor([i[3] for i in items], dtype=torch.int64)}
    if tokens is not None:
        out["text_tokens"] = torch.stack([tokens[int(u)] for u in utt])
    return out


# ---- the committed fixtures (tests/golden/make_golden_batches.py) ---------------------------------------------------
def variants(n_body):
    """(predict, dif, norm) of every expected batch a fixture of this body size holds."""
    return [(p, d, n) for p in (PREDICTS if n_body == 12 else PREDICTS[:1]) for d in (0, 1) for n in (0, 1)]


def key(predict, dif, norm, sel, name):
    return f"{predict}_d{dif}_n{norm}_{sel}_{name}"


def load_fixture(name):
    """One fixture: the store as host tensors, T, the utterance lists and every expected batch.
    rec["store"] = (rows, offsets, n_body, tokens); rec["lists"] = {list name: utt}; rec["starts"][(sel, list name)];
    rec["expected"][(predict, dif, norm, sel, list name)] = batch dict of host tensors."""
    with np.load(os.path.join(BATCHES, name + ".npz")) as d:
        raw = {k: d[k] for k in d.files}
    n_body, T, S = (int(v) for v in raw["meta"])
    rec = {"n_body": n_body, "T": T, "S": S, "frame0": n_body == 12,
           "store": (torch.from_numpy(raw["rows"]), torch.from_numpy(raw["offsets"]), n_body, torch.from_numpy(raw["tokens"])),
           "lists": {}, "starts": {}, "expected": {}}
    if "frames_json" in raw:
        rec["frames"] = json.loads(str(raw["frames_json"]))
    for k in raw:
        if k.startswith("utt_"):
            rec["lists"][k[4:]] = torch.from_numpy(raw[k])
    sels = sorted({k.split("_")[1] for k in raw if k.startswith("start_")})
    for sel in sels:
        for ln in rec["lists"]:
            rec["starts"][(sel, ln)] = torch.from_numpy(raw[f"start_{sel}_{ln}"])
            for p, dn, nn in variants(n_body):
                rec["expected"][(p, dn, nn, sel, ln)] = {
                    f: torch.from_numpy(raw[key(p, dn, nn, sel, ln) + "_" + f])
                    for f in ("input_kp", "target_kp", "target_conf", "n_frames", "text_tokens")}
    rec["selections"] = sels
    return rec


def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(BATCHES, "*.npz")))


def same_bits(a, b):
    """Equal shape, dtype and bit patterns (torch.equal treats -0.0 == 0.0 and NaN != NaN; this does neither)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    view = torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(a.view(view), b.view(view))
