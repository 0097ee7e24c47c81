#!/usr/bin/env python3
"""Generate the expected training batches of tests/golden/batches/ from the *reference's* datasets and transforms.

Runs only where the reference is present (the path of make_golden.py).  It loads dataloaders/text_pose_dataset.py and
steps/utils.py by file path, with in-memory stubs for the absent `h5py`, `tokenizers` and `fairseq`, and calls the
reference's own methods on seeded stores:
  h5_store    n_body 8, zero padding: TextPoseH5Dataset.array2item / pad / clip / to_tensor (text_pose_dataset.py:587-649)
              on utterances of 0, 1, 3, 7, 8 and 19 frames;
  json_store  n_body 12, frame-0 padding: select_jsons (:52-68) and FastTextPoseDataset.load_jsons / pad / clip /
              to_tensor (:478-544) on utterances of 1, 3, 7, 8 and 19 OpenPose frames, selection "first" and
              "randomcrop" (the drawn starts are recorded);
then the transform classes of steps/utils.py:180-277 in run.py:83-104's order for every `--predict` choice the body
size allows and each of dif_encoding / normalize on and off, stacked with torch's default collate.  T = 7, S = 5.
Nothing of the reference (source or bytecode) is copied: the .npz files hold data only.

The reference cannot index an empty HDF5 dataset (array2item's reshape((0, 3, -1)) is ambiguous to numpy), so the
empty utterance's item is array2item of one row with every array cut to zero frames; pad, clip and to_tensor then run on
it as on any other.  BuildIndexItem and Build3fingerItem keep no "target_conf"; the fixture records what the issue
defines, the target joints of the item's "right_hand_conf".

    python tests/golden/make_golden_batches.py          # rewrites tests/golden/batches/*.npz
"""
import json
import os
import random
import sys
import types

import numpy as np
import torch
from torch.utils.data import default_collate

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _load, _stub_fairseq, _stub_io_deps  # noqa: E402

OUT = os.path.join(HERE, "batches")
T, S, N_TOKENS = 7, 5, 1000
TARGET = {"right_index": slice(5, 9), "right_3fingers": slice(1, 13)}
FIELDS = ("input_kp", "target_kp", "target_conf", "n_frames", "text_tokens")


def _stub_tokenizers():
    if "tokenizers" not in sys.modules:
        m = types.ModuleType("tokenizers")
        m.Tokenizer = type("Tokenizer", (), {})
        sys.modules["tokenizers"] = m


def transforms(utils, predict, dif, norm):
    """run.py:83-104."""
    ts = []
    if dif:
        ts += [utils.WristDifference(), utils.ChestDifference()]
    if norm:
        ts.append(utils.NormalizeFixedFactor(1280))
    ts.append({"right_index": utils.BuildIndexItem, "right_3fingers": utils.Build3fingerItem,
               "right_hand": utils.BuildRightHandItem}[predict]())
    return ts


def finish(utils, item, predict, dif, norm):
    """The transforms on one to_tensor'ed item, then the five entries a batch keeps."""
    conf = item["right_hand_conf"]
    for t in transforms(utils, predict, dif, norm):
        item = t(item)
    if predict != "right_hand":
        item["target_conf"] = conf[:, TARGET[predict]]
    return {f: item[f] for f in FIELDS}


def save(name, rec, expected):
    for k, b in expected.items():
        for f in FIELDS:
            rec[k + "_" + f] = b[f].numpy()
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **rec)
    print(f"{name}: {len(expected)} batches, {os.path.getsize(path)} bytes")


def h5_store(tpd, utils, seed):
    rng = np.random.default_rng(seed)
    lengths = [0, 1, 3, 7, 8, 19]
    utts = []
    for n in lengths:
        x, y, c = rng.uniform(0, 1280, (n, 50)), rng.uniform(0, 720, (n, 50)), rng.uniform(0, 1, (n, 50))
        utts.append(np.concatenate([x, y, c], axis=1).astype(np.float32))
    tokens = rng.integers(0, N_TOKENS, (len(lengths), S)).astype(np.int64)
    fake = types.SimpleNamespace(max_frames=T)
    H5 = tpd.TextPoseH5Dataset

    def raw_item(u):
        arr = utts[u]
        if arr.shape[0] == 0:       # see the module docstring
            item = {k: v[:0] for k, v in H5.array2item(fake, np.zeros((1, 150), np.float32)).items()}
        else:
            item = H5.array2item(fake, arr.copy())
        item["n_frames"] = min(arr.shape[0], T)     # :661-662
        item = H5.to_tensor(fake, H5.clip(fake, H5.pad(fake, item)))
        item["text_tokens"] = torch.tensor(tokens[u].tolist(), dtype=torch.long)
        return item

    lists = {"a": [0, 1, 2, 3], "b": [4, 5], "c": [5, 3, 3, 1, 0]}
    rec = {"meta": np.array([8, T, S]), "rows": np.concatenate(utts, axis=0),
           "offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), "tokens": tokens}
    expected = {}
    for ln, utt in lists.items():
        rec["utt_" + ln] = np.array(utt, np.int64)
        rec["start_first_" + ln] = np.zeros(len(utt), np.int64)      # the H5 dataset clips to the first T frames
        for dif in (0, 1):
            for norm in (0, 1):
                expected[f"right_hand_d{dif}_n{norm}_first_{ln}"] = default_collate(
                    [finish(utils, raw_item(u), "right_hand", dif, norm) for u in utt])
    save("h5_store", rec, expected)


def json_store(tpd, utils, seed):
    rng = np.random.default_rng(seed)
    lengths = [1, 3, 7, 8, 19]

    def flat(n):
        kp = np.concatenate([rng.uniform(0, 1280, (n, 1)), rng.uniform(0, 720, (n, 1)), rng.uniform(0, 1, (n, 1))], axis=1)
        return [float(round(v, 3)) for v in kp.reshape(-1)]

    frames = [[{"version": 1.3, "people": [{"person_id": [-1], "pose_keypoints_2d": flat(25), "face_keypoints_2d": [],
                                            "hand_left_keypoints_2d": flat(21), "hand_right_keypoints_2d": flat(21)}]}
               for _ in range(n)] for n in lengths]
    tokens = rng.integers(0, N_TOKENS, (len(lengths), S)).astype(np.int64)
    fake = types.SimpleNamespace(max_frames=T)
    FT = tpd.FastTextPoseDataset

    def raw_item(u, sel):
        chosen, start = tpd.select_jsons(frames[u], T, selection_type=sel)
        item = FT.load_jsons(fake, chosen)
        item["n_frames"] = min(len(frames[u]), T)                    # :447
        item = FT.to_tensor(fake, FT.clip(fake, FT.pad(fake, item)))
        del item["json_paths"]
        item["text_tokens"] = torch.tensor(tokens[u].tolist(), dtype=torch.long)
        return item, start

    # the store rows: each frame's 12 body, 21 left-hand and 21 right-hand joints as the reference's load_keypoints
    # returns them, rounded to float32 as to_tensor rounds them, in the layout of include/b2h.h
    rows = []
    for utt in frames:
        for fr in utt:
            r_kp, r_conf, l_kp, l_conf, b_kp, b_conf = tpd.load_keypoints(fr)
            kp = torch.tensor(b_kp + l_kp + r_kp).float().numpy()
            conf = torch.tensor(b_conf + l_conf + r_conf).float().numpy()
            rows.append(np.concatenate([kp[:, 0], kp[:, 1], conf]))
    lists = {"a": [0, 1, 2, 3], "b": [4], "c": [4, 3, 3, 1, 0]}
    rec = {"meta": np.array([12, T, S]), "rows": np.stack(rows).astype(np.float32),
           "offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), "tokens": tokens,
           "frames_json": np.array(json.dumps(frames))}
    expected = {}
    random.seed(seed)
    for sel in ("first", "randomcrop"):
        for ln, utt in lists.items():
            rec["utt_" + ln] = np.array(utt, np.int64)
            # one draw per item, used for every variant of this (selection, list): re-seeding replays it
            state = random.getstate()
            starts = None
            for predict in ("right_hand", "right_index", "right_3fingers"):
                for dif in (0, 1):
                    for norm in (0, 1):
                        random.setstate(state)
                        pairs = [raw_item(u, sel) for u in utt]
                        drawn = [s for _, s in pairs]
                        assert starts is None or starts == drawn
                        starts = drawn
                        expected[f"{predict}_d{dif}_n{norm}_{sel}_{ln}"] = default_collate(
                            [finish(utils, it, predict, dif, norm) for it, _ in pairs])
            rec[f"start_{sel}_{ln}"] = np.array(starts, np.int64)
    save("json_store", rec, expected)


def main():
    _stub_fairseq()
    _stub_io_deps()
    _stub_tokenizers()
    utils = _load(os.path.join(REF, "steps", "utils.py"), "ref_steps_utils")
    tpd = _load(os.path.join(REF, "dataloaders", "text_pose_dataset.py"), "ref_text_pose_dataset")
    h5_store(tpd, utils, 61)
    json_store(tpd, utils, 62)


if __name__ == "__main__":
    main()
