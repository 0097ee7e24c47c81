"""Utterance inference on the MI355X path: OpenPose JSON frames in, OpenPose JSON frames out.

The working equivalent of the reference's `infer_utterance.py` (:52-111) + `steps/traintest.py`
`infer_utterance` (:214-300) for `--model Conv --predict right_hand`:

    python -m hand_pose_sl_amd.infer --data <folder of *_keypoints.json> \
        --model-checkpoint best_model.pth --output-folder out/ [--model Conv|TransformerEnc|TextPoseTransformer]
        [--conv-channels 30] [--conv-pos-emb] [--max-frames 200] [--no-normalize] [--dif-encoding]
        [--precision fp32] [--tokens ids.json | --text "..." --tokenizer tokenizer.json]
        [--predict right_hand|right_index|right_3fingers]
        [--all-frames [--batch-size 128] [--overlap K [--blend linear|centre]]]

With `--model Conv` (default) transforms, model and de-normalisation run as ONE fused kernel
(`ConvModel.forward_fused`); with `--model TransformerEnc` (infer_utterance.py:99-101) the item
transforms run inside the transformer path's own first and last kernel
(`TransformerEnc.forward_fused`).  `--model TextPoseTransformer` (the reference's default,
infer_utterance.py:27-28,102-105) is the text-conditioned model: its geometry (n_tokens and the two
layer counts) is read from the checkpoint, the rest is the reference's (12 joints in, 21 out, 4 heads,
128 hidden), and the token ids come from `--tokens FILE` -- JSON, a list of ids for one utterance or an
object mapping each utterance folder's base name to its list -- or from `--text STRING --tokenizer
tokenizer.json` through the `tokenizers` package.  Ids are staged as the reference's dataset stages them
(text_pose_dataset.py:467-470): the first 40, right-padded with id 0 (`pad_tokens`).  At the default
`--max-frames 200` it runs the long-attention kernels (`TextPoseTransformer.forward_fused`).
With `--predict right_index` / `right_3fingers` (TextPoseTransformer only; infer_utterance.py:62-85) the model's input is
the 12 body joints and the right hand without the predicted fingers (29 or 21 joints, built by one HIP kernel,
`TextPoseTransformer.build_item`), its output the 4 or 12 finger joints, and only those joints of each frame's
`hand_right_keypoints_2d` are rewritten.
No torch elementwise kernel runs on any of the three paths.
Several utterances (sub-folders) are batched into one launch.
With `--all-frames` every frame of every utterance is predicted, not only the first `--max-frames`: the utterances
become a device-resident store (`DeviceDataset.from_frames`) and `predict_dataset` runs the model over windows of
`--max-frames` frames that cover it once; `--dif-encoding` is then the trainer's pair of transforms (the hand relative to
the raw wrist, the body to the chest) and the wrist is added back to the prediction.  `--overlap K` makes those
windows overlap by K frames and blends the two predictions of the shared frames (`predict_dataset(overlap=, blend=)`).
"""
import argparse
import glob
import json
import os
import re

import numpy as np
import torch

from . import openpose
from .conv_model import ConvModel
from .padding import check_mask_padding, token_lengths
from .text_pose_transformer import TextPoseTransformer
from .transformer_enc import TransformerEnc

N_TOKENS_PER_UTTERANCE = 40   # text_pose_dataset.py:467-470
# --predict -> (n_joints, nout) of the TextPoseTransformer the reference's inference scripts build for it
# (infer_utterance.py:62-85): 12 body joints, alone or with the 17 / 9 hand joints that are not predicted
PREDICT_GEOMETRY = {"right_hand": (12, 21 * 2), "right_index": (12 + 17, 4 * 2), "right_3fingers": (9 + 12, 12 * 2)}


def pad_tokens(ids, n=N_TOKENS_PER_UTTERANCE):
    """The reference dataset's staging of an utterance's token ids: the first `n`, right-padded with id 0."""
    ids = [int(i) for i in ids][:n]
    return ids + [0] * (n - len(ids))


def predict_utterances(model, utterances, max_frames=200, dif_encoding=False, normalize=True, tokens=None,
                       mask_padding=False):
    """`utterances`: list of frame lists (paths or dicts).  Returns (pred_px (U, max_frames, J, 2)
    numpy in pixel units, list of n_frames), J = 21, or the 4 / 12 finger joints of a composite TextPoseTransformer,
    which also reads the utterances' right hands.  Same staging as the reference's dataset (first
    `max_frames` frames, short utterances padded by repeating frame 0).  `tokens`: for a
    TextPoseTransformer, one list of token ids per utterance (staged with `pad_tokens`).  `mask_padding`
    (TextPoseTransformer only): run with the key-padding masks of the padded ids and frames, as a model trained with
    train_epoch(mask_padding=True) needs."""
    mask_padding = check_mask_padding("predict_utterances()", model, mask_padding)
    items = [openpose.load_utterance(u, max_frames) for u in utterances]
    body = torch.from_numpy(np.stack([it["body_kp"] for it in items]))
    dev = next(model.parameters()).device
    lead, extra = (), {}
    if isinstance(model, TextPoseTransformer):
        if tokens is None or len(tokens) != len(items):
            raise ValueError("a TextPoseTransformer needs `tokens`: one list of token ids per utterance")
        lead = (torch.tensor([pad_tokens(t) for t in tokens], dtype=torch.int64),)
        if model.ninp in (42, 58):   # `--predict right_3fingers` / `right_index`
            extra = {"right_hand": torch.from_numpy(np.stack([it["right_hand_kp"] for it in items])).to(dev)}
        if mask_padding:
            extra.update(text_lengths=token_lengths(lead[0].to(dev)), frame_lengths=[it["n_frames"] for it in items])
    elif tokens is not None:
        raise ValueError("`tokens` is for a TextPoseTransformer")
    with torch.no_grad():   # steps/utils.py:180-210 and traintest.py:270-271 fused into the model's kernels
        pred = model.forward_fused(*lead, body.to(dev), dif_encoding=dif_encoding, normalize=normalize,
                                   denormalize=normalize, mask_tail=False, **extra)
    return pred.cpu().numpy(), [it["n_frames"] for it in items]


def predict_all_frames(model, utterances, max_frames=200, dif_encoding=False, normalize=True, tokens=None,
                       predict="right_hand", batch_size=128, mask_padding=False, overlap=0, blend="linear"):
    """`utterances` as predict_utterances takes them, every frame of each predicted (predict_dataset over windows of
    `max_frames` frames, short utterances padded by repeating frame 0).  Returns one (n_i, J, 2) numpy array per
    utterance in pixel units, J = 21, or the 4 / 12 predicted finger joints; with `dif_encoding` the loader's transforms
    are the trainer's and the prediction gets the raw wrist back.  `mask_padding`, `overlap`, `blend`: predict_dataset's."""
    from .dataset import DeviceDataset, DeviceLoader
    from .predict import predict_dataset
    if isinstance(model, TextPoseTransformer):
        if tokens is None or len(tokens) != len(utterances):
            raise ValueError("a TextPoseTransformer needs `tokens`: one list of token ids per utterance")
        tokens = torch.tensor([pad_tokens(t) for t in tokens], dtype=torch.int64)
    elif tokens is not None:
        raise ValueError("`tokens` is for a TextPoseTransformer")
    ds = DeviceDataset.from_frames(utterances, tokens=tokens, device=next(model.parameters()).device)
    loader = DeviceLoader(ds, batch_size, max_frames, selection="first", predict=predict, dif_encoding=dif_encoding,
                          normalize=normalize, pad="frame0")
    hand = slice(33 + openpose.PREDICT_TARGET_JOINTS[predict].start, 33 + openpose.PREDICT_TARGET_JOINTS[predict].stop)
    out = predict_dataset(model, loader, mask_padding=mask_padding, overlap=overlap, blend=blend)
    return [np.stack([r[:, :54][:, hand], r[:, 54:108][:, hand]], axis=2) for r in out.utterance_rows()]


def _tpt_geometry(state):
    """(n_tokens, n_enc_layers, n_dec_layers) of a TextPoseTransformer checkpoint, from its keys and shapes."""
    def layers(stack):
        idx = [int(m.group(1)) for k in state for m in [re.match(rf"transformer\.{stack}\.layers\.(\d+)\.", k)] if m]
        if not idx:
            raise SystemExit(f"the checkpoint has no transformer.{stack}.layers.* keys: not a TextPoseTransformer")
        return max(idx) + 1
    if "token_embedding.weight" not in state:
        raise SystemExit("the checkpoint has no token_embedding.weight: not a TextPoseTransformer")
    return int(state["token_embedding.weight"].shape[0]), layers("encoder"), layers("decoder")


def _utterance_tokens(args, names):
    """One list of token ids per utterance (base names `names`), from --tokens or --text + --tokenizer."""
    if args.tokens:
        with open(args.tokens) as f:
            data = json.load(f)
        if isinstance(data, dict):
            missing = [n for n in names if n not in data]
            if missing:
                raise SystemExit(f"--tokens {args.tokens} has no entry for utterance(s) {missing}")
            return [data[n] for n in names]
        if len(names) != 1:
            raise SystemExit("--tokens holds one list of ids but there are several utterances: use an object "
                             "mapping each utterance folder's base name to its ids")
        return [data]
    if args.text is not None and args.tokenizer:
        from tokenizers import Tokenizer   # only for this option
        ids = Tokenizer.from_file(args.tokenizer).encode(args.text).ids
        return [ids for _ in names]
    raise SystemExit("--model TextPoseTransformer needs token ids: --tokens FILE (JSON list of ids, or an object "
                     "mapping utterance names to lists), or --text STRING with --tokenizer tokenizer.json")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="folder with one utterance's frame JSONs, a folder with one sub-folder per utterance, or one merged utterance file")
    ap.add_argument("--model-checkpoint", required=True)
    ap.add_argument("--output-folder", required=True)
    ap.add_argument("--model", default="Conv", choices=["Conv", "TransformerEnc", "TextPoseTransformer"])
    ap.add_argument("--conv-channels", type=int, default=30)
    ap.add_argument("--conv-pos-emb", action="store_true")
    ap.add_argument("--max-frames", type=int, default=200)
    ap.add_argument("--no-normalize", dest="normalize", action="store_false")
    ap.add_argument("--dif-encoding", action="store_true")
    ap.add_argument("--precision", default="fp32",
                    help="kernel: fp32 (default, the reference's arithmetic, <= 1.2e-7 vs its CPU forward), f16x3 (fp32-grade, "
                         "3x faster); Conv also f16 (18 G frames/s; 5e-5 on normalised keypoints, <= 1e-3 up to |x| ~ 20) and "
                         "bf16 (same speed; 5e-4 on normalised keypoints but 1.05e-3 at N(0,1): above the 1e-3 gate on "
                         "unnormalised inputs -- use f16 there)")
    ap.add_argument("--tokens", help="TextPoseTransformer: JSON file with the token ids, a list for one utterance or an "
                                     "object mapping each utterance folder's base name to a list")
    ap.add_argument("--text", help="TextPoseTransformer: the utterance's text, tokenised with --tokenizer")
    ap.add_argument("--tokenizer", help="TextPoseTransformer: a `tokenizers` tokenizer.json for --text")
    ap.add_argument("--predict", default="right_hand", choices=sorted(PREDICT_GEOMETRY),
                    help="what the model predicts (infer_utterance.py:62-85): the whole right hand, or -- TextPoseTransformer "
                         "only -- its index finger / three fingers from the body and the rest of the hand")
    ap.add_argument("--all-frames", action="store_true",
                    help="predict and write EVERY frame of every utterance (windows of --max-frames frames over a "
                         "device-resident store), not only the first --max-frames; --dif-encoding then means the trainer's "
                         "pair of transforms (hand minus raw wrist, body minus chest) with the wrist added back to the output")
    ap.add_argument("--batch-size", type=int, default=128, help="--all-frames: windows per model launch (traintest.py:339)")
    ap.add_argument("--overlap", type=int, default=0,
                    help="--all-frames: the windows of an utterance longer than --max-frames overlap by this many frames "
                         "(0 .. max-frames // 2) and the two predictions of those frames are blended (--blend), so no frame "
                         "next to a window boundary is predicted from one side only")
    ap.add_argument("--blend", default="linear", choices=["linear", "centre"],
                    help="--overlap: cross-fade the two windows (linear), or take each frame from the window whose centre is "
                         "nearer (centre)")
    ap.add_argument("--mask-padding", action="store_true",
                    help="TextPoseTransformer, --precision fp32: key-padding masks for the padded token ids and frames; "
                         "required for a checkpoint trained with mask_padding=True, wrong for one trained without")
    args = ap.parse_args(argv)
    if args.predict != "right_hand" and args.model != "TextPoseTransformer":
        # the reference's ConvModel / TransformerEnc hard-code 12 input and 21 output joints (HandPoseModels.py:28,32)
        raise SystemExit(f"--predict {args.predict} needs --model TextPoseTransformer")
    if args.overlap and not args.all_frames:
        raise SystemExit("--overlap needs --all-frames (without it only the first --max-frames frames are predicted, by one window)")
    if not 0 <= args.overlap <= args.max_frames // 2:
        raise SystemExit(f"--overlap must be in 0 .. --max-frames // 2 = {args.max_frames // 2}")
    if args.mask_padding and args.model != "TextPoseTransformer":
        raise SystemExit("--mask-padding needs --model TextPoseTransformer")
    if args.mask_padding and args.precision != "fp32":
        raise SystemExit("--mask-padding runs with --precision fp32 (the f16x3 attention kernels take no key lengths)")
    if args.model == "TextPoseTransformer":
        if not args.tokens and not (args.text is not None and args.tokenizer):
            _utterance_tokens(args, [])   # raises SystemExit with the message
        if args.precision not in ("fp32", "f16x3"):
            raise SystemExit("--model TextPoseTransformer runs with --precision fp32 or f16x3")

    if os.path.isdir(args.output_folder):
        raise Exception("Experiment name " + args.output_folder + " already exists.")  # infer_utterance.py:55-56
    merged = os.path.isfile(args.data)   # one merged utterance file (How2Sign/util_scripts/merge_utt_jsons.py)
    if merged:
        utts = [(args.data, openpose.load_merged_utterance(args.data))]
    else:
        subs = sorted(d for d in glob.glob(os.path.join(args.data, "*")) if os.path.isdir(d))
        folders = subs if subs else [args.data]
        utts = [sorted(glob.glob(os.path.join(f, "*.json"))) for f in folders]
        utts = [(f, u) for f, u in zip(folders, utts) if u]
    if not utts:
        raise SystemExit("no *.json frames under " + args.data)

    state = torch.load(args.model_checkpoint, map_location="cpu", weights_only=True)
    tokens = None
    if args.model == "Conv":
        model = ConvModel(args.conv_channels, "ReLU", pos_emb=args.conv_pos_emb, precision=args.precision)
    elif args.model == "TransformerEnc":  # infer_utterance.py:99-101
        if args.precision not in ("fp32", "f16x3"):
            raise SystemExit("--model TransformerEnc runs with --precision fp32 or f16x3")
        model = TransformerEnc(ninp=12 * 2, nhead=4, nhid=128, nout=21 * 2, nlayers=4, precision=args.precision)
    else:  # infer_utterance.py:102-105; the geometry the reference hard-codes is read from the checkpoint
        n_tokens, n_enc, n_dec = _tpt_geometry(state)
        n_joints, nout = PREDICT_GEOMETRY[args.predict]
        model = TextPoseTransformer(n_tokens=n_tokens, n_joints=n_joints, joints_dim=2, nhead=4, nhid=128, nout=nout,
                                    n_enc_layers=n_enc, n_dec_layers=n_dec).set_precision(args.precision)
        tokens = _utterance_tokens(args, [os.path.basename(os.path.normpath(f)) for f, _ in utts])
    model.load_state_dict(state)
    model = model.to("cuda").eval()
    if args.all_frames:
        pred = predict_all_frames(model, [u for _, u in utts], args.max_frames, args.dif_encoding, args.normalize,
                                  tokens=tokens, predict=args.predict, batch_size=args.batch_size,
                                  mask_padding=args.mask_padding, overlap=args.overlap, blend=args.blend)
        n_frames = [len(p) for p in pred]
    else:
        pred, n_frames = predict_utterances(model, [u for _, u in utts], args.max_frames, args.dif_encoding,
                                            args.normalize, tokens=tokens, mask_padding=args.mask_padding)
    os.mkdir(args.output_folder)
    for (folder, frames), p, n in zip(utts, pred, n_frames):
        if merged:
            openpose.write_merged_predictions(frames[:n], p, os.path.join(args.output_folder, os.path.basename(folder)),
                                              predict=args.predict)
            continue
        out = args.output_folder if len(utts) == 1 else os.path.join(args.output_folder, os.path.basename(folder))
        openpose.write_predictions(frames[:n], p, out, predict=args.predict)
    print(f"wrote {sum(n_frames)} frames of {len(utts)} utterance(s) to {args.output_folder}")


if __name__ == "__main__":
    main()
