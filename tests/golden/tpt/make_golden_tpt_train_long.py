#!/usr/bin/env python3
"""Generate the TextPoseTransformer training fixture at the trainer's default length
(tests/golden/tpt/long_train_e2_d2_b2_s40_t200[.partN].npz) from the *reference* class.

The reference's trainer pads every item to `--max-frames 200` (run.py:28; text_pose_dataset.py:145-162), so its
loop body sees (B, 40) ids and (B, 200, 8 | 12, 2) poses.  This is make_golden_tpt_train.py's recipe, stored keys
and 1000 KiB limit per file at (B, S, T) = (2, 40, 200), 2 + 2 layers, lengths [200, 130], inputs scaled by 1 / 1280,
`small=True`; it runs only where the reference checkout is available.  The name does not start with `train_`: that
prefix is pinned to the two shorter fixtures.

    python tests/golden/tpt/make_golden_tpt_train_long.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_tpt_train as short  # noqa: E402  (the recipe; also puts tests/golden on the path)

LONG_CASE = "long_train_e2_d2_b2_s40_t200"


def main():
    mg = short.mg
    mg._stub_fairseq()
    hpm = mg._load(os.path.join(mg.REF, "models", "HandPoseModels.py"), "ref_HandPoseModels")
    utils = mg._load(os.path.join(mg.REF, "steps", "utils.py"), "ref_steps_utils")
    short.case(utils, hpm.TextPoseTransformer, LONG_CASE, 2, 40, 200, 50, 2, 2, [200, 130], 1.0 / 1280, 502, small=True)


if __name__ == "__main__":
    main()
