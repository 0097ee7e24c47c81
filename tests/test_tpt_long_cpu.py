"""The long TextPoseTransformer path without a GPU: b2h_tpt_forward_fused is declared, typed, exported and refuses
a NULL model; the CLI's token staging and its token sources; the Python-side errors of forward_fused; the fixture
of the GPU tests meets the condition its bar rests on."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from tpt_ref import TPT, recipe_model


def test_symbol_declared_typed_exported():
    from hand_pose_sl_amd import _lib
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    assert re.search(r"\bb2h_tpt_forward_fused\s*\(", src), "b2h_tpt_forward_fused not declared in include/b2h.h"
    assert re.search(r"#define\s+B2H_TPT_MAX_FRAMES\s+1024\b", src)
    assert "b2h_tpt_forward_fused" in _lib.SYMBOLS and hasattr(lib, "b2h_tpt_forward_fused")
    assert len(_lib.SYMBOLS["b2h_tpt_forward_fused"][1]) == 13
    assert lib.b2h_version() == 100


def test_refuses_a_null_model():
    from hand_pose_sl_amd import _lib
    lib = _lib.load()
    buf = ctypes.c_void_p(4096)  # never dereferenced: the model is NULL
    assert lib.b2h_tpt_forward_fused(None, buf, buf, buf, 1, 40, 200, 0, 1.0, None, buf, 1 << 20, None) == _lib.ERR_INVALID
    assert lib.b2h_tpt_forward_fused(None, None, None, None, 1, 40, 200, 15, 1280.0, buf, None, 0, None) == _lib.ERR_INVALID


def test_pad_tokens():
    from hand_pose_sl_amd.infer import pad_tokens
    assert pad_tokens([]) == [0] * 40
    ids = list(range(1, 42))
    assert pad_tokens(ids[:39]) == ids[:39] + [0]
    assert pad_tokens(ids[:40]) == ids[:40]
    assert pad_tokens(ids) == ids[:40]
    assert pad_tokens([3, 4], n=3) == [3, 4, 0]


def test_cli_needs_a_token_source(tmp_path):
    from hand_pose_sl_amd import infer
    base = ["--data", str(tmp_path), "--model-checkpoint", str(tmp_path / "m.pth"), "--output-folder", str(tmp_path / "out"),
            "--model", "TextPoseTransformer"]
    with pytest.raises(SystemExit, match="--tokens"):
        infer.main(base)
    with pytest.raises(SystemExit, match="--tokens"):
        infer.main(base + ["--text", "hello"])          # --text needs --tokenizer
    assert not (tmp_path / "out").exists()


def test_forward_fused_python_side_errors():
    model = recipe_model(21, 100, 1, 1)
    tok, body = torch.zeros((2, 5), dtype=torch.int64), torch.zeros((2, 200, 12, 2))
    with pytest.raises(ValueError, match="n_frames"):
        model.forward_fused(tok, body, mask_tail=True)
    with pytest.raises(RuntimeError, match="input_pose"):
        model.forward_fused(tok, body[:, :, :5])
    model.train()                                       # dropout 0.5: inference kernels have none
    with torch.no_grad(), pytest.raises(RuntimeError, match="model.eval"):
        model.forward_fused(tok, body)


def test_fixture_meets_the_condition():
    with np.load(os.path.join(TPT, "long_default_b2_s40_t200.npz")) as d:
        r = {k: d[k] for k in d.files}
    assert os.path.getsize(os.path.join(TPT, "long_default_b2_s40_t200.npz")) <= 1024 * 1024
    assert r["body"].shape == (2, 200, 12, 2) and r["tokens"].shape == (2, 40) and r["body"].max() > 1000
    assert [int(v) for v in r["meta"]] == [2, 40, 200, 1000, 4, 4, 7]
    for key in ("norm", "chest"):
        err = np.abs(r["y32_" + key].astype(np.float64) - r["y64_" + key]).max() / 1280
        assert err <= 3e-6, (key, err)
    n = int(r["n_frames"][1])
    assert (r["y64_chest"][1, n:] == 0).all() and (r["y64_norm"][1, n:] != 0).any()


def test_text_option_uses_the_tokenizer(tmp_path):
    from types import SimpleNamespace
    from tokenizers import Tokenizer
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    from hand_pose_sl_amd import infer
    tk = Tokenizer(WordLevel({"[UNK]": 0, "hello": 5, "world": 9, "sign": 2}, unk_token="[UNK]"))
    tk.pre_tokenizer = Whitespace()
    path = tmp_path / "tokenizer.json"
    tk.save(str(path))
    args = SimpleNamespace(tokens=None, text="hello sign world hello", tokenizer=str(path))
    ids = infer._utterance_tokens(args, ["utt"])
    assert ids == [[5, 2, 9, 5]]
    assert infer.pad_tokens(ids[0]) == [5, 2, 9, 5] + [0] * 36
    # --tokens: a list for one utterance, an object by utterance name for several
    f = tmp_path / "ids.json"
    f.write_text(json.dumps([7, 8]))
    assert infer._utterance_tokens(SimpleNamespace(tokens=str(f), text=None, tokenizer=None), ["a"]) == [[7, 8]]
    f.write_text(json.dumps({"a": [1], "b": [2, 3]}))
    assert infer._utterance_tokens(SimpleNamespace(tokens=str(f), text=None, tokenizer=None), ["b", "a"]) == [[2, 3], [1]]
    with pytest.raises(SystemExit):
        infer._utterance_tokens(SimpleNamespace(tokens=str(f), text=None, tokenizer=None), ["c"])
