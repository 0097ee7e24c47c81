"""The third opt-in switch of TextPoseTransformer training (b2h_tpt_set_train_whole: the whole-matrix fp32 MFMA attention
pair of kernel_train_attn_whole_mfma.h for every attention of at most 128 x 128; TextPoseTransformer.set_train_whole)
without a GPU: the entry points are declared, typed and exported and answer a NULL model; the Python switch, independent
of the other two; the pair still compiles for gfx950 without scratch, spills or static LDS; and its dynamic LDS, as the
header's own mw_sdpa_lds_bytes computes it on the host, stays within the 160 KB of a workgroup at every Tq != Tk."""
import os
import shutil
import subprocess
import warnings

import pytest

import hand_pose_sl_amd as hps
from conftest import ROOT
from hand_pose_sl_amd import _lib
from kernel_remarks import kernel_remarks

DECLARATIONS = {
    "b2h_tpt_set_train_whole": "int b2h_tpt_set_train_whole(b2h_tpt* m, int kernel);",
    "b2h_tpt_train_enc_attn_name": "const char* b2h_tpt_train_enc_attn_name(const b2h_tpt* m);",
    "b2h_tpt_train_attn_name": "const char* b2h_tpt_train_attn_name(const b2h_tpt* m, int64_t T);",
}
ROUTE = ("b2h_tpt_set_train_kernel", "b2h_tpt_set_train_linear", "b2h_tpt_set_train_whole")


def test_entry_points_declared_typed_exported_and_null_safe():
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    for name, line in DECLARATIONS.items():
        assert line in header, name
        assert name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["b2h_tpt_set_train_whole"] == _lib.SYMBOLS["b2h_tpt_set_train_kernel"]
    assert _lib.SYMBOLS["b2h_tpt_train_enc_attn_name"] == _lib.SYMBOLS["b2h_tpt_train_linear_name"]
    assert "typedef enum b2h_train_kernel { B2H_TRAIN_VALU = 0, B2H_TRAIN_MFMA = 1 } b2h_train_kernel;" in header
    assert _lib.TRAIN_KERNELS == {"valu": 0, "mfma": 1}  # unchanged: one enum, one more switch
    lib = _lib.load()                                   # types every symbol: a missing export raises here
    for kernel in (0, 1, 2, -1):
        assert lib.b2h_tpt_set_train_whole(None, kernel) == _lib.ERR_INVALID
        assert lib.b2h_last_error()
    assert lib.b2h_tpt_train_enc_attn_name(None) is None
    for T in (0, 1, 100, 130):
        assert lib.b2h_tpt_train_attn_name(None, T) is None


def _model():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return hps.TextPoseTransformer(50, 12, 2, 4, 128, 42, 1, 1, dropout=0.1)


def test_python_switch_defaults_validates_and_is_independent():
    m = _model()
    assert (m.train_kernels, m.train_linear, m.train_whole) == ("valu", "valu", "valu")
    for kernels in ("valu", "mfma"):
        for linear in ("valu", "mfma"):
            for whole in ("valu", "mfma"):
                assert m.set_train_kernels(kernels).set_train_linear(linear).set_train_whole(whole) is m
                assert (m.train_kernels, m.train_linear, m.train_whole) == (kernels, linear, whole)
                want = tuple(zip(ROUTE, (_lib.TRAIN_KERNELS[v] for v in (kernels, linear, whole))))
                assert m._train_route() == want and len(want) == 3
    m.set_train_kernels("valu").set_train_linear("mfma")
    for bad in ("MFMA", "", None, 1, "whole"):
        with pytest.raises(ValueError):
            m.set_train_whole(bad)
        assert (m.train_kernels, m.train_linear, m.train_whole) == ("valu", "mfma", "mfma")   # nothing changed
    assert m.set_train_whole("valu") is m and m.train_whole == "valu"
    assert _model().train_whole == "valu"               # a new model does not inherit another's setting
    assert "_choose_train_route" not in vars(hps.TextPoseTransformer)   # the shared validation


def test_transformer_enc_keeps_two_switches():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        m = hps.TransformerEnc(24, 4, 128, 42, 1, dropout=0.1)
    assert m._train_route() == (("b2h_tenc_set_train_kernel", 0), ("b2h_tenc_set_train_linear", 0))
    assert not hasattr(m, "set_train_whole")


def test_graph_trainer_key_names_the_switch():
    import inspect
    from hand_pose_sl_amd import graph_trainer
    assert '"train_whole"' in inspect.getsource(graph_trainer.GraphTrainer._graph_key)


def test_mw_kernels_have_no_scratch_spills_or_static_lds():
    kernels, _ = kernel_remarks()
    pair = {n: r for n, r in kernels.items() if "b2h_mw_" in n}
    assert len(pair) == 2 and all(any(k in n for n in pair) for k in ("b2h_mw_sdpaE", "b2h_mw_sdpa_bwdE")), sorted(pair)
    for name, res in sorted(pair.items()):
        print(name, "VGPRs", res["VGPRs"], "AGPRs", res["AGPRs"], "occupancy", res["Occupancy [waves/SIMD]"])
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)   # dynamic LDS only; the caps are raised at creation


HOST_PROGRAM = r"""
#include <cstdio>
#include "kernel_train_attn_whole_mfma.h"
int main() {
    size_t worst[2] = {0, 0};
    int at[2][2] = {{0, 0}, {0, 0}};
    for (int bwd = 0; bwd < 2; ++bwd)
        for (int tq = 1; tq <= 128; ++tq)
            for (int tk = 1; tk <= 128; ++tk) {
                const size_t n = b2h::mw_sdpa_lds_bytes(tq, tk, bwd != 0);
                // the layout the kernels carve: rows at kMwRow, the matrix at mw_ps(Tk), the mask bytes behind it
                const size_t rows = (size_t)((bwd ? 2 : 0) * b2h::mw_pad(tq) + 2 * b2h::mw_pad(tk)) * b2h::kMwRow;
                const size_t want = 4 * (rows + (size_t)b2h::mw_pad(tq) * b2h::mw_ps(tk)) + (bwd ? (size_t)tq * tk : 0);
                if (n < want || b2h::mw_ps(tk) % 32 != 18 || b2h::mw_ps(tk) < b2h::mw_pad(tk)) return 1;
                if (n >= worst[bwd]) worst[bwd] = n, at[bwd][0] = tq, at[bwd][1] = tk;
            }
    std::printf("%zu %d %d %zu %d %d\n", worst[0], at[0][0], at[0][1], worst[1], at[1][0], at[1][1]);
    return 0;
}
"""


def test_lds_bytes_within_a_workgroup_at_every_tq_tk(tmp_path):
    """mw_sdpa_lds_bytes itself, in a program that runs on the host alone, over all 1 <= Tq, Tk <= 128: never below what the kernels
    carve out of it (Q, dO, K, V rows, the (Tq, Tk) matrix at a pitch of 18 mod 32, the backward's mask bytes) and never
    above the 160 KB a gfx950 workgroup can have."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "mw_lds.hip", tmp_path / "mw_lds"
    src.write_text(HOST_PROGRAM)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-function", "-Wno-pass-failed",
                           "-I" + os.path.join(ROOT, "hand_pose_sl_amd", "csrc"), str(src), "-o", str(exe)], timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r
    fwd, fq, fk, bwd, bq, bk = (int(v) for v in r.stdout.split())
    print(f"largest forward {fwd} B at ({fq}, {fk}), backward {bwd} B at ({bq}, {bk})")
    assert (fq, fk) == (bq, bk) == (128, 128)
    assert fwd == 109568 and bwd == 160768 <= 160 * 1024   # the header's own figures
