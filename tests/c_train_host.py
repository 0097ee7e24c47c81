"""Helpers for the C host that trains (examples/c_abi_train_host.cpp): compile it against libb2h, write its input file
from a trajectory fixture, read its output.  A helper module, not a conftest.py: the tests import it by name."""
import os
import shutil
import subprocess

import numpy as np

from conftest import ROOT
from hand_pose_sl_amd import build as b2h_build
from train_ref import KEYS

SRC = os.path.join(ROOT, "examples", "c_abi_train_host.cpp")
EXE = os.path.join(ROOT, "examples", "c_abi_train_host")


def compile_host():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lib = b2h_build.build()
    libdir = os.path.dirname(lib)
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(lib)):
        subprocess.check_call([hipcc, "-O2", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-o", EXE, SRC, "-L" + libdir, "-lb2h", "-Wl,-rpath," + libdir])
    return EXE


def write_input(path, rec):
    """`rec`: a trajectory fixture of train_ref.load_train (state, x, target, lengths, lr, steps)."""
    with open(path, "wb") as f:
        np.array([rec["C"], int(rec["pos_emb"]), rec["B"], rec["T"], int(rec["steps"])], dtype=np.int32).tofile(f)
        np.array([float(rec["lr"])], dtype=np.float32).tofile(f)
        for k in KEYS:
            np.ascontiguousarray(rec["state"][k], dtype=np.float32).tofile(f)
        np.ascontiguousarray(rec["x"], dtype=np.float32).tofile(f)
        np.ascontiguousarray(rec["target"], dtype=np.float32).tofile(f)
        np.ascontiguousarray(rec["lengths"], dtype=np.int64).tofile(f)


def read_output(path, rec):
    """(losses, {key: final tensor}) as the program wrote them."""
    out = np.fromfile(path, dtype=np.float32)
    steps = int(rec["steps"])
    losses, rest, final = out[:steps], out[steps:], {}
    for k in KEYS:
        n = rec["state"][k].size
        final[k], rest = rest[:n].reshape(rec["state"][k].shape), rest[n:]
    assert rest.size == 0
    return losses, final
