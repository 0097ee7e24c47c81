"""hipcc's resource-usage remarks of every gfx950 kernel of b2h_api.hip, and the assembly listing, from ONE compile
per pytest process (about a minute, no GPU needed).  The "no scratch, no spills" tests of the kernel families and
tests/test_isa_audit.py all read this one table; each keeps its own filter, count and assertions."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def kernel_remarks():
    """(kernels: mangled name -> {remark field: value}, path of the gfx950 listing); skips the test without hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tempfile.mkdtemp(prefix="b2h_remarks_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    src = os.path.join(ROOT, "hand_pose_sl_amd", "csrc", "b2h_api.hip")
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-function",
                        "--save-temps", "-Rpass-analysis=kernel-resource-usage", "-o", "x.so", src],
                       cwd=tmp, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    listing = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
    assert listing, os.listdir(tmp)
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: [^ ]*\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = kernels.setdefault(t.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in t:
            k, v = t.rsplit(":", 1)
            cur[k.strip()] = v.strip()
    return kernels, os.path.join(tmp, listing[0])

