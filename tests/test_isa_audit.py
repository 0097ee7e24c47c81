"""Static checks of the compiled gfx950 kernels (no GPU needed), from the one compile of b2h_api.hip with
--save-temps and hipcc's resource-usage remarks that tests/kernel_remarks.py makes per pytest process:
* no buffer/global store may have its data registers rewritten within two wait states
  (tools/store_war_audit.py) -- the store-data write-after-read hazard that produced wrong frames in
  the fused 16-bit kernel;
* no kernel may spill or use scratch, and each must reach the occupancy its launch bound promises -- a
  refactor once left the wide 16-bit kernel with 24 spilled VGPRs and serialised weight loads (-22 %),
  visible only in a width sweep on the GPU."""
import os
import subprocess
import sys

import pytest

from kernel_remarks import kernel_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def compiled():
    kernels, listing = kernel_remarks()
    return listing, kernels


def test_no_close_store_data_overwrite(compiled):
    a = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "store_war_audit.py"), compiled[0], "2"],
                       capture_output=True, text=True, timeout=300)
    assert a.returncode == 0, a.stderr
    assert a.stdout.strip().splitlines()[-1] == "total 0", a.stdout


def test_no_kernel_spills_and_promised_occupancy(compiled):
    kernels = compiled[1]
    conv = {n: r for n, r in kernels.items() if "b2h_fwd" in n or "b2h_tenc_chain" in n or "b2h_attn" in n}
    assert len(conv) >= 25, sorted(kernels)             # every instantiation of every kernel family was seen
    for name, r in conv.items():
        assert r["ScratchSize [bytes/lane]"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", (name, r)
    # launch bounds -> waves per SIMD the design counts on
    want = {"b2h_fwd_mfma16I": 2, "b2h_fwd_mfma16wI": 2, "b2h_fwd_mfma_f16x3I": 2, "b2h_fwd_mfma_f16x3wI": 1, "b2h_tenc_chainI": 2}
    for name, r in conv.items():
        for key, occ in want.items():
            if key in name:
                assert int(r["Occupancy [waves/SIMD]"]) >= occ, (name, r)


def test_audit_detects_the_pattern(tmp_path):
    """The audit on synthetic listings: the exact sequence that broke the fused kernel is reported,
    padded / branch-separated / MFMA-late-writer variants are handled as documented."""
    audit = os.path.join(ROOT, "tools", "store_war_audit.py")

    def total(body, window="2"):
        f = tmp_path / "k.s"
        f.write_text("_Z1kv:\n" + body + "\n\ts_endpgm\n")
        r = subprocess.run([sys.executable, audit, str(f), window], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return int(r.stdout.strip().splitlines()[-1].split()[1])

    bad = "\tbuffer_store_dwordx4 v[106:109], v226, s[36:39], s93 offen\n\tv_pk_mul_f32 v[106:107], v[186:187], v[100:101]"
    assert total(bad) == 1
    assert total(bad.replace("v_pk_mul_f32 v[106:107]", "v_pk_mul_f32 v[110:111]")) == 0          # other registers
    assert total(bad.replace("offen\n", "offen\n\ts_nop 3\n")) == 0                             # padded
    assert total(bad.replace("offen\n", "offen\n.LBB0_1:\n")) == 0                              # new basic block
    assert total("\tglobal_store_dwordx4 v[0:1], v[142:145], off\n\tv_mov_b32_e32 v143, v7") == 1
    assert total("\tbuffer_store_dwordx2 v[114:115], v116, s[8:11], 0 offen\n\tv_cndmask_b32_e32 v114, v74, v118, vcc") == 1


# ---- the dynamic claim's destination register (kernel_mfma16.h, Sched16) ---------------------------------------
# The device-wide claim is an inline-asm `global_atomic_add vD, ... sc0` whose answer lands in vD asynchronously; the
# compiler does not track that write (inline asm is opaque to its wait-count insertion).  The kernel is correct only
# while nothing reads or writes vD before the `s_waitcnt vmcnt(0)` of pin_loads16: a copy or a live-range split of
# `pv` there would read a stale claim and skip or repeat chunks.
_CLAIM_KERNEL = "_ZN3b2h14b2h_fwd_mfma16I"


def _vregs(text):
    """VGPR numbers an operand string names, single registers and v[a:b] ranges."""
    import re
    regs = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        regs.update(range(int(a), int(b) + 1))
    regs.update(int(r) for r in re.findall(r"\bv(\d+)\b", text))
    return regs


def claim_register_violations(listing):
    """(claims, done_counts, violations) over every b2h_fwd_mfma16 instantiation of an assembly listing: each
    returning global_atomic_add's destination must be untouched until the next s_waitcnt with vmcnt(0)."""
    import re
    claims = done = 0
    bad = []
    kernel = None
    lines = listing.splitlines()
    for i, raw in enumerate(lines):
        line = raw.split(";", 1)[0].rstrip()
        label = re.match(r"^(_Z\w+):", line)
        if label:
            kernel = label.group(1) if label.group(1).startswith(_CLAIM_KERNEL) else None
            continue
        if kernel is None:
            continue
        m = re.match(r"^\s*global_atomic_add\s+v(\d+),(.*)\bsc0\b", line)
        if not m:
            continue
        vd = int(m.group(1))
        if "offset:" in m.group(2):
            done += 1
        else:
            claims += 1
        for j in range(i + 1, len(lines)):
            nxt = lines[j].split(";", 1)[0].strip()
            if re.match(r"^s_waitcnt\b.*\bvmcnt\(0\)", nxt):
                break
            if re.match(r"^(_Z\w+:|s_endpgm\b)", nxt):
                bad.append((kernel, i + 1, "no vmcnt(0) before the end of the kernel"))
                break
            if not nxt or nxt.endswith(":") or nxt.startswith("."):
                continue
            parts = nxt.split(None, 1)
            if len(parts) == 2 and vd in _vregs(parts[1]):
                bad.append((kernel, j + 1, f"v{vd} used before the wait: {nxt}"))
    return claims, done, bad


def test_claim_register_untouched_until_the_wait(compiled):
    with open(compiled[0]) as f:
        claims, done, bad = claim_register_violations(f.read())
    assert claims == 8, claims        # one claim per b2h_fwd_mfma16<PREC, FUSED, STREAM>: the check is not vacuous
    assert done == 8, done            # and one finished-workgroup count (offset:4) each
    assert not bad, bad


def test_claim_register_audit_detects_uses():
    """The claim audit on synthetic listings: a copy or an overwrite of the destination before the wait is
    reported, a read after it is not."""
    head = "_ZN3b2h14b2h_fwd_mfma16ILi1ELb0ELb1EEEvPKfPfiiilPKviNS_9FusedArgsENS_7Sched16E:\n"
    atomic = "\tglobal_atomic_add v202, v2, v6, s[10:11] sc0\n\tv_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]\n"
    wait = "\ts_waitcnt vmcnt(0)\n"
    tail = "\tv_readfirstlane_b32 s0, v202\n\ts_endpgm\n"

    def audit(body):
        return claim_register_violations(head + body)

    assert audit(atomic + wait + tail) == (1, 0, [])                                  # read after the wait: fine
    assert len(audit(atomic + "\tv_mov_b32_e32 v5, v202\n" + wait + tail)[2]) == 1    # copied before the wait
    assert len(audit(atomic + "\tv_add_u32_e32 v202, 1, v3\n" + wait + tail)[2]) == 1  # overwritten before the wait
    assert len(audit(atomic + "\tv_pk_mov_b32 v[201:202], v[8:9], v[8:9] op_sel:[0,1]\n" + wait + tail)[2]) == 1
    assert len(audit(atomic + "\ts_waitcnt vmcnt(3)\n\tv_mov_b32_e32 v5, v202\n" + wait + tail)[2]) == 1
    assert audit(atomic + "\ts_waitcnt vmcnt(0) lgkmcnt(0)\n" + tail)[2] == []
    assert audit(atomic + "\tv_mov_b32_e32 v5, v2020\n" + wait + tail)[2] == []
    # the finished-workgroup count (offset:4) obeys the same rule
    done = "\tglobal_atomic_add v1, v1, v2, s[10:11] offset:4 sc0\n.LBB13_105:\n\ts_or_b64 exec, exec, s[0:1]\n"
    assert audit(done + wait + "\tv_readfirstlane_b32 s0, v1\n\ts_endpgm\n") == (0, 1, [])
    assert len(audit(done + "\tv_mov_b32_e32 v0, v1\n" + wait + "\ts_endpgm\n")[2]) == 1
    # other kernels are not audited (their atomics are waited for by the compiler)
    assert claim_register_violations("_Z5otherv:\n" + atomic + "\tv_mov_b32_e32 v5, v202\n" + wait) == (0, 0, [])
