"""The pointer-alignment audit without a GPU: the kernel the audit added compiles without scratch or spills, the table
of DESIGN.md has a row for every entry point include/b2h.h declares with a device pointer, and every row's verdict is
"access <= promise".  (tests/test_alignment_gpu.py runs every entry point at the weak alignments.)"""
import os
import re

from kernel_remarks import ROOT, kernel_remarks


def test_new_kernel_has_no_scratch_or_spills():
    kernels, _ = kernel_remarks()
    new = {n: r for n, r in kernels.items() if "b2h_embed_dwords" in n}
    assert len(new) == 1, sorted(new)
    for name, res in new.items():
        assert res["ScratchSize [bytes/lane]"] == "0" and res["VGPRs Spill"] == "0" and res["SGPRs Spill"] == "0", (name, res)


def _table():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    start = text.index("### Pointer alignment: promise and widest access")
    end = text.find("\n## ", start)
    rows = [line for line in text[start:end if end > 0 else None].splitlines() if line.startswith("| `b2h_")]
    return [[c.strip() for c in line.strip().strip("|").split("|")] for line in rows]


def test_every_row_of_the_table_reads_access_within_promise():
    rows = _table()
    assert len(rows) >= 40
    for r in rows:
        assert len(r) == 6, r
        assert r[5].startswith("access ≤ promise"), r


def test_the_table_covers_every_entry_point_that_takes_a_device_pointer():
    header = open(os.path.join(ROOT, "include", "b2h.h")).read()
    declared = set(re.findall(r"^int (b2h_\w+)\(", header, re.M))
    # no device pointer, or none the caller aligns: life cycle, switches, sizes, introspection, the timing wrapper of
    # b2h_forward (same checks, same kernel)
    without = {"b2h_version", "b2h_build_flags", "b2h_device_count", "b2h_create", "b2h_destroy", "b2h_tenc_create",
               "b2h_tenc_destroy", "b2h_tenc_set_kernel", "b2h_tpt_create", "b2h_tpt_destroy", "b2h_tpt_set_kernel",
               "b2h_tpt_info", "b2h_tpt_set_train_kernel", "b2h_tpt_set_train_linear", "b2h_tenc_set_train_kernel",
               "b2h_tenc_set_train_linear", "b2h_model_info", "b2h_kernel_supported", "b2h_time_forward", "b2h_stream_sync"}
    assert without <= declared
    covered = set()
    for r in _table():
        covered |= set(re.findall(r"b2h_\w+", r[0]))
    assert declared - without <= covered, sorted(declared - without - covered)
