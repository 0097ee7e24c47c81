#!/usr/bin/env python3
"""Per-launch times of the whole-matrix training attention kernels by shape, from a rocprofv3 kernel trace of
TextPoseTransformer training steps at T <= 128.
The stats table of `rocprofv3 --kernel-trace --stats` has one row per kernel name; a step launches each of
b2h_tt_sdpa(_bwd) / b2h_mw_sdpa(_bwd) at three shapes, and the trace records neither the arguments nor the dynamic LDS.
What tells the shapes apart is the order of a step's launches (b2h_tpt_train_forward / b2h_tpt_backward): forward, the
n_enc encoder layers (S x S), then per decoder layer self (T x T) and cross (T x S); backward, per decoder layer cross
and then self, then the n_enc encoder layers.  This sorts a kernel's dispatches by start time, classifies them by their
position modulo n_enc + 2 n_dec and prints one JSON line per (kernel, shape): launches, mean / min / max microseconds
(DESIGN.md section 30).
    python tools/attn_launch_times.py <kernel_trace.csv> [n_enc=4] [n_dec=4]"""
import csv
import json
import re
import sys

if len(sys.argv) < 2:
    sys.exit(__doc__)
n_enc = int(sys.argv[2]) if len(sys.argv) > 2 else 4
n_dec = int(sys.argv[3]) if len(sys.argv) > 3 else 4
period = n_enc + 2 * n_dec
launches = {}
with open(sys.argv[1], newline="") as f:
    for row in csv.DictReader(f):
        name = re.sub(r"\(.*", "", row["Kernel_Name"]).replace("b2h::", "")
        if name in ("b2h_tt_sdpa", "b2h_tt_sdpa_bwd", "b2h_mw_sdpa", "b2h_mw_sdpa_bwd"):
            launches.setdefault(name, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
for name, spans in sorted(launches.items()):
    if len(spans) % period:
        sys.exit(f"{name}: {len(spans)} launches are no multiple of {period}; give n_enc and n_dec")
    shapes = {}
    for i, (t0, t1) in enumerate(sorted(spans)):
        pos = i % period
        if name.endswith("_bwd"):
            shape = "S x S" if pos >= 2 * n_dec else ("T x S", "T x T")[pos % 2]
        else:
            shape = "S x S" if pos < n_enc else ("T x T", "T x S")[(pos - n_enc) % 2]
        shapes.setdefault(shape, []).append((t1 - t0) / 1e3)
    for shape, us in sorted(shapes.items()):
        print(json.dumps({"kernel": name, "shape": shape, "launches": len(us), "mean_us": round(sum(us) / len(us), 2),
                          "min_us": round(min(us), 2), "max_us": round(max(us), 2)}))
