#!/usr/bin/env python3
"""(CPU) Two gfx950 listings of b2h_api.hip (hipcc --save-temps: b2h_api-hip-amdgcn-amd-amdhsa-gfx950.s), kernel by
kernel: is the instruction stream the same once labels are numbered in order of appearance, and are the resources the
compiler reports (VGPRs, AGPRs, SGPRs, scratch, LDS, occupancy) the same.  One row per kernel symbol, a summary first.
    python tools/device_code_diff.py <parent.s> <new.s> [name-substring ...]   (substrings: rows marked `touched`)"""
import hashlib, json, re, sys

RES = {"vgpr": "NumVgprs", "agpr": "NumAgprs", "sgpr": "TotalNumSgprs", "scratch": "ScratchSize", "lds": "LDSByteSize",
       "occupancy": "Occupancy"}


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for name in names:
        body = text[re.search(r"^" + re.escape(name) + r":", text, re.M).start():]
        tail = body[body.index(".Lfunc_end"):][:6000]
        body = body[:body.index(".Lfunc_end")]
        labels, insns = {}, []
        for line in body.split("\n")[1:]:
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") and not line.startswith(".LBB"):
                continue
            line = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), line)
            insns.append(re.sub(r"\s+", " ", line))
        res = {k: int(re.search(r";\s*" + v + r":\s*(\d+)", tail).group(1)) for k, v in RES.items()}
        n = sum(1 for i in insns if not i.endswith(":"))
        out[name] = (n, hashlib.sha256("\n".join(insns).encode()).hexdigest()[:16], res)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    touched = sys.argv[3:]
    rows, differing = [], []
    for name in sorted(set(a) & set(b)):
        same = a[name][1] == b[name][1] and a[name][2] == b[name][2]
        if not same:
            differing.append(name)
        mark = " touched" if any(t in name for t in touched) else ""
        res = json.dumps(a[name][2], sort_keys=True) if a[name][2] == b[name][2] else \
            json.dumps({"parent": a[name][2], "new": b[name][2]}, sort_keys=True)
        rows.append("%-7s %5d %5d insns  sha256 %s %s  %s  %s%s" % ("same" if same else "DIFFERS", a[name][0], b[name][0],
                                                                   a[name][1], b[name][1], res, name, mark))
    print(json.dumps({"kernels_parent": len(a), "kernels_new": len(b), "only_parent": sorted(set(a) - set(b)),
                      "only_new": sorted(set(b) - set(a)), "differing": differing}))
    print("\n".join(rows))


if __name__ == "__main__":
    main()
