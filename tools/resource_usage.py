#!/usr/bin/env python
"""Compiler resource usage of the kernels of one or more csrc files, with the build's own flags (no GPU needed):

    python tools/resource_usage.py [-D...] [--filter REGEX] [--csrc DIR] bn.hip spconv_ws.hip ...

One line per kernel: SGPRs, VGPRs, AGPRs, scratch bytes, occupancy (waves per SIMD), LDS bytes -- the figures of
hipcc -Rpass-analysis=kernel-resource-usage, names demangled."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openscene_amd import build as B  # noqa: E402

FIELDS = [("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "Scratch"),
          ("Occupancy [waves/SIMD]", "Occupancy"), ("LDS Size [bytes/block]", "LDS")]


def usage(src, defines, csrc):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [B.hipcc()] + B.FLAGS + defines + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, src), "-o",
                                                 os.path.join(tmp, "o.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\[[^\]]*\] )?\s*(.*)$", line)
        if not m:
            continue
        t = re.sub(r"\s*\[-Rpass-analysis=[^\]]*\]\s*$", "", m.group(1)).strip()
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            rows.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.rsplit(":", 1)
            cur[k.strip()] = v.strip()
    names = [r_["name"] for r_ in rows]
    if names:
        dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
        for r_, d in zip(rows, dem):
            d = re.sub(r"^void ", "", d)
            d = re.sub(r"\(.*$", "", d).replace("osn::", "")
            r_["name"] = d
    return rows


def main():
    args = sys.argv[1:]
    defines = [a for a in args if a.startswith("-D")]
    flt, csrc, srcs = None, B.CSRC, []
    rest = [a for a in args if not a.startswith("-D")]
    i = 0
    while i < len(rest):
        if rest[i] == "--filter":
            flt = re.compile(rest[i + 1]); i += 2
        elif rest[i] == "--csrc":
            csrc = rest[i + 1]; i += 2
        else:
            srcs.append(rest[i]); i += 1
    print("%-64s %6s %6s %6s %8s %10s %8s" % (("kernel",) + tuple(h for _, h in FIELDS)))
    for src in srcs:
        for r_ in sorted(usage(src, defines, csrc), key=lambda q: q["name"]):
            if flt and not flt.search(r_["name"]):
                continue
            print("%-64s %6s %6s %6s %8s %10s %8s" % ((r_["name"],) + tuple(r_.get(k, "?") for k, _ in FIELDS)))


if __name__ == "__main__":
    main()
