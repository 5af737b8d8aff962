#!/usr/bin/env python3
"""Per-kernel register / scratch / LDS table of two builds, side by side.

Input: the stderr of `hipcc <the Makefile's flags> -Rpass-analysis=kernel-resource-usage -c FILE.hip` for the parent
commit and for this tree (one pair of logs per source file).

    python profiles/resource_table.py parent_conv_gemm.log:new_conv_gemm.log parent_wgrad.log:new_wgrad.log

Prints one row per kernel (old -> new where a figure moved) and the list of rows in which Occupancy, ScratchSize,
a spill count or the LDS size differs; exit status 1 if there is any such row."""
import re
import subprocess
import sys

KEYS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "VGPRs Spill", "SGPRs Spill", "LDS Size"]
MUST_MATCH = ["ScratchSize", "Occupancy", "VGPRs Spill", "SGPRs Spill", "LDS Size"]


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None and k in KEYS:
            cur[k] = int(v)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(anonymous namespace\)::|\(.*$", "", d) for n, d in zip(names, r)}


bad = []
for pair in sys.argv[1:]:
    old, new = (parse(p) for p in pair.split(":"))
    pretty = demangle(sorted(set(old) | set(new)))
    print(f"== {pair}: {len(old)} kernels in the parent, {len(new)} in this tree")
    print(f"{'kernel':<72}" + "".join(f"{k:>14}" for k in KEYS))
    for name in sorted(pretty, key=pretty.get):
        o, n = old.get(name), new.get(name)
        if o is None or n is None:
            print(f"{pretty[name]:<72}  only in the {'parent' if n is None else 'new'} build")
            bad.append(pretty[name])
            continue
        cells = [str(o[k]) if o[k] == n[k] else f"{o[k]}->{n[k]}" for k in KEYS]
        print(f"{pretty[name]:<72}" + "".join(f"{c:>14}" for c in cells))
        if any(o[k] != n[k] for k in MUST_MATCH):
            bad.append(pretty[name])
print("rows that differ in " + ", ".join(MUST_MATCH) + ": " + (", ".join(bad) if bad else "none"))
sys.exit(1 if bad else 0)
