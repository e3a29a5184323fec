"""Kernel resource tables from the compiler's remarks, parent commit against a change (needs no GPU).

Compile the same source at both commits for gfx950 with the build's flags plus
`--cuda-device-only -c -Rpass-analysis=kernel-resource-usage`, keep each compile's stderr, and give the files here:

    python tools/kernel_resources.py --parent parent_remarks.txt --change change_remarks.txt [more_change.txt ...]
                                     --source "rsv_segmented.hip (+ rsv_indexed.hip at the change)" --out resources.tsv

Kernels are matched by their demangled signature; one row per kernel in the format of
profiles/elements_shared/resources.tsv, verdict `same` when every figure agrees, `CHANGED` when one differs, `new` /
`removed` for a kernel only one side has.
"""
from __future__ import annotations

import argparse
import re
import subprocess

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
          "VGPRs Spill", "LDS Size [bytes/block]"]


def parse(paths):
    out, cur = {}, None
    for path in paths:
        for line in open(path):
            m = re.search(r"remark: +(.*?) \[-Rpass-analysis=kernel-resource-usage\]", line)
            if not m:
                continue
            text = m.group(1).strip()
            if text.startswith("Function Name:"):
                cur = out.setdefault(text.split(":", 1)[1].strip(), {})
            elif cur is not None and ":" in text:
                name, value = text.rsplit(":", 1)
                cur[name.strip()] = value.strip()
    return out


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--change", nargs="+", required=True)
    ap.add_argument("--source", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    parent, change = parse(a.parent), parse(a.change)
    names = demangle(sorted(set(parent) | set(change)))
    rows, counts = [], {"same": 0, "CHANGED": 0, "new": 0, "removed": 0}
    for sym in sorted(names, key=lambda s: (s not in parent, names[s])):
        p, c = parent.get(sym), change.get(sym)
        verdict = "new" if p is None else "removed" if c is None else \
            "same" if all(p.get(f) == c.get(f) for f in FIELDS) else "CHANGED"
        counts[verdict] += 1
        cells = [names[sym] if p is not None else "-", names[sym] if c is not None else "-"]
        for f in FIELDS:
            cells += [p.get(f, "-") if p else "-", c.get(f, "-") if c else "-"]
        rows.append("\t".join(cells + [verdict]))
    with open(a.out, "w") as f:
        f.write(f"# {a.source} compiled for gfx950 (-O3, -Rpass-analysis=kernel-resource-usage) at the parent commit and "
                f"with this change; kernels matched by signature; occupancy is the compiler's figure from the register "
                f"counts; {counts['same']} same, {counts['CHANGED']} changed, {counts['new']} new, "
                f"{counts['removed']} removed\n")
        f.write("\t".join(["kernel (parent)", "kernel (change)"] + [f"{x} {side}" for x in FIELDS
                                                                    for side in ("parent", "change")] + ["verdict"]) + "\n")
        f.write("\n".join(rows) + "\n")
    print(counts)


if __name__ == "__main__":
    main()
