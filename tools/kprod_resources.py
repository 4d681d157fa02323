#!/usr/bin/env python3
"""Per-kernel resources of csrc/kprod.hip as the compiler reports them (no GPU needed): VGPRs, AGPRs, SGPRs, scratch,
occupancy and static LDS of every kernel instantiation, from `hipcc -Rpass-analysis=kernel-resource-usage`.

    python tools/kprod_resources.py [--source PATH/kprod.hip] [--out listing.txt] [--against other_listing.txt]

--source: another checkout's kprod.hip (its own headers beside it are used), e.g. the parent commit's, to list what ran before.
--against: compare with a listing written earlier; every kernel of that listing must be here with the same figures
(template arguments `true` / `false` of the older listing are read as 1 / 0: the launch mode was a bool before it had a
third value).  Exit status 1 if any differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]",
        "LDS Size [bytes/block]")


def listing(source):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                            "-c", source, "-o", os.path.join(tmp, "kprod.o")], capture_output=True, text=True, check=True)
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0]
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+)", line)
        if m and cur and m.group(1).strip() in KEYS:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def write(rows, fh):
    fh.write("# kernel | " + " | ".join(KEYS) + "\n")
    for name in sorted(rows):
        fh.write(name + " | " + " | ".join(rows[name].get(k, "?") for k in KEYS) + "\n")


def read(path):
    rows = {}
    for line in open(path):
        if line.startswith("#") or "|" not in line:
            continue
        cells = [c.strip() for c in line.split("|")]
        name = re.sub(r"\btrue\b", "1", re.sub(r"\bfalse\b", "0", cells[0]))
        rows[name] = dict(zip(KEYS, cells[1:]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=os.path.join(ROOT, "stheno.jl_amd", "csrc", "kprod.hip"))
    ap.add_argument("--out")
    ap.add_argument("--against")
    a = ap.parse_args()
    rows = listing(a.source)
    if a.out:
        with open(a.out, "w") as fh:
            write(rows, fh)
    else:
        write(rows, sys.stdout)
    if a.against:
        old = read(a.against)
        bad = [n for n in old if rows.get(n) != old[n]]
        for n in bad:
            print("DIFFERS", n, old[n], rows.get(n), file=sys.stderr)
        print(f"{len(old)} kernels of {a.against}: {len(old) - len(bad)} unchanged, {len(bad)} differ; "
              f"{len(set(rows) - set(old))} new", file=sys.stderr)
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
