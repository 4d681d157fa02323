#!/usr/bin/env python3
"""Per-kernel resources of every assembly and gradient translation unit as the compiler reports them (no GPU needed), in
the listing format of tools/kprod_resources.py, whose parser this reuses.

    python tools/deriv_resources.py [--csrc DIR] [--out listing.txt] [--against other_listing.txt]

--csrc: another checkout's stheno.jl_amd/csrc (the parent commit's, say).  Sources it does not have are skipped, so a
parent without deriv.hip lists what it has.  --against: every kernel of that earlier listing must be here with the same
figures; exit status 1 if any differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kprod_resources as kr  # noqa: E402



def listing(source):
    """kprod_resources.listing for any source: kernels of anonymous namespaces keep their names ("{anon}::name"), and a
    remark block without a function name is skipped"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                            "-c", source, "-o", os.path.join(tmp, "unit.o")], capture_output=True, text=True, check=True)
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = name.replace("(anonymous namespace)", "{anon}").split("(")[0].strip()
            if cur:
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+)", line)
        if m and cur and m.group(1).strip() in kr.KEYS:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


SOURCES = ("kernelmatrix.hip", "grad.hip", "conv.hip", "stencil.hip", "kprod.hip", "predgrad.hip", "deriv.hip")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(kr.ROOT, "stheno.jl_amd", "csrc"))
    ap.add_argument("--out")
    ap.add_argument("--against")
    a = ap.parse_args()
    rows = {}
    for name in SOURCES:
        path = os.path.join(a.csrc, name)
        if os.path.exists(path):
            rows.update(listing(path))
    if a.out:
        with open(a.out, "w") as fh:
            kr.write(rows, fh)
    else:
        kr.write(rows, sys.stdout)
    if a.against:
        old = kr.read(a.against)
        # (kr.read spells boolean template arguments 1 / 0; this compiler's demangler prints true / false)
        rows = {re.sub(r"\btrue\b", "1", re.sub(r"\bfalse\b", "0", n)): v for n, v in rows.items()}
        bad = [n for n in old if rows.get(n) != old[n]]
        for n in bad:
            print("DIFFERS", n, old[n], rows.get(n), file=sys.stderr)
        print(f"{len(old)} kernels of {a.against}: {len(old) - len(bad)} unchanged, {len(bad)} differ; "
              f"{len(set(rows) - set(old))} new", file=sys.stderr)
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
