"""The kind table of the product path (stheno.jl_amd/csrc/kprod_kinds_table.h: which codes are kinds, their tiers, the
(DMAX class, MN, NK) a launcher picks, the parameter rules and their refusal texts) is host-side work: compiled for the host
with g++ and checked against written-out values in tests/kprod_kinds_host.cpp.  The Python side (lib.py, flatten.py,
kernels.py) keeps its own kind constants: each of them must be a kind of the table, and the table must know no other."""
import os
import subprocess
import tempfile

import pytest

import stheno_jl_amd as P

HERE = os.path.dirname(os.path.abspath(__file__))
KNOWN = set(range(0, 8)) | set(range(10, 15)) | {16, 17, 20, 24, 25, 26}
LIB_KINDS = ["SE", "MATERN12", "MATERN32", "MATERN52", "WHITE", "CONST", "RQ", "LINEAR", "COSINE", "GAMMAEXP", "MATERN_NU", "WIENER",
             "PIECEWISE0", "PIECEWISE1", "PIECEWISE2", "PIECEWISE3", "NEURALNET", "FBM", "EXPONENTIATED"]


@pytest.fixture(scope="module")
def host_run():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "kprod_kinds_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "kprod_kinds_host.cpp"), "-o", exe])
        return subprocess.run([exe], capture_output=True, text=True, timeout=60)


def test_kinds_tiers_launch_modes_and_parameter_rules(host_run):
    assert host_run.returncode == 0, host_run.stdout[-3000:]
    last = host_run.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) > 1500 and int(last[3]) == 0, host_run.stdout[-500:]


def test_the_kind_constants_of_lib_py_are_the_kinds_of_the_table(host_run):
    first = host_run.stdout.splitlines()[0].split()
    assert first[0] == "known"
    known = {int(c) for c in first[1:]}
    assert known == KNOWN
    ours = {name: getattr(P.lib, name) for name in LIB_KINDS}
    assert all(code in known for code in ours.values()), ours
    assert set(ours.values()) == known
    assert P.lib.KIND_MASK == 0xff and P.lib.KIND_TIMES_PREV == 0x100
