"""Which terms of a block pair are plain, patch, stencil and chain terms (stheno.jl_amd/csrc/spec_segments.h: PairSegs,
pair_segments, chain_end, chain_dmax) is host-side work: compiled for the host with g++ and checked against written-out
boundaries in tests/spec_segments_host.cpp -- an empty pair, a pair of each single class, one with all four and one with two
chains of lengths 1 and 3."""
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host_run():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "spec_segments_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "spec_segments_host.cpp"), "-o", exe])
        return subprocess.run([exe], capture_output=True, text=True, timeout=60)


def test_pair_boundaries_and_chains_against_written_out_values(host_run):
    assert host_run.returncode == 0, host_run.stdout[-3000:]
    last = host_run.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) == 60 and int(last[3]) == 0, host_run.stdout[-500:]
