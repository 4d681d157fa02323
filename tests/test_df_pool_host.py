"""The task order of a RAGGED pool of the dataflow factorisation (stheno.jl_amd/csrc/df_pool.h: members of different tile grids
merged by proportional dealing into one id sequence, the table the kernel reads) is integer work that must be exact, and the
kernel's freedom from deadlock rests on one property of it: every member sees its own tasks in its own column-major order, so
every input of a task belongs to a smaller id.  Compiled for the host with g++ (tests/df_pool_host.cpp) for the pools
{(2,1),(2,1),(3,2),(9,8)}, a 16-member ramp, the gradient shapes {(5,2),(7,3),(13,6)} with their border patterns (and with no
tile skipped) and 16 x (33,32): the ids map one to one onto (member, i, j), each member's ids ascend in its own order, a
replay of the kernel's task loop with 1, 2, 7, 256 and 512 simulated workgroups always runs to completion, and equal shapes
reproduce the equal-size batch's round robin id for id."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def test_ragged_order_is_a_merge_of_the_members_orders_and_always_makes_progress():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "df_pool_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "df_pool_host.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    # "pools P replays R equal E bad X"
    assert last[0] == "pools" and int(last[1]) == 5 and int(last[3]) == 25 and int(last[5]) == 32 and int(last[7]) == 0, \
        r.stdout[-500:]
