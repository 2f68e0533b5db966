"""The traversal of the blocked passes on the host (montecarlo_amd/csrc/amc_blocks.h): tests/aux/blocks_plan_host.cpp
enumerates every (launch, HIP block, thread, trip) with the header's own index functions -- what bridge_sums_blocks_kernel and
corr_sums_blocks_kernel walk -- over G in {1, 2, 3, 7, 64}, B in {2, 3, 8, 64}, C in {1, 5, 36, 37}, grids of B, 2B and 7B blocks, 1,
C - 1, C B + 1 and 30 001 ladders, shard offsets that cut a chunk and that put l_global across 2^32, and lane caps of 1, 2 and 3 that
force the launch split.  Every local ladder is visited exactly once, by a HIP block of its own b, inside its launch's range, and no
lane goes over the cap.  A stand-alone program built with -fsanitize=address,undefined: nothing is loaded into this process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "montecarlo_amd", "csrc")


def test_every_ladder_once_by_its_own_block_within_the_cap(tmp_path):
    exe = str(tmp_path / "blocks_plan_host")
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "aux", "blocks_plan_host.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 5000, r.stdout[-500:]
