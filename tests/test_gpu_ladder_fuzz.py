"""Random operation walks over handles with a temperature ladder, on the device against the composed host twins (tests/ladder_fuzz.py):
random R, ladders, pools, potentials, state and parameter types, offsets up to and across chain id 2^32, geometric / random / equal
beta, planted non-finite positions; then a walk over sweeps in every launch form (sliced single-sweep launches included), exchange
steps, widths per rung set, rewritten and cleared behind queued sweeps, tracking on and off, uploaded labels, gap counters and Move
counters, exchange step indices up to 2^48, another ladder in the middle -- and the observers in between: state, counters, labels,
flow, trips, per-rung sums, histograms and counter totals, the callback records.  Everything bit for bit or integer for integer.

The same walk draws the ladder tools among them, so that they meet on one handle in an order nobody wrote down: bridge snapshots
under a drawn mask, reset and put back; respacings by acceptance and by flow, with the handle's own counts and with explicit global
ones, taken and not; tunings with their window restarted, its base set and Move counters uploaded behind it; marks, samples and
set_corr; partitions of 2 to 64 blocks at chunks of 0, 1, 5 and every ladder; upload_state in the middle; the calls that must be
refused with AMC_ERR_STATE -- observed through the ladder, the two status records and the table, the window, the bridge and
correlation records word for word, merged and per block (whose merge must be the merged fetch).  What each call zeroes, keeps or
refuses is the text of include/amc.h, held in ladder_fuzz.LadderReference.

The pinned cases (ladder_fuzz.PINNED) come first; AMC_LADDER_FUZZ_CASES (default 40 drawn cases) and AMC_LADDER_FUZZ_SEED widen or
move the sample.  Measured on an MI355X, one box, one session: the file at its defaults (10 pinned + 40 drawn cases) takes 20.0 s
the first time and 4.8 s run again at once (the Float32-state kernels are compiled at run time and kept: the difference is theirs);
300 drawn cases of another seed take 39.0 s.  The file as it was before the ladder tools (6 pinned + 40 drawn cases; 16.3 s on
record) takes 6.6 s in that same warm state: the twins' extra Python is not what the time goes to, the slowest single walk is 3.2 s.
Custom (run-time compiled) potentials stay out: each costs seconds of compile time, and the exchange files cover them.
"""
import os
import re

import numpy as np
import pytest

import ladder_fuzz as LF

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("AMC_LADDER_FUZZ_CASES", str(LF.DEFAULT_CASES)))
SEED = int(os.environ.get("AMC_LADDER_FUZZ_SEED", str(LF.DEFAULT_SEED)))


def slice_lines(err):
    return re.findall(r"\[amc\] sweep slice (\d+) of (\d+): pairs from (\d+), (\d+) chains in a grid of (\d+) blocks", err)


def walk_on_the_device(gpu, capfd, case):
    """Sliced-route cases: every sweep_launches(n >= 2) call takes the slices test_gpu_sliced_launches.expected_slices counts -- all
    of them on 256-pair boundaries, together the whole shard -- where the handle's kernels are the offline ones; a Float32-state
    handle compiles its kernels at run time and stays whole."""
    M, S = case["n_chains"], case["slices"]
    want = LF.expected_slices(M, S) if S and case["dtype"] == "f64" else 1

    def after_op(op):
        if not S or op[0] != "launches":
            return
        took = slice_lines(capfd.readouterr().err)
        n = want if op[1] >= 2 and want > 1 else 0
        assert len(took) == n, (op, took, case)
        if took:
            assert sum(int(t[3]) for t in took) == M and [int(t[2]) % 256 for t in took] == [0] * n, (took, case)

    if S:
        capfd.readouterr()
    return LF.run_case(gpu.HipEngine, case, after_op=after_op)


@pytest.mark.parametrize("index", range(len(LF.PINNED)))
def test_pinned_case(gpu, oracle, capfd, index):
    walk_on_the_device(gpu, capfd, dict(LF.PINNED[index]))


@pytest.mark.parametrize("index", range(N_CASES))
def test_random_ladder_random_operations(gpu, oracle, capfd, index):
    walk_on_the_device(gpu, capfd, LF.draw_case(np.random.default_rng([SEED, index])))
