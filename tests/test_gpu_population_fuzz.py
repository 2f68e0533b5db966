"""Random operation walks over handles with one shared beta, on the device against the composed host twins
(tests/population_fuzz.py): ensembles of 1 to 3075 chains at the wave, block and prefix-tile edges of the annealing kernels, one to
three moves, both potentials and state types, planted non-finite positions, one dominant chain; then a walk over sweeps in every launch
form, annealing steps (cooling, heating, to the same beta, to a far one), searches for the next beta at 1, 3 and 6 rounds followed by
the step they ask for, families on, off and uploaded, the log drained and put back, the annealing step index set up to 2^47, the shared
beta set, marks, samples and the partition of the jackknife blocks, uploads of state and counters, and the calls the header says are
refused -- with the observers in between: state, counters, the log, beta, the step index, families and their statistics, the
correlation records merged and per block, the callback records.  Everything bit for bit or integer for integer.

The pinned cases (population_fuzz.PINNED) come first; AMC_POPULATION_FUZZ_CASES (default 40 drawn cases) and
AMC_POPULATION_FUZZ_SEED widen or move the sample.  Measured on an MI355X, one box, one session: the file at its defaults (5 pinned
+ 40 drawn cases) takes 8.6 s the first time (the first Float32-state walk alone 3.2 s, against 0.3 s once its kernels exist) and 4.6 s run
again at once; 300 drawn cases of another seed take 7.8 s.  Beside it, in the same session, tests/test_gpu_ladder_fuzz.py as it was
before this file existed (16.3 s on record) takes 6.6 s with its kernels compiled.
Custom (run-time compiled) potentials stay out, as in the ladder walk.
"""
import os

import numpy as np
import pytest

import population_fuzz as PF

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("AMC_POPULATION_FUZZ_CASES", str(PF.DEFAULT_CASES)))
SEED = int(os.environ.get("AMC_POPULATION_FUZZ_SEED", str(PF.DEFAULT_SEED)))


@pytest.mark.parametrize("index", range(len(PF.PINNED)))
def test_pinned_case(gpu, oracle, index):
    PF.run_case(gpu.HipEngine, dict(PF.PINNED[index]))


@pytest.mark.parametrize("index", range(N_CASES))
def test_random_population_random_operations(gpu, oracle, index):
    PF.run_case(gpu.HipEngine, PF.draw_case(np.random.default_rng([SEED, index])))
