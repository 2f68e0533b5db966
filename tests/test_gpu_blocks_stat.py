"""The error bar end to end on the harmonic potential, where log(Z_(r+1) / Z_r) = 1/2 log(beta_r / beta_(r+1)) exactly: 4096 ladders of
R = 4 rungs in B = 32 blocks, one burn-in, a bridge snapshot behind every exchange step for 64 steps.  Every gap of every estimator
lies within 5 jackknife standard errors of the exact value -- with 31 degrees of freedom a correct error bar misses that with a
probability of about 2e-5 per estimate; the seed is fixed --, and the device's (theta, se) are those of jackknife() applied to the
host twin's block records, bit for bit.

The ladder, beta_r = 1.1^r: thermodynamic integration by the trapezoid carries a quadrature bias that the bound has to leave room for.
With <e> = 1 / (2 beta) the trapezoid gives (1 + 1/1.1) / 40 = 0.047727 for the exact 0.047655, a bias of 7e-5, below the standard
errors of 1.3e-4 to 1.8e-4 that the run has.

The seed was checked on the CPU before it was committed: this configuration through the engine double of the host tests
(exchange_twin.TwinEngine, the oracle's sweeps and exchange steps) and blocks_twin gives the figures the device gives, and its worst
|estimate - exact| / se is 1.39 (acceptance), 1.39 (exponential, forward), 1.42 (exponential, backward) and 0.92 (ti): the reference
alone stays inside 5 se with a margin of 3.5."""
import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd.jackknife import block_counts, jackknife

import blocks_twin as K
import bridge_twin as BT

pytestmark = pytest.mark.gpu
R, L, B, C, STEPS = 4, 4096, 32, 64, 64
BETAS = 1.1 ** np.arange(R)


def estimators(n_snapshots):
    def means(v, n):
        return v / (float(n_snapshots) * float(n))
    return {"acceptance": lambda v, n: np.log(v[:-1, 4]) - np.log(v[1:, 5]),
            "exponential forward": lambda v, n: np.log(means(v, n)[:-1, 2]),
            "exponential backward": lambda v, n: -np.log(means(v, n)[1:, 3]),
            "ti": lambda v, n: -0.5 * (means(v, n)[:-1, 0] + means(v, n)[1:, 0]) * (BETAS[1:] - BETAS[:-1])}


def test_every_gap_lies_within_five_standard_errors_and_the_device_matches_the_twin(gpu):
    M = R * L
    rng = np.random.default_rng(20240611)
    beta = np.tile(BETAS, L)
    eng = gpu.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[1.2], weight=[1.0], seed=41)
    eng.upload_state(rng.standard_normal(M) / np.sqrt(beta), beta)
    eng.set_ladder(R)
    eng.sweep_exchange(100, 2)                           # the burn-in
    eng.set_blocks(B, C)
    parts = []
    for _ in range(STEPS):
        eng.sweep(2); eng.exchange(1)
        eng.bridge_accumulate()
        parts.append(K.bridge_records(eng.download_state()[1], beta, R, B, C))
    got, n = eng.bridge_fetch_blocks()
    twin = np.stack([BT.merge([p[b] for p in parts]) for b in range(B)])
    assert n == STEPS and np.array_equal(got.view(np.uint64), twin.view(np.uint64))
    counts = block_counts(L, B, C)
    assert np.array_equal(counts, K.counts(L, B, C)) and counts.sum() == L
    exact = 0.5 * np.log(BETAS[:-1] / BETAS[1:])
    for name, fn in estimators(n).items():
        theta, se = jackknife(got, counts, fn)
        theta_t, se_t = jackknife(twin, counts, fn)
        assert np.array_equal(theta, theta_t) and np.array_equal(se, se_t), name
        print(name, "estimate - exact:", (theta - exact).tolist(), "se:", se.tolist())
        assert np.all(se > 0) and np.all(np.abs(theta - exact) <= 5.0 * se), (name, theta - exact, se)
    eng.close()
