"""Replica exchange on the device, statistically: every rung keeps its own distribution, and the ladder does what it is for -- it
carries chains across a barrier the coldest rung never crosses on its own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HARMONIC_BETAS = (0.5, 1.0, 2.0, 4.0)
HARMONIC_LADDERS = 65536
HARMONIC_BURN_IN = 16          # sweeps; see test_each_rung_keeps_its_distribution
HARMONIC_ROUNDS = 200

WELL_BETAS = (0.5, 1.0, 2.0, 4.0, 8.0)
WELL_LADDERS = 16384
WELL_ROUNDS = 440              # twice the round of first entry; see test_the_ladder_crosses_the_barrier


def harmonic_engine(gpu):
    R, L = len(HARMONIC_BETAS), HARMONIC_LADDERS
    eng = gpu.HipEngine(n_chains=R * L, potential="harmonic", beta=1.0, sigma=[1.0], weight=[1.0], seed=101, per_chain_counters=False)
    eng.upload_state(np.zeros(R * L), np.tile(HARMONIC_BETAS, L))
    eng.init_uniform(-2.0, 2.0)
    return eng


def harmonic_deviation(eng):
    """Per rung, |<x^2> - 1/(2 beta)| in units of the bound 5 (1/(2 beta)) sqrt(2 / L): five standard errors of the mean of x^2 under
    the exact target N(0, s^2), s^2 = 1/(2 beta), whose Var(x^2) = 2 s^4; ladders are independent."""
    R, L = len(HARMONIC_BETAS), HARMONIC_LADDERS
    x = eng.download_state(want_e=False)[0].reshape(L, R)
    s2 = 1.0 / (2.0 * np.array(HARMONIC_BETAS))
    return np.abs((x * x).mean(axis=0) - s2) / (5.0 * s2 * np.sqrt(2.0 / L))


def test_each_rung_keeps_its_distribution(gpu):
    """Harmonic, R = 4, beta = (0.5, 1, 2, 4), 65 536 ladders, sigma = 1: after the burn-in, 200 rounds of [sweep; exchange] leave
    every rung at its own <x^2> = 1/(2 beta) within five standard errors.  Burn-in: doubled from 16 sweeps until the run WITHOUT
    exchanges (burn-in + 200 sweeps) met the same bound: 16 already did (largest deviation 0.39 of the bound; 32, 64, 128: 0.20,
    0.21, 0.28), so the burn-in is 16 sweeps.  With exchanges the measured deviations were 0.03, 0.28, 0.23, 0.10 of the bound."""
    eng = harmonic_engine(gpu)
    eng.sweep(HARMONIC_BURN_IN)
    eng.set_ladder(len(HARMONIC_BETAS))
    eng.sweep_exchange(HARMONIC_ROUNDS, 1)
    dev = harmonic_deviation(eng)
    acc, att = eng.exchange_counters()
    print("deviation / bound per rung:", dev, "swap acceptance per gap:", acc / att)
    assert np.all(dev <= 1.0), dev
    assert np.all(att == 100 * HARMONIC_LADDERS) and np.all(acc > 0)
    eng.close()


def well_engine(gpu, betas=WELL_BETAS):
    R, L = len(betas), WELL_LADDERS
    eng = gpu.HipEngine(n_chains=R * L, potential="double_well", beta=1.0, sigma=[0.3], weight=[1.0], seed=202, per_chain_counters=False)
    x0 = 0.8 + 0.4 * ((np.arange(R * L) * 0.6180339887498949) % 1.0)          # every chain in the right well
    eng.upload_state(x0, np.tile(betas, L))
    return eng


def cold_left_fraction(eng, R):
    return float((eng.download_strided(R - 1, R, WELL_LADDERS) < 0.0).mean())


def test_the_ladder_crosses_the_barrier(gpu):
    """Double well (x^2 - 1)^2, beta = (0.5, 1, 2, 4, 8), 16 384 ladders, sigma = 0.3, every chain started in the right well.  With an
    exchange step after every sweep the coldest rung (beta = 8) ends with half its chains in each well -- the fraction with x < 0 is
    within 5 sqrt(0.25 / L) of 0.5 --, the same run without exchanges leaves it below 0.1, and every gap's swap acceptance is in
    (0.05, 0.95).  Rounds: the run (bit-equal to the twin at the parity tests' shapes) first entered the band at round 220, looked at
    every 10 rounds (0.4832 against a band of 0.0195; it stayed inside at every look up to round 8000); twice that, 440, is used.  Without
    exchanges the fraction grows by about 8e-5 per sweep (0.363 after 8000 sweeps): 0.03 expected after 440.  Measured swap acceptance
    per gap: 0.86, 0.81, 0.76, 0.76."""
    R, band = len(WELL_BETAS), 5.0 * np.sqrt(0.25 / WELL_LADDERS)
    eng = well_engine(gpu)
    eng.set_ladder(R)
    eng.sweep_exchange(WELL_ROUNDS, 1)
    frac = cold_left_fraction(eng, R)
    acc, att = eng.exchange_counters()
    ratio = acc / att
    eng.close()
    plain = well_engine(gpu)
    plain.sweep(WELL_ROUNDS)
    frac_plain = cold_left_fraction(plain, R)
    plain.close()
    print("fraction left of the barrier, coldest rung:", frac, "without exchanges:", frac_plain, "band:", band, "swap acceptance:", ratio)
    assert abs(frac - 0.5) <= band, (frac, band)
    assert frac_plain < 0.1, frac_plain
    assert np.all((ratio > 0.05) & (ratio < 0.95)), ratio
