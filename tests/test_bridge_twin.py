"""The host twin of the bridge sums (tests/bridge_twin.py; DESIGN.md section 3.13 "Bridge sums") against statistics and against plain
numpy, on the CPU: exact Gaussian samples of the harmonic well U = x^2 at every rung, x ~ N(0, 1 / (2 beta_r)), for which
Z_r = sqrt(pi / beta_r) and log(Z_(r+1) / Z_r) = log(beta_r / beta_(r+1)) / 2."""
import math

import numpy as np
import pytest

import bridge_twin as B

BETAS = np.array([0.5, 1.0, 2.0, 4.0])
L = 8192


def gaussian_ensemble():
    """(x, beta) of L ladders over BETAS, chain l R + r at rung r: x ~ N(0, 1 / (2 beta_r)) from numpy.random.default_rng(7)."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((L, BETAS.size)) / np.sqrt(2.0 * BETAS)
    return x.reshape(-1), np.tile(BETAS, L)


def numpy_summands(x, beta, R):
    """The six columns from numpy and libm alone, shape (L, R) each (unused slots hold zeros)."""
    e = (x * x).reshape(-1, R)
    b = beta.reshape(-1, R)
    wf, wb = np.zeros_like(e), np.zeros_like(e)
    wf[:, :-1] = np.exp(-e[:, :-1] * (b[:, 1:] - b[:, :-1]))
    wb[:, 1:] = np.exp(-e[:, 1:] * (b[:, :-1] - b[:, 1:]))
    return [e, e * e, wf, wb, np.minimum(1.0, wf), np.minimum(1.0, wb)]


def acceptance_estimate_and_error(cols):
    """log mean MF[r] - log mean MB[r + 1] per gap and its standard error by the delta method (independent samples at the two rungs)."""
    mf, mb = cols[4][:, :-1], cols[5][:, 1:]
    n = mf.shape[0]
    est = np.log(mf.mean(axis=0)) - np.log(mb.mean(axis=0))
    se = np.sqrt(mf.var(axis=0, ddof=1) / (n * mf.mean(axis=0) ** 2) + mb.var(axis=0, ddof=1) / (n * mb.mean(axis=0) ** 2))
    return est, se


@pytest.fixture(scope="module")
def ensemble(oracle):
    x, beta = gaussian_ensemble()
    rec = B.records(B.energies("harmonic", x), beta, BETAS.size)
    return x, beta, rec


def test_acceptance_estimate_is_within_five_standard_errors_of_the_exact_ratio(ensemble):
    x, beta, rec = ensemble
    exact = 0.5 * np.log(BETAS[:-1] / BETAS[1:])
    _, se = acceptance_estimate_and_error(numpy_summands(x, beta, BETAS.size))
    got = B.log_z_acceptance(rec)
    z = np.abs(got - exact) / se
    print("acceptance estimate", got, "exact", exact, "standard errors off", z)
    assert got.shape == (BETAS.size - 1,) and np.all(z < 5.0), z


def test_rounded_sums_equal_fsum_of_the_same_summands(ensemble):
    x, beta, rec = ensemble
    R = BETAS.size
    cols = numpy_summands(x, beta, R)
    val = B.values(rec)
    for r in range(R):
        for c in range(B.COLS):
            if B.has_summand(c, r, R):
                want = math.fsum(cols[c][:, r])
                assert val[r, c] == pytest.approx(want, rel=1e-12), (r, c, val[r, c], want)
            else:
                assert not rec[r, c].any()                    # an all-zero record


def test_masks_and_merge(ensemble):
    x, beta, rec = ensemble
    R = BETAS.size
    e = B.energies("harmonic", x)
    only = B.records(e, beta, R, B.ACCEPTANCE_SET)
    for c in range(B.COLS):
        if B.ACCEPTANCE_SET >> c & 1:
            assert np.array_equal(only[:, c], rec[:, c])
        else:
            assert not only[:, c].any()
    half = R * (L // 2)
    parts = [B.records(e[:half], beta[:half], R), B.records(e[half:], beta[half:], R)]
    assert np.array_equal(B.merge(parts), rec)                 # integers: the split into shards (or snapshots) does not matter
    n = float(L)
    assert B.heat_capacity(rec, n, BETAS) == pytest.approx(0.5, abs=0.1)         # (5 standard errors: kurtosis 15, 8192 samples)
    assert B.log_z_ti(rec, n, BETAS).shape == (R - 1,) and B.log_z_exponential(rec, n).shape == (2, R - 1)
