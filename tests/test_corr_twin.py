"""The host twin of the time correlation (tests/corr_twin.py) against plain numpy, and the tau_int estimator
(montecarlo_amd.correlation.rho_from_records / tau_from_rho) against a process with a known answer.  No GPU."""
import math

import numpy as np
import pytest

import montecarlo_amd as ma

import corr_twin as T

M_SMALL = 4096
G = 4


@pytest.fixture(scope="module")
def ensemble(oracle):
    """Gaussian positions at a mark and at two later times (correlated with the mark), and the twin's records of the energy."""
    rng = np.random.default_rng(2024)
    x0 = rng.normal(0.0, 0.7, M_SMALL)
    xs = [x0, 0.8 * x0 + 0.6 * rng.normal(0.0, 0.7, M_SMALL), rng.normal(0.0, 0.7, M_SMALL)]
    series = [T.observable("energy", "harmonic", x) for x in xs]
    return xs, series, T.records(series, G)


def test_rounded_sums_equal_fsum_of_the_same_summands(ensemble):
    xs, series, rec = ensemble
    assert rec.shape == (3, G, 3, T.WORDS)
    val = T.values(rec)
    a = (xs[0] * xs[0]).reshape(-1, G)
    for s, x in enumerate(xs):
        o = (x * x).reshape(-1, G)                     # the harmonic energy: one IEEE multiplication
        for g in range(G):
            for c, col in enumerate((o[:, g], o[:, g] * o[:, g], a[:, g] * o[:, g])):
                want = math.fsum(col)
                assert val[s, g, c] == pytest.approx(want, rel=1e-12), (s, g, c, val[s, g, c], want)


def test_slot_zero_holds_the_origin_moments(ensemble):
    _, series, rec = ensemble
    assert np.array_equal(rec[0, :, 1], rec[0, :, 2])            # OO and AO of sample 0: the same summands


def test_observable_x_and_one_group(oracle):
    x = np.random.default_rng(5).normal(size=257)
    rec = T.records([T.observable("x", "harmonic", x), T.observable("x", "harmonic", -x)], 1)
    val = T.values(rec)
    assert val[1, 0, 0] == pytest.approx(-math.fsum(x), rel=1e-12) and val[1, 0, 2] == pytest.approx(-math.fsum(x * x), rel=1e-12)


def test_merging_split_ensembles_gives_the_bits_of_the_whole(ensemble):
    _, series, rec = ensemble
    for cut in (G, M_SMALL // 2, M_SMALL - 3 * G):                # whole ladders on either side, as shards hold them
        parts = [T.records([s[:cut] for s in series], G), T.records([s[cut:] for s in series], G)]
        assert np.array_equal(T.merge(parts).view(np.uint64), rec.view(np.uint64)), cut


def test_a_nan_flags_its_own_records_only(oracle):
    a = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    o = np.array([1.0, np.nan, 3.0, 4.0, 5.0, 6.0])
    clean = T.sample_records(a, a, 2)
    rec = T.sample_records(a, o, 2)
    assert np.array_equal(rec[0].view(np.uint64), T.sample_records(a[0::2], o[0::2], 1)[0].view(np.uint64))
    assert np.all(np.isnan(T.values(rec[1]))) and np.all(np.isfinite(T.values(rec[0])))
    origin_nan = T.sample_records(o, a, 2)                         # a NaN origin value with a finite later value: AO alone
    v = T.values(origin_nan)
    assert np.isnan(v[1, 2]) and np.isfinite(v[1, 0]) and np.isfinite(v[1, 1])
    assert np.array_equal(origin_nan[0].view(np.uint64), clean[0].view(np.uint64))


# ---- the estimator: AR(1), o_(k+1) = phi o_k + sqrt(1 - phi^2) xi from a stationary start, tau_exact = (1 + phi) / (2 (1 - phi)) ------------
M_AR, N_LAGS = 1 << 18, 80


def ar1_records(phi, n_lags, seed):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=M_AR)
    series = [o]
    for _ in range(n_lags):
        o = phi * o + math.sqrt(1.0 - phi * phi) * rng.normal(size=M_AR)
        series.append(o)
    return T.records(series, 1)


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_tau_int_of_ar1(oracle, amc, phi):
    rec = ar1_records(phi, N_LAGS, 11)
    rho = ma.rho_from_records(rec, M_AR)
    assert rho.shape == (1, N_LAGS + 1) and rho[0, 0] == pytest.approx(1.0, abs=1e-12)
    tau, window, converged = ma.tau_from_rho(rho)
    W = int(window[0])
    exact = (1.0 + phi) / (2.0 * (1.0 - phi))
    # per-lag sampling error of a correlation coefficient, at most 1 / sqrt(M), five of them per lag, added over the W lags without
    # assuming independence; plus the exact truncated tail sum_{k > W} phi^k
    tol = 5.0 * W / math.sqrt(M_AR) + phi ** (W + 1) / (1.0 - phi)
    print("phi", phi, "tau", tau[0], "exact", exact, "window", W, "tolerance", tol)
    assert converged[0] and abs(tau[0] - exact) <= tol
    if phi == 0.0:
        assert W <= 3


def test_a_window_longer_than_the_lags_is_not_converged(oracle, amc):
    rec = ar1_records(0.9, 10, 12)
    tau, window, converged = ma.tau_from_rho(ma.rho_from_records(rec, M_AR))
    assert not converged[0] and window[0] == 10 and tau[0] == pytest.approx(0.5 + sum(0.9 ** k for k in range(1, 11)), abs=0.1)
