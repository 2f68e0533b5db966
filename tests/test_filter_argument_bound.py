"""The harmonic sweeps' filter argument against the reference-ordered dlogp (CPU; model in filter_argument_model.py).

What amc_model.h claims for a lane inside the guard (y no NaN), with t = y ln 2 and D = the reference-ordered dlogp:
  (b)  |D + beta delta s| <= 2^-53 (6.01 beta m^2 + 2.01 |D|),  m = max(|x|, |xn|), and beta m^2 < 2^29 (1 + 2^-50)
       -- so (b) <= 6.1 2^-24 = 3.7e-7 for |D| <= 17.01, its share of the budget being 2^-21;
  (a)  |t + beta delta s| <= 5.01 2^-24 |beta delta s| + 2^-34.
Measured here (the figures quoted in the comment and in DESIGN.md): (b) at most 2.7e-8 where |D| <= 17.01, against the derived
3.7e-7; (a) + (b) at most 3.3e-6 against the derived 5.5e-6."""
from fractions import Fraction

import numpy as np

import filter_argument_model as F

SHARE_B = 2.0 ** -21


def _cases(rng, n):
    """(x, delta, beta, sigma) with x well inside and up to the guard, delta = sigma z."""
    out = []
    for _ in range(n // 50000):
        beta = float(2.0 ** rng.uniform(-20, 10))
        _, _, l = F.setup(beta, 2.0 ** -30)
        sigma = float(2.0 ** rng.uniform(-12, l - 5))
        z = np.clip(rng.standard_normal(50000), -8.5, 8.5)
        x = rng.uniform(-1, 1, 50000) * 2.0 ** rng.uniform(-3, l - 1, 50000)
        out.append((x, sigma * z, beta, sigma))
    return out


def _adversarial(rng):
    out = []
    for beta in (2.0 ** -20, 0.37, 2.0, 1000.0, 2.0 ** 10, float(np.nextafter(2.0 ** 11, 0))):
        _, _, l = F.setup(beta, 2.0 ** -30)
        L = 2.0 ** l
        for sigma in (1e-3, 0.1, 3.0, L / 64):       # (L / 64: the largest sigma the launch constants admit)
            z = np.clip(rng.standard_normal(4096), -8.5, 8.5)
            d = sigma * z
            # x ~ -delta / 2: s cancels to a few ulp, dlogp is all rounding error of the squares
            out.append((-d / 2 * (1 + rng.integers(-4, 5, 4096) * 2.0 ** -52), d, beta, sigma))
            # |x| at the guard's bound: |s| = |2 x + delta| just below L
            x = np.sign(rng.standard_normal(4096)) * (L / 2) * (1 - rng.uniform(0, 2.0 ** -10, 4096))
            out.append((x - d / 2, d, beta, sigma))
            # delta far below x's ulp (xn == x) and the largest the guard lets through
            out.append((x / 2, d * 2.0 ** -60, beta, sigma))
            out.append((rng.uniform(-1, 1, 4096), np.sign(d) * 8.5 * (L / 64) * rng.uniform(0.5, 1, 4096), beta, L / 64))
    return out


def _term_b_exact(x, d, beta):
    """|D + beta delta s| and the derived bound, in exact rational arithmetic."""
    xn = x + d
    s = xn + x
    D = float(F.dlogp_reference(x, d, beta))
    err = abs(Fraction(D) + Fraction(beta) * Fraction(d) * Fraction(s))
    m = max(abs(x), abs(xn))
    bound = Fraction(1, 2 ** 53) * (Fraction(601, 100) * Fraction(beta) * Fraction(m) ** 2 + Fraction(201, 100) * abs(Fraction(D)))
    return float(err), float(bound), D, beta * m * m


def test_filter_argument_stays_inside_its_share_of_the_budget():
    rng = np.random.default_rng(20261019)
    worst_ab = worst_b = 0.0
    seen = 0
    for x, d, beta, sigma in _cases(rng, 1_000_000) + _adversarial(rng):
        y = F.y_model(x, d, beta, sigma)
        D = F.dlogp_reference(x, d, beta)
        inside = ~np.isnan(y)
        xn = x + d
        m2 = beta * np.maximum(np.abs(x), np.abs(xn)) ** 2
        assert np.all(m2[inside] < 2.0 ** 29 * (1 + 2.0 ** -49)), "the guard lets beta m^2 beyond its bound through"
        t = y.astype(np.float64) * F.LN2
        err = np.abs(t - D)
        # the claim as the comment states it, for every D (relative part) ...
        claim = 5.01 * 2.0 ** -24 * (np.abs(D) + 1e-6) + 2.0 ** -34 + 2.0 ** -53 * (6.01 * m2 + 2.01 * np.abs(D))
        assert np.all(err[inside] <= claim[inside]), float(np.max((err / claim)[inside]))
        # ... and as the budget uses it, where the filter relies on accuracy
        rel = inside & (np.abs(D) <= 17.01)
        seen += int(rel.sum())
        if rel.any():
            worst_ab = max(worst_ab, float(err[rel].max()))
            assert worst_ab <= 5.1e-6 + 6.1 * 2.0 ** -24
        # the sign ranges: D > 0 must not look like a reject, D < -17 not like an accept
        assert np.all(t[inside & (D > 0)] > -4e-7) and np.all(t[inside & (D < -17.0)] < -16.99)
        # term (b) exactly, on a slice of each batch
        for i in np.flatnonzero(rel)[:400]:
            e, bound, Di, bm2 = _term_b_exact(float(x[i]), float(d[i]), beta)
            assert e <= bound, (e, bound, float(x[i]), float(d[i]), beta)
            worst_b = max(worst_b, e)
    assert seen > 500_000
    print(f"largest |t - D| where |D| <= 17.01: {worst_ab:.3e} (derived 5.5e-6); largest term (b): {worst_b:.3e} (derived 3.7e-7, share {SHARE_B:.2e})")
    assert worst_b < 6.1 * 2.0 ** -24 < SHARE_B


def test_launch_constants():
    # the bound L = 2^l and where the launch falls back on accept_exact for every wave
    assert F.setup(2.0, 0.1)[2] == 13 and F.setup(2.0 ** 10, 0.1)[2] == 9 and F.setup(2.0 ** -20, 0.1)[2] == 24
    assert F.setup(0.0, 0.1)[2] == 46 and not np.isnan(F.setup(0.0, 0.1)[0])
    for beta in (np.inf, np.nan, -1.0, -0.0, 2.0 ** 25):
        assert np.isnan(F.setup(beta, 0.1)[0])
    assert not np.isnan(F.setup(float(np.nextafter(2.0 ** 25, 0)), 1e-3)[0])
    assert np.isnan(F.setup(2.0, 1e6)[0])                   # 8.6 sigma beyond L: every wave of the launch decides by accept_exact
    assert np.isnan(F.setup(2.0, np.inf)[0]) and np.isnan(F.setup(2.0, 2.0 ** 9)[0]) and not np.isnan(F.setup(2.0, 255.0)[0])


def test_special_values_end_undecided_or_exact():
    nan = np.nan
    x = np.array([np.inf, -np.inf, nan, 4096.0, -4096.0, 0.0, -0.0, 5e-324, 1.0, 1.0])
    d = np.array([0.1, 0.1, 0.1, 0.1, -0.1, 0.1, 0.1, 0.1, 0.0, 5e-324])
    y = F.y_model(x, d, 2.0, 0.1)
    assert np.all(np.isnan(y[:5])) and not np.any(np.isnan(y[5:]))
    assert y[8] == 0.0 and y[9] == 0.0                      # delta = 0, subnormal delta: ex = 1, an accept unless k = 4095
    assert np.all(np.isnan(F.y_model(x, d, np.inf, 0.1)))
    y0 = F.y_model(x, d, 0.0, 0.1)
    assert np.all(y0[5:] == 0.0)                            # beta = 0: D = 0, accept_exact accepts
