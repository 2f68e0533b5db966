"""The deposit rule of the moments per energy bin (DESIGN.md section 3.17 "Moments per bin") on the CPU, three ways: the host twin
(tests/emom_twin.py, numpy with rint), exact rational arithmetic (fractions.Fraction, round half to even) and the product's own
__host__ __device__ functions compiled for the host (tests/aux/emom_deposit_host.cpp).  All three give the same integers."""
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import emom_twin as E

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "aux", "emom_deposit_host.cpp")
_CSRC = os.path.join(os.path.dirname(_HERE), "montecarlo_amd", "csrc")
BOUNDS = [4.0, 3.7, 0.3, 1.0, 2.0 ** -40, 1.5 * 2.0 ** 60]          # powers of two and not, small and large


def _lsb1(v: float) -> float:
    return struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", v))[0] | 1))[0]


def _exact(v: float, e: int) -> int:
    """RN(lsb1(v) / 2^e) in exact rational arithmetic; Python rounds a Fraction half to even."""
    return round(Fraction(_lsb1(v)) / (Fraction(2) ** e))


def edge_values(x_bound: float):
    e_x, e_xx = E.exponents(x_bound)
    q, qq = 2.0 ** e_x, 2.0 ** e_xx
    sub = 5e-324
    vals = [0.0, -0.0, sub, -sub, 2.0 ** -1030, -(2.0 ** -1030), x_bound, -x_bound, np.nextafter(x_bound, 0.0), -np.nextafter(x_bound, 0.0)]
    for k in (0, 1, 2, 12345, 2 ** 31 - 1):              # one ulp either side of a half quantum of x, and the half quantum itself
        h = (k + 0.5) * q
        if h <= x_bound:
            vals += [h, np.nextafter(h, 0.0), np.nextafter(h, np.inf), -h, -np.nextafter(h, 0.0), -np.nextafter(h, np.inf)]
    for k in (0, 1, 7, 99991):                           # ... and positions whose square lies at a half quantum of x^2, as near as a root gets
        r = math.sqrt((k + 0.5) * qq)
        if r <= x_bound:
            vals += [r, np.nextafter(r, 0.0), np.nextafter(r, np.inf), -r]
    # Float32-representable positions (their squares are exact in Float64)
    f32 = np.array([0.1, 0.7, 1.0 / 3.0, 0.999, 1e-3, 1e-20], dtype=np.float32).astype(np.float64) * x_bound
    vals += [float(np.float32(v)) for v in f32] + [-float(np.float32(v)) for v in f32]
    rng = np.random.default_rng(5)
    vals += list(rng.uniform(-x_bound, x_bound, 200)) + list(x_bound * 2.0 ** -rng.uniform(0, 60, 100))
    out = np.array([v for v in vals if abs(v) <= x_bound], dtype=np.float64)
    assert out.size >= 300
    return out


@pytest.mark.parametrize("x_bound", BOUNDS)
def test_exponents_bound_a_summand_by_two_to_the_32(x_bound):
    e_x, e_xx = E.exponents(x_bound)
    eb = e_x + 32
    assert 2.0 ** (eb - 1) <= x_bound < 2.0 ** eb and e_xx == 2 * eb - 32
    d = E.deposits(np.array([x_bound, -x_bound]), x_bound)
    assert np.all(np.abs(d[E.X]) <= 2 ** 32) and np.all(np.abs(d[E.XX]) <= 2 ** 32)


@pytest.mark.parametrize("x_bound", BOUNDS)
def test_twin_deposits_equal_exact_rational_arithmetic(x_bound):
    e_x, e_xx = E.exponents(x_bound)
    vals = edge_values(x_bound)
    d = E.deposits(vals, x_bound)
    for i, v in enumerate(vals):
        v = float(v)
        assert int(d[E.X][i]) == _exact(v, e_x), (v, "x")
        assert int(d[E.XX][i]) == _exact(v * v, e_xx), (v, "x2")          # v * v: one Float64 rounding, as the rule has it
        assert int(d[E.POS][i]) == (1 if v > 0 else 0)
        # lsb1 leaves no tie: the exact quotient is never an integer plus one half
        assert (Fraction(_lsb1(v)) / Fraction(2) ** e_x).denominator != 2


@pytest.fixture(scope="module")
def deposit_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("emom_deposit")
    exe, data = str(d / "emom_deposit_host"), str(d / "values.f64")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", _CSRC, _SRC, "-o", exe], check=True, capture_output=True)

    def run(values, x_bound):
        np.ascontiguousarray(values, dtype="<f8").tofile(data)
        out = subprocess.run([exe, data, repr(float(x_bound))], check=True, capture_output=True, text=True).stdout.splitlines()
        return tuple(int(v) for v in out[0].split()), np.array([[int(w) for w in line.split()] for line in out[1:]], dtype=np.int64)
    return run


@pytest.mark.parametrize("x_bound", BOUNDS)
def test_the_products_deposit_function_on_the_host_prints_the_twins_integers(deposit_host, x_bound):
    vals = edge_values(x_bound)
    beyond = np.array([np.nextafter(x_bound, np.inf), -np.nextafter(x_bound, np.inf), np.nan, np.inf, -np.inf, 2.0 * x_bound])
    exps, got = deposit_host(np.concatenate([vals, beyond]), x_bound)
    assert exps == E.exponents(x_bound)
    d = E.deposits(vals, x_bound)
    n = vals.size
    assert np.array_equal(got[:n, 0], d[E.X]) and np.array_equal(got[:n, 1], d[E.XX]) and np.array_equal(got[:n, 2], d[E.POS])
    assert np.all(got[:n, 3] == 1) and np.all(got[n:, 3] == 0)          # |x| <= x_bound; beyond it and NaN


def test_twin_snapshot_against_a_plain_loop():
    """The twin's cells and sums on a small made-up state, chain by chain in Python integers: the fourth tail cell takes the chains
    of a bin with |x| > x_bound or NaN, and such chains -- like those outside the bins -- reach no sum."""
    x = np.array([0.5, -0.5, 1.25, -1.75, 3.0, np.nan, 0.0, -0.0, 2.0, 1.0, 0.25, -2.5])
    e = np.where(np.isnan(x), 0.3, x * x)                    # (the NaN position is given an energy inside the bins)
    e[9] = np.nan                                            # ... and a position inside the bound an energy that is NaN
    lo, hi, n, G, x_bound = 0.25, 9.5, 5, 2, 2.0
    counts, sums = E.moments(e, x, lo, hi, n, E.X | E.XX | E.POS, x_bound, G)
    want_c, want_s = np.zeros((G, n + 4), dtype=np.int64), np.zeros((G, 3, n), dtype=np.int64)
    e_x, e_xx = E.exponents(x_bound)
    inv_w = n / (hi - lo)
    for i, (xi, ei) in enumerate(zip(x, e)):
        g = i % G
        cell = n + 2 if ei != ei else n if ei < lo else n + 1 if ei >= hi else min(int((ei - lo) * inv_w), n - 1)
        if cell < n and not abs(xi) <= x_bound:
            cell = n + 3
        want_c[g, cell] += 1
        if cell < n:
            want_s[g, 0, cell] += _exact(float(xi), e_x)
            want_s[g, 1, cell] += _exact(float(xi) * float(xi), e_xx)
            want_s[g, 2, cell] += 1 if xi > 0 else 0
    assert np.array_equal(counts.astype(np.int64), want_c) and np.array_equal(sums, want_s)
    assert want_c[:, n + 3].sum() == 3 and want_c[:, n + 2].sum() == 1          # 3.0, NaN, -2.5 beyond the bound; one NaN energy
    only_xx = E.moments(e, x, lo, hi, n, E.XX, x_bound, G)[1]
    assert only_xx.shape == (G, 1, n) and np.array_equal(only_xx[:, 0], sums[:, 1])
