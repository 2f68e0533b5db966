"""Host twin of the choice of the next beta (DESIGN.md section 3.14 "Choosing the next beta"), beside anneal_twin.py.

Written from the DESIGN text with the oracle's own primitives -- amo_potential (amo_potential_f32 for Float32 state), amo_exp -- numpy
operations on float64 / float32 values for the arithmetic in the state's type T (each a single IEEE operation, elementwise on arrays
as on scalars: nothing is contracted), and Python integers for everything that crosses chains (the weights and their three sums per
candidate).  It shares no code with the product.
"""
import math

import numpy as np

import anneal_twin as A
import oracle_lib as O

CANDIDATES = 8
MAX_ROUNDS = 16
WORDS = 8
OK, LIMIT, BELOW_RESOLUTION, STALLED, ALL_NAN, INF, NO_WEIGHT = range(7)
NAN_BITS = 0x7FF8000000000000
MASK30 = (1 << A.WEIGHT_BITS) - 1


def _T(f32):
    return np.float32 if f32 else np.float64


def span(beta, beta_limit, f32):
    """D = Float64(T(beta_limit) - T(beta))."""
    T = _T(f32)
    return float(T(beta_limit) - T(beta))


def energies(pot, x, f32):
    """ne_i = -potential(x_i) in T, as Float64 (exact)."""
    lib = O.load()
    T = _T(f32)
    if f32:
        return np.array([float(-T(lib.amo_potential_f32(pot, float(T(v))))) for v in x], dtype=np.float64)
    return np.array([float(-T(lib.amo_potential(pot, float(v)))) for v in x], dtype=np.float64)


def extremes(ne):
    """(ne_hi, ne_lo): the largest and the smallest non-NaN ne in the order of the keys (-0 below +0); None when every one is a NaN."""
    keyed = [(A.order_key(v), v) for v in map(float, ne) if v == v]
    if not keyed:
        return None
    return max(keyed)[1], min(keyed)[1]


def product(ne, d, f32):
    """Float64(T(ne) * T(d)), ne a scalar or an array."""
    T = _T(f32)
    with np.errstate(all="ignore"):
        p = np.asarray(ne, dtype=np.float64).astype(T) * T(d)
    assert p.dtype == T
    return p.astype(np.float64)


def candidates(lo, hi, ne_hi, ne_lo, f32):
    """The eight steps of a round and the largest log-weight of each."""
    T = _T(f32)
    with np.errstate(all="ignore"):
        w = np.float64(hi) - np.float64(lo)
        deltas = [float(T(np.float64(lo) + w * np.float64((k + 1) / 8.0))) for k in range(CANDIDATES - 1)] + [float(hi)]
    a_max = [float(product(ne_hi if d > 0.0 else ne_lo, d, f32)) for d in deltas]
    return deltas, a_max


def sums(ne, d, a_max, f32):
    """(S1, S2h, S2l) of one candidate: Python integers."""
    exp = O.load().amo_exp
    with np.errstate(all="ignore"):
        t = product(ne, d, f32) - np.float64(a_max)
    scale = 2.0 ** A.WEIGHT_BITS
    W = [0 if (v != v or v == -math.inf) else int(math.floor(scale * exp(v))) for v in t.tolist()]
    assert all(0 <= w <= 1 << A.WEIGHT_BITS for w in W)
    sq = [w * w for w in W]
    return sum(W), sum(s >> A.WEIGHT_BITS for s in sq), sum(s & MASK30 for s in sq)


def rho_of(S, M):
    s1 = np.float64(S[0])
    s2 = np.float64(S[1]) * np.float64(2.0 ** 30) + np.float64(S[2])
    with np.errstate(all="ignore"):
        return float((s1 * s1) / (np.float64(M) * s2))


def next_beta(pot, x, beta, beta_limit, target, rounds, f32):
    """(beta_new, diag, trace) as amc_anneal_next_beta returns them: diag 8 integers, trace rounds x 8 x 3 integers."""
    assert 0.0 < target < 1.0 and 1 <= rounds <= MAX_ROUNDS and math.isfinite(beta_limit)
    T = _T(f32)
    M = len(x)
    trace = [[[0, 0, 0] for _ in range(CANDIDATES)] for _ in range(rounds)]
    D = span(beta, beta_limit, f32)
    assert math.isfinite(D)
    if D == 0.0:
        return float(beta_limit), [LIMIT, 0, 0, 0, 0, 0, 0, 0], trace
    ne = energies(pot, x, f32)
    ext = extremes(ne)
    one = A.f64_bits(1.0)
    if ext is None:
        return float(beta_limit), [ALL_NAN, 0, A.f64_bits(D), one, A.f64_bits(D), 0, NAN_BITS, NAN_BITS], trace
    ne_hi, ne_lo = ext
    lo, hi, rho_lo, rho_hi = 0.0, D, 1.0, 0.0
    for r in range(rounds):
        deltas, a_max = candidates(lo, hi, ne_hi, ne_lo, f32)
        S = [sums(ne, d, am, f32) for d, am in zip(deltas, a_max)]
        trace[r] = [list(s) for s in S]
        if r == 0 and not math.isfinite(a_max[-1]):
            assert a_max[-1] == a_max[-1]
            status = INF if a_max[-1] > 0 else NO_WEIGHT
            return float(beta_limit), [status, 0, A.f64_bits(D), one, A.f64_bits(D), 0, A.f64_bits(ne_hi), A.f64_bits(ne_lo)], trace
        rho = [rho_of(s, M) for s in S]
        fails = [k for k in range(CANDIDATES) if not rho[k] >= target]
        if not fails:
            assert r == 0, "hi fails from round 1 on"
            return float(beta_limit), [LIMIT, 1, A.f64_bits(D), A.f64_bits(rho[-1]), A.f64_bits(D), 0, A.f64_bits(ne_hi),
                                       A.f64_bits(ne_lo)], trace
        j = fails[0]
        hi, rho_hi = deltas[j], rho[j]
        if j > 0:
            lo, rho_lo = deltas[j - 1], rho[j - 1]
    status, step = OK, lo
    if lo == 0.0:
        status, step = BELOW_RESOLUTION, hi
    with np.errstate(all="ignore"):
        beta_new = float(T(beta) + T(step))
    if beta_new == float(T(beta)):
        status, beta_new = STALLED, float(beta)
    elif (beta_new > beta_limit) if D > 0.0 else (beta_new < beta_limit):
        beta_new = float(beta_limit)               # never past the limit
    diag = [status, rounds, A.f64_bits(step), A.f64_bits(rho_lo), A.f64_bits(hi), A.f64_bits(rho_hi), A.f64_bits(ne_hi), A.f64_bits(ne_lo)]
    return beta_new, diag, trace


def twin_next_beta(tw, beta_limit, target, rounds=6):
    """next_beta on the state of an anneal_twin.AnnealTwin, as numpy arrays shaped like HipEngine.anneal_next_beta's."""
    b, diag, trace = next_beta(tw.pot, tw.x(), tw.beta, float(beta_limit), float(target), int(rounds), tw.f32)
    return b, np.array(diag, dtype=np.uint64), np.array(trace, dtype=np.uint64).reshape(int(rounds), CANDIDATES, 3)


class AnnealSearchTwinEngine(A.AnnealTwinEngine):
    """anneal_twin.AnnealTwinEngine with HipEngine.anneal_next_beta, computed by the twin above."""

    def anneal_next_beta(self, beta_limit, target, rounds=6):
        assert self.whole, "the handle does not hold the whole ensemble"
        return twin_next_beta(self.twin, beta_limit, target, rounds)
