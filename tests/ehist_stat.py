"""The setup of the one statistical test of the energy histograms (tests/test_gpu_ehist_run.py) and its exact side, on the host: the
double well U = (x^2 - 1)^2 on the ladder beta_r = 0.5 * 1.5^r, R = 6, binned on [0, HI) in N_BINS bins; the exact probability of
every bin at every rung by quadrature of exp(-beta_r U); the continuum values the binned estimator approaches as the bins shrink.

A bin [a, b) of e = (x^2 - 1)^2 is, for x >= 0, the outer interval x^2 in [1 + sqrt(a), 1 + sqrt(b)) and -- while a < 1 -- the inner
one x^2 in (1 - sqrt(min(b, 1)), 1 - sqrt(a)]; the integrand is smooth on each, so a 24-point Gauss-Legendre rule is exact to rounding.
"""
import numpy as np

R = 6
BETAS = 0.5 * 1.5 ** np.arange(R)
LO, HI, N_BINS = 0.0, 80.0, 1600                     # 6 x 1603 = 9618 cells: the per-block LDS path
SHARDS, LADDERS = 16, 256                            # 16 handles, each a shard of 256 ladders of one ensemble
BURN_ROUNDS, ROUNDS, SWEEPS = 200, 300, 2            # rounds of [SWEEPS sweeps; one exchange step (; one snapshot)]
N_SAMPLES = SHARDS * LADDERS * R * ROUNDS            # every binned energy of the run
TARGET_BETAS = np.sqrt(BETAS[:4] * BETAS[1:5])       # four beta between the rungs: the geometric middles of the first four gaps

_GL_X, _GL_W = np.polynomial.legendre.leggauss(24)


def potential(x):
    return (x * x - 1.0) ** 2


def _integrate(f, lo, hi):
    """Gauss-Legendre over every interval [lo_i, hi_i] at once."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    half, mid = 0.5 * (hi - lo), 0.5 * (hi + lo)
    return half * np.sum(_GL_W * f(mid[..., None] + half[..., None] * _GL_X), axis=-1)


def bin_weights(beta, lo=LO, hi=HI, n_bins=N_BINS):
    """w_b = the integral of exp(-beta U) over {x : U(x) in bin b}, b < n_bins."""
    edges = lo + (hi - lo) / n_bins * np.arange(n_bins + 1)
    ra, rb = np.sqrt(edges[:-1]), np.sqrt(edges[1:])
    f = lambda x: np.exp(-beta * potential(x))
    outer = _integrate(f, np.sqrt(1.0 + ra), np.sqrt(1.0 + rb))
    inner = _integrate(f, np.sqrt(np.maximum(1.0 - rb, 0.0)), np.sqrt(np.maximum(1.0 - ra, 0.0)))
    return 2.0 * (outer + inner)


def tail_weight(beta, hi=HI):
    """The integral of exp(-beta U) over {U >= hi}: x beyond sqrt(1 + sqrt(hi)), cut where the integrand has left Float64."""
    x0 = np.sqrt(1.0 + np.sqrt(hi))
    pieces = x0 + np.arange(65) * 0.125
    return 2.0 * float(np.sum(_integrate(lambda x: np.exp(-beta * potential(x)), pieces[:-1], pieces[1:])))


def bin_probabilities():
    """p[R, N_BINS]: the exact probability of every bin at every rung (rows sum to 1 minus the tail beyond HI)."""
    w = np.stack([bin_weights(b) for b in BETAS])
    z = w.sum(axis=1) + np.array([tail_weight(b) for b in BETAS])
    return w / z[:, None]


def continuum(betas):
    """(log Z, <e>, C) of the continuum at every beta, by the same quadrature on fine bins (the moments of e inside a bin integrated,
    not taken at the centre)."""
    out = []
    for b in np.atleast_1d(betas):
        edges = np.linspace(0.0, 40.0 / min(b, 1.0) + 40.0, 4001)
        ra, rb = np.sqrt(edges[:-1]), np.sqrt(edges[1:])
        mom = []
        for k in range(3):
            f = lambda x: potential(x) ** k * np.exp(-b * potential(x))
            mom.append(2.0 * float(np.sum(_integrate(f, np.sqrt(1.0 + ra), np.sqrt(1.0 + rb)) +
                                          _integrate(f, np.sqrt(np.maximum(1.0 - rb, 0.0)), np.sqrt(np.maximum(1.0 - ra, 0.0))))))
        z, m1, m2 = mom[0], mom[1] / mom[0], mom[2] / mom[0]
        out.append((np.log(z), m1, b * b * (m2 - m1 * m1)))
    return tuple(np.array(v) for v in zip(*out))


def theta(counts, wham, reweight, energies):
    """The nine quantities of the test from counts[R, N_BINS] (integers or exact probabilities): f_r - f_0, r = 1 .. 5, and C at
    TARGET_BETAS."""
    log_g, f, _ = wham(counts, BETAS, energies)
    return np.concatenate([f[1:] - f[0], reweight(log_g, energies, TARGET_BETAS)[3]])
