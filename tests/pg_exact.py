"""An exact per-sample reference of the policy-gradient estimator's summands (Gaussian displacement policy) -- TEST INFRASTRUCTURE.

Plain Python: ``decimal`` at 80 digits and ``fractions``; it shares no code with the oracle (oracle/amc_oracle.c) or the
kernels.  One sample of gradients.jl:93-109 with P = 1 is split in two parts:

* The STATE-LIKE quantities are rounded, and the sweep tests pin them bit for bit.  They are formed here in IEEE arithmetic
  of the state's type T (numpy scalars), in the reference's order (particle_1d.jl:20-22,30-35, metropolis.jl:74):
  delta = T(0 + sigma z), x' = x + delta, e1 = V(x), e2 = V(x'), dlogp = (-e2 beta) - (-e1 beta), x'' = x' + (-delta),
  r = delta delta.  beta is a field of type T; sigma and z are Float64.
* The MATHEMATICAL quantities are evaluated exactly from those rounded inputs: alpha = exp(min(dlogp, 0)),
  j = r alpha, d = r / sigma^3 - 1 / sigma, grad j = j d, g = d^2.  d and g are rationals (``Fraction``), alpha is a
  ``Decimal`` good to 80 digits.  The delta^2 inside d is r, the square ROUNDED in T: the reference forms -(delta^2) in the
  action's type before it meets the Float64 sigma (particle_1d.jl:52-54), which matters for Float32 state.

``min`` keeps a NaN (Julia's rule): a dlogp that is NaN gives NaN for alpha, j and grad j, while d and g stay finite.
"""
from __future__ import annotations

import decimal
import functools
import math
from decimal import Decimal
from fractions import Fraction

import numpy as np

CTX = decimal.Context(prec=80, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN, rounding=decimal.ROUND_HALF_EVEN)
PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899862803482534211707")
U = Fraction(1, 2 ** 52)                     # the unit of every bound: one ulp of a Float64 in [1, 2)
TINY = Decimal(2) ** -1074                    # the smallest Float64 step: what a result near the underflow edge rounds to
FLUSH = -708.0                               # exp of an argument below this is flushed to 0 by the spec (amc_math.h)


def _dec(v) -> Decimal:
    if isinstance(v, Decimal):
        return v
    if isinstance(v, Fraction):
        return CTX.divide(Decimal(v.numerator), Decimal(v.denominator))
    return Decimal(float(v))                 # exact


def _potential(pot: str, x):
    """V(x) in the type of x: particle_1d.jl's two potentials, operation for operation."""
    if pot == "double_well":
        q = x * x - type(x)(1.0)
        return q * q
    if pot != "harmonic":
        raise ValueError(pot)
    return x * x


@functools.lru_cache(maxsize=256)
def _sigma_constants(sigma: float):
    """(1 / sigma, sigma^3, 2 sigma^2 as Fractions, log(2 pi sigma^2) / 2 as a Decimal)"""
    fs = Fraction(sigma)
    return 1 / fs, fs ** 3, 2 * fs * fs, CTX.divide(CTX.ln(CTX.multiply(2 * PI, _dec(fs * fs))), Decimal(2))


class Sample:
    """One estimator sample: the rounded state-like floats, the exact values, and the scales the bounds are written in."""
    __slots__ = ("delta", "x_moved", "x_after", "e1", "e2", "dlogp", "r", "sigma", "nan", "alpha", "j", "d", "dj", "g",
                 "terms", "abs_logq")

    def exact(self):
        """(j, grad j, d logq / d sigma, g) -- Decimal, Decimal, Fraction, Fraction; the first two None when NaN."""
        return self.j, self.dj, self.d, self.g


def sample(potential: str, beta: float, sigma: float, z: float, x: float, dtype: str = "f64") -> Sample:
    T = {"f64": np.float64, "f32": np.float32}[dtype]
    s = Sample()
    with np.errstate(all="ignore"):
        sig, zz = np.float64(sigma), np.float64(z)
        delta = T(np.float64(0.0) + sig * zz)
        x0, b = T(x), T(beta)
        x1 = x0 + delta
        e1, e2 = _potential(potential, x0), _potential(potential, x1)
        dlogp = ((-e2) * b) - ((-e1) * b)
        x2 = x1 + (-delta)
        r = delta * delta
    s.delta, s.x_moved, s.x_after, s.e1, s.e2 = float(delta), float(x1), float(x2), float(e1), float(e2)
    s.dlogp, s.r, s.sigma = float(dlogp), float(r), float(sigma)
    # the exact part: from the ROUNDED delta, r and dlogp
    inv, cube, den, half_log = _sigma_constants(float(sigma))
    fr = Fraction(s.r)
    quad = fr / cube
    s.d = quad - inv
    s.terms = quad + inv
    s.g = s.d * s.d
    # |log q(delta; sigma)| = |-(delta^2) / (2 sigma^2) - log(2 pi sigma^2) / 2|, the reference form's exp argument detours through it
    logq = -_dec(fr / den) - half_log
    s.abs_logq = abs(logq)
    s.nan = math.isnan(s.dlogp)
    if s.nan:
        s.alpha = s.j = s.dj = None
        return s
    arg = min(s.dlogp, 0.0)
    s.alpha = Decimal(0) if arg == -math.inf else CTX.exp(Decimal(arg))
    s.j = CTX.multiply(Decimal(s.r), s.alpha)
    s.dj = CTX.multiply(s.j, _dec(s.d))
    return s


def units(s: Sample):
    """The four units of the bounds (Decimals): 2^-52 |j|, 2^-52 |j| terms, 2^-52 terms, 2^-52 terms^2.
    None for the first two when the sample is NaN."""
    u, t = _dec(U), _dec(s.terms)
    ut = CTX.multiply(u, t)
    if s.nan:
        return None, None, ut, CTX.multiply(ut, t)
    uj = CTX.multiply(u, abs(s.j))
    return uj, CTX.multiply(uj, t), ut, CTX.multiply(ut, t)


def errors(got, s: Sample):
    """|got[i] - exact[i]| as Decimals (None where the exact value is NaN); got: four floats, finite where the exact value is."""
    ex = s.exact()
    out = []
    for i in range(4):
        if ex[i] is None:
            out.append(None)
        elif isinstance(ex[i], Decimal):
            out.append(abs(CTX.subtract(Decimal(float(got[i])), ex[i])))
        else:
            out.append(_dec(abs(Fraction(float(got[i])) - ex[i])))       # the difference of two rationals, formed exactly
    return out


def reference_argument(s: Sample) -> Decimal:
    """2 + |dlogp| + |logq|: the reference-ordered form's alpha goes through exp(dlogp + logq_b - logq_f), whose argument carries
    rounding errors of this size times 2^-52."""
    return 2 + Decimal(abs(s.dlogp)) + s.abs_logq


# ---- a whole estimator call, sample by sample ---------------------------------------------------------------------------

def normals(oracle_lib, seed: int, chain_ids, t_est: int, draw: int):
    """z of every chain in ``chain_ids`` (global ids) for draw index ``draw`` of estimator step ``t_est``: chains 2p and 2p + 1
    share one Box-Muller draw of pair p.  Philox and Box-Muller are pinned by their own known-answer tests."""
    cache, out = {}, []
    for g in chain_ids:
        p = int(g) >> 1
        if p not in cache:
            cache[p] = oracle_lib.box_muller(oracle_lib.draw_words(seed, p, t_est, draw, oracle_lib.STREAM_ESTIMATOR))
        out.append(cache[p][int(g) & 1])
    return out


def walk_call(oracle_lib, *, potential, beta, sigma, seed, t_est, learn, q_batch, x, chain_offset=0, dtype="f64"):
    """One estimator call over M = len(x) chains, the loop order of amo_pg_estimate_plain: per learnable move l, chain c and
    sample q the draw index is l * q_batch + q, and every sample starts from the position the previous one left.
    Returns (samples[l][c][q], x after the call)."""
    x = [float(v) for v in x]
    M = len(x)
    ids = [chain_offset + c for c in range(M)]
    out = []
    for l, lid in enumerate(learn):
        zs = [normals(oracle_lib, seed, ids, t_est, l * q_batch + q) for q in range(q_batch)]
        per_chain = []
        for c in range(M):
            row = []
            for q in range(q_batch):
                s = sample(potential, beta, sigma[lid], zs[q][c], x[c], dtype)
                x[c] = s.x_after
                row.append(s)
            per_chain.append(row)
        out.append(per_chain)
    return out, x


def dsum(values) -> Decimal:
    """The sum of Decimals / Fractions, every addition rounded to 80 digits."""
    acc = Decimal(0)
    for v in values:
        acc = CTX.add(acc, _dec(v))
    return acc
