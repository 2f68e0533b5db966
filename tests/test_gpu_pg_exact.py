"""The estimator kernels' per-sample summands on the device: equal to the spec twin bit for bit, and within the host-measured
bounds of an EXACT reference (tests/pg_exact.py), so that an edit of kernel and twin together still fails.

One sample is visible from the device only through a call with one chain, one learnable move and q_batch = 1, and only as
its kind-Q deposit RN(lsb1(v) / 2^E) 2^E (amc_xsum.h): the bounds of tests/test_pg_exact_host.py (SPEC_BOUND, REF_BOUND,
measured on the CPU against the exact reference alone) are therefore taken together with the deposit term derived there from
the sum's definition -- half a quantum and 3 u |v| -- and with nothing else.  One handle per (potential, state type, beta);
sigma moves through set_parameters, x through upload_state, the draw through the estimator_step setter.
"""
import math

import numpy as np
import pytest

import oracle_lib as O
import pg_exact as X
import test_pg_exact_host as H

pytestmark = pytest.mark.gpu

BETAS = (0.2, 2.0, 20.0)
SEED = 0x5EED0000AB
N_SIGMA = 40


def xbits(v, dtype):
    a = np.ascontiguousarray(v, dtype=np.float64)
    return a.astype(np.float32).view(np.uint32) if dtype == "f32" else a.view(np.uint64)


def sigmas(rng):
    return [1e-3, 10.0] + [float(np.exp(rng.uniform(np.log(1e-3), np.log(10.0)))) for _ in range(N_SIGMA)]


def one_z(t_est, chain=0):
    return O.box_muller(O.draw_words(SEED, chain >> 1, t_est, 0, O.STREAM_ESTIMATOR))[chain & 1]


class Pair:
    """A one-chain device handle and its oracle twin, moved together."""

    def __init__(self, gpu, pot, dtype, beta):
        kw = dict(potential=pot, beta=beta, sigma=[1.0], weight=[1.0], seed=SEED, dtype=dtype)
        self.pot, self.dtype, self.beta = pot, dtype, beta
        self.e = gpu.HipEngine(n_chains=1, **kw)
        self.o = O.OracleEngine(n_chains=1, **kw)

    def close(self):
        self.e.close()
        self.o.close()

    def sample(self, sigma, x, t_est):
        """Run one sample on both; returns (device records, twin records, device x after, z, exact sample)."""
        x = H.as_state(x, self.dtype)
        for h in (self.e, self.o):
            h.set_parameters(0, [sigma])
            h.upload_state(np.array([x]))
            h.estimator_step = t_est
        rec = self.e.pg_estimate_exact([0], 1)
        rec_o = self.o.sim.pg_estimate_records([0], 1)
        z = one_z(t_est)
        return rec, rec_o, self.e.download_state()[0], z, X.sample(self.pot, self.beta, sigma, z, x, self.dtype)


def check_one(p, sigma, x, t_est, where):
    """The three per-sample checks; returns the exact sample."""
    rec, rec_o, x_dev, z, s = p.sample(sigma, x, t_est)
    # 1. the twin, word for word, and the position
    assert np.array_equal(rec.view(np.uint64), rec_o.view(np.uint64)), (where, rec, rec_o)
    assert np.array_equal(xbits(x_dev, p.dtype), xbits([s.x_after], p.dtype)), (where, x_dev, s.x_after)
    assert np.array_equal(xbits(p.o.download_state()[0], p.dtype), xbits([s.x_after], p.dtype))
    got = O.xsum_round(rec[0])
    assert got[4] == 1.0
    # 2. the exact value: the host-measured bound and the deposit of ONE summand (a sum below 2^53 quanta rounds exactly)
    ex = O.gd_exponents(sigma)
    bounds = H.sample_bounds(s, ex)
    err = X.errors(got[:4], s)
    for i in range(4):
        assert err[i] <= bounds[i][1], (where, i, float(err[i]), float(bounds[i][1]), got, sigma, x, z)
    # 3. the reference-ordered form at the same z: through the exact value, its bound plus the spec form's
    ref, x_ref = O.pg_summands(p.pot, p.beta, sigma, z, H.as_state(x, p.dtype), "reference", p.dtype)
    assert np.array_equal(xbits([x_ref], p.dtype), xbits(x_dev, p.dtype))
    for i in range(4):
        d = abs(X.Decimal(float(got[i])) - X.Decimal(float(ref[i])))
        assert d <= bounds[i][1] + bounds[i][2], (where, "reference", i, float(d), got, ref)
    return s


@pytest.fixture(scope="module")
def pairs(gpu):
    made = {}

    def get(pot, dtype, beta):
        key = (pot, dtype, beta)
        if key not in made:
            made[key] = Pair(gpu, pot, dtype, beta)
        return made[key]
    yield get
    for p in made.values():
        p.close()


def grid_cases(pot, dtype, beta):
    rng = np.random.default_rng([H.GRID_SEED, 11, H.POTS.index(pot), H.DTYPES.index(dtype), int(beta * 10)])
    return [(sigma, float(rng.normal(0.0, 1.5)), int(rng.integers(0, 2 ** 40))) for sigma in sigmas(rng)]


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("pot", H.POTS)
def test_one_sample_equals_the_spec_twin_bit_for_bit(pairs, pot, dtype, beta):
    """pg_estimate_exact([0], 1) of one chain: records equal to the oracle's (the spec twin's deposits), word for word, and the
    position bit for bit; over >= 40 sigma log-uniform in [1e-3, 10] and both ends, a fresh x and draw each."""
    p = pairs(pot, dtype, beta)
    for k, (sigma, x, t) in enumerate(grid_cases(pot, dtype, beta)):
        rec, rec_o, x_dev, z, s = p.sample(sigma, x, t)
        assert np.array_equal(rec.view(np.uint64), rec_o.view(np.uint64)), (k, sigma, x, z, rec, rec_o)
        assert np.array_equal(xbits(x_dev, dtype), xbits(p.o.download_state()[0], dtype))
        assert np.array_equal(xbits(x_dev, dtype), xbits([s.x_after], dtype))


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("pot", H.POTS)
def test_one_sample_within_the_exact_bounds(pairs, pot, dtype, beta):
    """The device's rounded summands within SPEC_BOUND (measured on the host against the exact reference alone) of
    pg_exact's values, plus the deposit term of the one summand; nothing for the device itself."""
    p = pairs(pot, dtype, beta)
    for k, (sigma, x, t) in enumerate(grid_cases(pot, dtype, beta)):
        check_one(p, sigma, x, t ^ 0x55, (pot, dtype, beta, k))


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("pot", H.POTS)
def test_one_sample_against_the_reference_ordered_form(pairs, pot, dtype, beta):
    """Against amo_pg_summands_reference(_f32) at the reconstructed z: REF_BOUND plus SPEC_BOUND (with the deposit), the
    triangle inequality through the exact value; both measured on the CPU.  (check_one asserts all three relations; this
    test walks other draws than the two above.)"""
    p = pairs(pot, dtype, beta)
    for k, (sigma, x, t) in enumerate(grid_cases(pot, dtype, beta)):
        check_one(p, sigma, x, t ^ 0xAA00, (pot, dtype, beta, k))


@pytest.fixture(scope="module")
def tail_steps():
    """The first eight estimator steps whose z for chain 0 has |z| >= 4 (P ~ 6.3e-5 per draw)."""
    found, t = [], 0
    while len(found) < 8:
        if abs(one_z(t)) >= 4.0:
            found.append(t)
        t += 1
        assert t < 2_000_000
    return found


@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("pot", H.POTS)
def test_tail_draws(pairs, tail_steps, pot, dtype):
    """Draws from the tail of the normal (|z| >= 4, found by scanning the estimator stream on the host), the alpha == 0 arm
    (sigma = 12 from |x| = 30) and the dlogp ~ 0 arm (x = 0, sigma = 1e-3): the same three checks, and each arm really hit."""
    p = pairs(pot, dtype, 2.0)
    for t in tail_steps:
        for sigma in (1e-3, 0.37, 10.0):
            s = check_one(p, sigma, 0.4, t, (pot, dtype, "tail", t, sigma))
            assert abs(s.delta) >= 3.99 * sigma
    flushed = near_zero = 0
    for t in range(16):
        # away from the origin (x takes the sign of the draw): dlogp < -708 as soon as |z| > 0.45
        s = check_one(p, 12.0, math.copysign(30.0, one_z(1000 + t)), 1000 + t, (pot, dtype, "alpha == 0", t))
        flushed += s.dlogp < X.FLUSH
        s = check_one(p, 1e-3, 0.0, 2000 + t, (pot, dtype, "dlogp ~ 0", t))
        near_zero += abs(s.dlogp) < 1e-4
    assert flushed >= 4 and near_zero == 16, (flushed, near_zero)


# ---- whole calls -------------------------------------------------------------------------------------------------------------

OFFSETS = (0, 2 ** 20 + 2)
LEARN = [2, 0]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("pot", H.POTS)
def test_fold_against_the_exact_sum(gpu, pot, dtype, offset):
    """M in {1, 2, 63, 65, 4099} chains from chain_offset, learn = [2, 0] of a K = 3 pool, q in {1, 3} (and q = 20 once at
    M = 65: more than 32 summands per lane, the mid-loop flush): every column's rounded sum against the exact sum of pg_exact's
    per-sample values, within the sum of the per-sample bounds plus the kind-Q deposit terms (test_pg_exact_host.py, where the
    same bound is confirmed with the oracle's fold); the reference-ordered left-to-right fold under its own bound; the count
    exactly M q.  The exact values of the first m chains do not depend on M, so one walk over 4099 chains serves every M."""
    runs = [(q, H.FOLD_M) for q in (1, 3)] + ([(20, (65,))] if offset else [])
    for q, Ms in runs:
        kw, x = H.fold_case(pot, dtype, max(Ms))
        per_chain, x_after = H.fold_reference(learn=LEARN, q_batch=q, x=x, chain_offset=offset, t_est=0, **kw)
        for m in Ms:
            e = gpu.HipEngine(n_chains=m, chain_offset=offset, n_chains_global=offset + m, weight=[0.5, 0.25, 0.25], **kw)
            o = O.OracleSim(m, chain_offset=offset, weight=[0.5, 0.25, 0.25], **kw)
            e.upload_state(x[:m])
            o.set_x(x[:m])
            got = e.pg_estimate(LEARN, q)
            H.check_fold(got, o.pg_estimate_plain(LEARN, q), per_chain, m, q, (pot, dtype, offset, q, m))
            assert np.array_equal(xbits(e.download_state()[0], dtype), xbits(x_after[:m], dtype))
            e.close()
            o.close()
