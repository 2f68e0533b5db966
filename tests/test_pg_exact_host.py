"""The estimator's per-sample summands against an exact reference (tests/pg_exact.py), on the host.

The kernels' arithmetic is restated by the oracle's spec twin; the device tests compare the two bit for bit
(tests/test_gpu_pg_exact.py).  THIS file ties the twin -- and the reference-ordered restatement of gradients.jl:93-109 -- to
the exact value of the same mathematics, so that an edit that changes kernel and twin together still fails.

Units (u = 2^-52): j in u |j|; grad j in u |j| terms; d logq / d sigma in u terms; g in u terms^2, with
terms = r / sigma^3 + 1 / sigma and r = fl(delta^2) in the state's type (d itself cancels to 0 at |z| = 1).  The same units
serve Float32 state: the state-like inputs (delta, r, dlogp) are exact in the helper, and alpha, d and g are Float64.
Every bound is the next power of two above the worst case measured on the grid below against the exact reference ALONE --
no device number enters.  j and grad j get one Float64 step (2^-1074) on top where r alpha nears the underflow edge.

Measured: GRID_N random samples per potential and state type (seed GRID_SEED) plus the edge cases, worst of both potentials:

    spec form vs exact                             Float64 state   Float32 state   bound
      j                  / (u |j|)                 1.371           1.465           2
      grad j             / (u |j| terms)           2.021           1.940           4
      d logq / d sigma   / (u terms)               1.454           1.613           2
      g                  / (u terms^2)             3.114           3.200           4
    reference-ordered form vs exact
      j        / ((2 + |dlogp| + |logq|) u |j|)         c = 0.883   0.528          c = 1
      grad j   / ((2 + |dlogp| + |logq|) u |j| terms)   c = 0.858   0.586          c = 1
      d logq / d sigma   / (u terms)               1.658           1.658           2
      g                  / (u terms^2)             3.114           3.200           4

dlogp = -0.0 does not occur with these potentials: dlogp = (-e2 beta) - (-e1 beta) with e1, e2 >= +0 is +0.0 when the two
products are equal, so only the +0.0 arm can be -- and is -- reached.
"""
import math

import numpy as np
import pytest

import oracle_lib as O
import pg_exact as X

GRID_N = 4000
GRID_SEED = 20261021
POTS = ("harmonic", "double_well")
DTYPES = ("f64", "f32")

# (j, grad j, d logq / d sigma, g) in the units above
SPEC_BOUND = (2, 4, 2, 4)
# reference-ordered form: c for j and grad j (times 2 + |dlogp| + |logq|), then d logq / d sigma and g in their units
REF_BOUND = (1, 1, 2, 4)


def as_state(v, dtype):
    return float(np.float32(v)) if dtype == "f32" else float(v)


def random_grid(pot, dtype, n=GRID_N):
    """(beta, sigma, z, x): the device fuzz test's ranges -- beta in [0.2, 20] and sigma in [1e-3, 10] log-uniform,
    x ~ N(0, 1.5^2), z normal with every fifth one scaled by 3."""
    rng = np.random.default_rng([GRID_SEED, POTS.index(pot), DTYPES.index(dtype)])
    out = []
    for i in range(n):
        beta = float(np.exp(rng.uniform(np.log(0.2), np.log(20.0))))
        sigma = float(np.exp(rng.uniform(np.log(1e-3), np.log(10.0))))
        z = float(rng.standard_normal()) * (3.0 if i % 5 == 4 else 1.0)
        out.append((beta, sigma, z, as_state(rng.normal(0.0, 1.5), dtype)))
    return out


def edge_grid(pot, dtype):
    """Finite inputs that reach every arm: sigma at both ends of its range, |z| around 1 (d cancels), moves downhill and
    exactly level (alpha == 1), x = 0 with a tiny sigma (dlogp = +0.0 or a rounding error below), dlogp in [-708, -700] and far
    below -708 (alpha flushed to 0)."""
    rng = np.random.default_rng([GRID_SEED, 77, POTS.index(pot), DTYPES.index(dtype)])
    out = []
    for sigma in (1e-3, 10.0):
        for _ in range(60):
            out.append((float(np.exp(rng.uniform(np.log(0.2), np.log(20.0)))), sigma, float(rng.standard_normal()),
                        as_state(rng.normal(0.0, 1.5), dtype)))
    for k in range(120):                                           # |z| near 1, both signs
        z = (1.0 + float(rng.uniform(-1, 1)) * 10.0 ** -(k % 12)) * (1 if k % 2 else -1)
        out.append((2.0, float(np.exp(rng.uniform(np.log(1e-3), np.log(10.0)))), z, as_state(rng.normal(0.0, 1.5), dtype)))
    out += [(2.0, 0.5, 1.0, 0.3), (2.0, 0.5, -1.0, 0.3), (2.0, 1e-3, 0.0, 0.3), (2.0, 1e-3, -0.0, 0.0)]
    for k in range(60):                                            # downhill in the harmonic well: x > 0, -2x < delta < 0
        x = as_state(rng.uniform(0.5, 2.0), dtype)
        out.append((float(rng.uniform(0.2, 20.0)), 1.0, -float(rng.uniform(0.0, 1.0)) * x, x))
    for k in range(40):                                            # from x = 0 with a tiny sigma: dlogp = +0.0, or -(tiny)
        out.append((float(rng.uniform(0.2, 20.0)), 1e-3, float(rng.standard_normal()) * 10.0 ** -(k % 8), 0.0))
    out += [(2.0, 1e-3, 1e-160, 0.0), (2.0, 1e-3, -1e-160, 0.0)]   # delta^2 underflows: dlogp = +0.0 exactly
    # dlogp in [-708, -700] and just below: from x = 0 with beta = 1 the move delta gives dlogp = -delta^2 in the harmonic
    # well and -(delta^4 - 2 delta^2) in the double well
    for target in np.linspace(700.0, 708.5, 35):
        d2 = float(target) if pot == "harmonic" else 1.0 + math.sqrt(1.0 + float(target))
        out.append((1.0, 10.0, math.sqrt(d2) / 10.0, 0.0))
    for k in range(20):                                            # far below: alpha == 0
        out.append((20.0, 10.0, 3.0 + k * 0.2, as_state(1.0 + 0.1 * k, dtype)))
    return out


def nonfinite_grid(dtype):
    return [(2.0, float(np.exp(s)), z, x) for s in (-6.0, -1.0, 2.0) for z in (-1.3, 0.0, 0.7)
            for x in (float("nan"), float("inf"), -float("inf"))]


def both_forms(pot, dtype, case):
    beta, sigma, z, x = case
    spec, xs = O.pg_summands(pot, beta, sigma, z, x, "spec", dtype)
    ref, xr = O.pg_summands(pot, beta, sigma, z, x, "reference", dtype)
    return spec, xs, ref, xr


def bits(v):
    return np.float64(v).view(np.uint64)


def measure(pot, dtype, cases):
    """Worst errors of both forms in their units, and which arms the cases reached; asserts the exact identities on the way
    (position bit for bit, alpha == 1 and alpha == 0 arms)."""
    worst_spec, worst_ref = [X.Decimal(0)] * 4, [X.Decimal(0)] * 4
    arms = dict(level=0, downhill=0, flushed=0, near_flush=0, cancel=0, zero_sign=set())
    for case in cases:
        s = X.sample(pot, *case, dtype)
        spec, xs, ref, xr = both_forms(pot, dtype, case)
        assert bits(xs) == bits(s.x_after) and bits(xr) == bits(s.x_after), (case, xs, xr, s.x_after)      # (c)
        assert not s.nan
        u = X.units(s)
        es, er = X.errors(spec, s), X.errors(ref, s)
        arg = X.reference_argument(s)
        if s.dlogp >= 0.0:                                       # alpha == 1 exactly: j is the reward
            assert spec[0] == s.r and ref[0] == s.r, (case, spec, ref, s.r)
            arms["downhill" if s.dlogp > 0.0 else "level"] += 1
            if s.dlogp == 0.0:
                arms["zero_sign"].add(math.copysign(1.0, s.dlogp))
        if s.dlogp < X.FLUSH:                                    # alpha flushed: j == 0 exactly, the exact j below r e^-708
            assert spec[0] == 0.0 and spec[1] == 0.0 and ref[0] == 0.0 and ref[1] == 0.0, (case, spec, ref)
            assert s.j <= X.CTX.multiply(X.Decimal(s.r), X.CTX.exp(X.Decimal(-708)))
            arms["flushed"] += 1
            es[0] = es[1] = er[0] = er[1] = X.Decimal(0)
        elif s.dlogp <= -700.0:
            arms["near_flush"] += 1
        if abs(s.d) <= s.terms / 1000:
            arms["cancel"] += 1
        for i in range(4):
            floor = X.TINY if i < 2 else 0                       # j near the underflow edge: one Float64 step
            scale_ref = u[i] * arg if i < 2 else u[i]
            if es[i] > floor:
                worst_spec[i] = max(worst_spec[i], (es[i] - floor) / u[i])
            if er[i] > floor:
                worst_ref[i] = max(worst_ref[i], (er[i] - floor) / scale_ref)
    return [float(v) for v in worst_spec], [float(v) for v in worst_ref], arms


@pytest.fixture(scope="module", autouse=True)
def built_oracle():
    O.build()


@pytest.fixture(scope="module")
def measured():
    return {(pot, dtype): measure(pot, dtype, random_grid(pot, dtype) + edge_grid(pot, dtype)) for pot in POTS for dtype in DTYPES}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pot", POTS)
def test_spec_twin_against_exact(measured, pot, dtype):
    """2(a): the spec form (what the kernels run) within SPEC_BOUND of the exact value, in the four units."""
    worst, _, arms = measured[(pot, dtype)]
    print(f"spec vs exact {pot} {dtype}: worst {worst}, bound {SPEC_BOUND}")
    for i in range(4):
        assert worst[i] <= SPEC_BOUND[i], (i, worst)
    # every arm was reached
    assert arms["downhill"] > 50 and arms["flushed"] >= 20 and arms["near_flush"] >= 20 and arms["cancel"] >= 20, arms
    assert arms["zero_sign"] == {1.0} and arms["level"] >= 3, arms


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pot", POTS)
def test_reference_ordered_form_against_exact(measured, pot, dtype):
    """2(b): the reference-ordered form: j and grad j within c (2 + |dlogp| + |logq|) u relative (grad j: times terms),
    d logq / d sigma and g within their measured bounds."""
    _, worst, _ = measured[(pot, dtype)]
    print(f"reference form vs exact {pot} {dtype}: worst {worst}, bound {REF_BOUND}")
    for i in range(4):
        assert worst[i] <= REF_BOUND[i], (i, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pot", POTS)
def test_nonfinite_positions_follow_julias_min(pot, dtype):
    """x = NaN, +-Inf: dlogp is NaN, and min keeps it (gradients.jl:100-104): NaN in j and grad j, d logq / d sigma and g
    finite and within their bounds, the position what the reference's two additions leave."""
    for case in nonfinite_grid(dtype):
        s = X.sample(pot, *case, dtype)
        assert s.nan and s.j is None
        spec, xs, ref, xr = both_forms(pot, dtype, case)
        for got, bound in ((spec, SPEC_BOUND), (ref, REF_BOUND)):
            assert math.isnan(got[0]) and math.isnan(got[1]), (case, got)
            assert math.isfinite(got[2]) and math.isfinite(got[3]), (case, got)
            err, u = X.errors(got, s), X.units(s)
            assert err[2] <= bound[2] * u[2] and err[3] <= bound[3] * u[3], (case, got)
        for xa in (xs, xr):
            assert bits(xa) == bits(s.x_after) or (math.isnan(xa) and math.isnan(s.x_after)), (case, xa, s.x_after)


C3_BOUND = 0.5


@pytest.mark.parametrize("dtype", DTYPES)
def test_spec_d_carries_the_low_part_of_c3(dtype):
    """d logq / d sigma where the quadratic term dominates (3 <= |z| <= 8), against r c3 - 1 / sigma with
    c3 = dden / den^2 evaluated EXACTLY from the rounded den = 2 fl(sigma^2) both forms start from (ForwardDiff's order).
    Against the exact sigma^3 the rounding of sigma^2 alone costs up to one unit, which hides the low part of the c3 split from
    the bounds above; here only the chain's own roundings remain.  Measured worst 0.469 (Float64 state) and 0.468 (Float32
    state) u terms, bound the next power of two, 0.5; without the low part of c3 the worst is 1.06 / 1.07."""
    from fractions import Fraction
    rng = np.random.default_rng([GRID_SEED, 9, DTYPES.index(dtype)])
    worst = 0.0
    for i in range(3000):
        sigma = float(np.exp(rng.uniform(np.log(1e-3), np.log(10.0))))
        z = float(rng.uniform(3.0, 8.0)) * (1 if i % 2 else -1)
        x = as_state(rng.normal(0.0, 1.5), dtype)
        s = X.sample("harmonic", 2.0, sigma, z, x, dtype)
        got, _ = O.pg_summands("harmonic", 2.0, sigma, z, x, "spec", dtype)
        fs = Fraction(sigma)
        den = 2 * Fraction(float(np.float64(sigma) * np.float64(sigma)))
        quad = Fraction(s.r) * 4 * fs / (den * den)
        worst = max(worst, float(abs(Fraction(float(got[2])) - (quad - 1 / fs)) / (X.U * (quad + 1 / fs))))
    print(f"spec d vs exact at the rounded denominator, {dtype}: worst {worst}, bound {C3_BOUND}")
    assert worst <= C3_BOUND


# ---- whole estimator calls: the fold against the exact sum -----------------------------------------------------------------
#
# What a kind-Q column holds (amc_xsum.h): K = sum_i RN(lsb1(v_i) / 2^E) -- for grad j and g RN(lsb1(a_i) lsb1(b_i) / 2^E),
# the EXACT product rounded once -- and the value RN53(K 2^E).  Against the summand v_i the spec form defines, one deposit is
# off by at most
#     2^(E-1)            the rounding to a multiple of the quantum, to nearest
#   + 3 u |v_i|          lsb1 moves an operand by <= 1 ulp (two operands for a product), and the product columns take the
#                        unrounded product where the per-sample summand is its rounding (half an ulp),
# and the fold's value by u / 2 |value| more (the final rounding to 53 bits).  The deposit term is derived from the sum's
# definition, not measured; the per-sample bounds are SPEC_BOUND / REF_BOUND above.

def deposit_term(s, i, e_i):
    ex = s.exact()[i]
    return X.Decimal(2) ** (e_i - 1) + 3 * X._dec(X.U) * abs(X._dec(ex))


def sample_bounds(s, exponents):
    """Per column: (exact value, bound of the deposited spec summand, bound of the reference-ordered summand)."""
    assert not s.nan
    u, arg, ex = X.units(s), X.reference_argument(s), s.exact()
    out = []
    for i in range(4):
        v = X._dec(ex[i])
        if i < 2 and s.dlogp < X.FLUSH:                           # both forms give 0: off by the exact value itself
            spec = ref = abs(v)
        else:
            spec = SPEC_BOUND[i] * u[i] + (X.TINY if i < 2 else 0)
            ref = REF_BOUND[i] * u[i] * (arg if i < 2 else 1) + (X.TINY if i < 2 else 0)
        out.append((v, spec + deposit_term(s, i, exponents[i]), ref))
    return out


def fold_reference(*, potential, dtype, beta, sigma, seed, t_est, learn, q_batch, x, chain_offset=0):
    """Per learnable move and chain the exact column sums of that chain's q samples and the two bounds: arrays
    [n_learn][M][4] of (value, spec bound, reference bound), so that a call over the first m chains is a prefix sum."""
    samples, x_after = X.walk_call(O, potential=potential, beta=beta, sigma=sigma, seed=seed, t_est=t_est, learn=learn,
                                   q_batch=q_batch, x=x, chain_offset=chain_offset, dtype=dtype)
    out = []
    for l, lid in enumerate(learn):
        ex = O.gd_exponents(sigma[lid])
        rows = []
        for chain in samples[l]:
            acc = [[X.Decimal(0)] * 3 for _ in range(4)]
            for s in chain:
                for i, t in enumerate(sample_bounds(s, ex)):
                    acc[i] = [X.CTX.add(a, b) for a, b in zip(acc[i], t)]
            rows.append(acc)
        out.append(rows)
    return out, x_after


def check_fold(got, got_plain, per_chain, m, q_batch, where):
    """got: the rounded fold (n_learn, 5) of a call over the first m chains; got_plain: the reference-ordered summands folded
    left to right in Float64 (or None)."""
    u = X._dec(X.U)
    for l, rows in enumerate(per_chain):
        assert got[l][4] == m * q_batch, (where, got[l][4])
        if got_plain is not None:
            assert got_plain[l][4] == m * q_batch
        for i in range(4):
            exact = X.dsum(r[i][0] for r in rows[:m])
            bound = X.dsum(r[i][1] for r in rows[:m]) + u / 2 * abs(X.Decimal(float(got[l][i])))
            err = abs(X.Decimal(float(got[l][i])) - exact)
            assert err <= bound, (where, l, i, float(err), float(bound), got[l][i])
            if got_plain is not None:
                # the left-to-right Float64 fold of n summands adds at most (n - 1) u / 2 sum |v_i| (1 + ...) of its own
                n = m * q_batch
                ref_bound = X.dsum(r[i][2] for r in rows[:m])
                size = X.dsum(abs(r[i][0]) for r in rows[:m]) + ref_bound
                err = abs(X.Decimal(float(got_plain[l][i])) - exact)
                assert err <= ref_bound + n * u / 2 * size * (1 + n * u), (where, "plain", l, i, float(err), float(ref_bound))


FOLD_SIGMA = (0.35, 0.02, 3.0)            # a K = 3 pool; learn = [2, 0]
FOLD_M = (1, 2, 63, 65, 4099)


def fold_case(pot, dtype, M):
    rng = np.random.default_rng([GRID_SEED, 5, POTS.index(pot), DTYPES.index(dtype)])
    x = rng.normal(0.0, 1.5, max(FOLD_M))[:M]
    return dict(potential=pot, dtype=dtype, beta=2.0, sigma=list(FOLD_SIGMA), seed=77 + POTS.index(pot)), \
        np.array([as_state(v, dtype) for v in x])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pot", POTS)
def test_fold_bound_holds_for_the_spec_twin(pot, dtype):
    """The bound the device test uses for whole calls (test_gpu_pg_exact.py::test_fold_against_the_exact_sum), confirmed here
    with the oracle's fold in the device's place: sum of the per-sample bounds plus the kind-Q deposit term."""
    M, offset, learn = 65, 2 ** 20 + 2, [2, 0]
    kw, x = fold_case(pot, dtype, M)
    for q in (1, 3, 20):
        per_chain, x_after = fold_reference(learn=learn, q_batch=q, x=x, chain_offset=offset, t_est=0, **kw)
        for m in (1, 2, 63, 65):
            sims = []
            for _ in range(2):
                o = O.OracleSim(m, chain_offset=offset, weight=[0.5, 0.25, 0.25], **kw)
                o.set_x(x[:m])
                sims.append(o)
            check_fold(sims[0].pg_estimate(learn, q), sims[1].pg_estimate_plain(learn, q), per_chain, m, q, (pot, dtype, q, m))
            for o in sims:
                assert np.array_equal(o.state()[0].view(np.uint64), np.array(x_after[:m]).view(np.uint64))
                o.close()
