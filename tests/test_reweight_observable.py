"""reweighting.reweight_observable on the CPU (DESIGN.md section 3.17 "Moments per bin"): an observable that is no function of the
energy, reweighted to any beta from its sums per bin and WHAM's density of states."""
import numpy as np
import pytest

from montecarlo_amd import reweighting as rw

LO, HI, N = 0.0, 6.0, 240
E = rw.bin_centres(LO, HI, N)
EDGES = LO + (HI - LO) / N * np.arange(N + 1)


def harmonic_bins():
    """The harmonic well e = x^2: bin [a, b) is |x| in [sqrt a, sqrt b).  g_b = its length in x, and the microcanonical mean of x^2
    over it, the integral of x^2 dx over the integral of dx = (b^1.5 - a^1.5) / (3 (sqrt b - sqrt a))."""
    ra, rb = np.sqrt(EDGES[:-1]), np.sqrt(EDGES[1:])
    return 2.0 * (rb - ra), (rb ** 3 - ra ** 3) / (3.0 * (rb - ra))


def expected_rows(betas, n_per_row, g, mean):
    """Exact expected counts n_kb = N_k g_b exp(-beta_k E_b) / Z_k of the binned model and the sums S_kb = n_kb o_b."""
    w = g[None, :] * np.exp(-np.outer(betas, E))
    counts = np.asarray(n_per_row, dtype=np.float64)[:, None] * w / w.sum(axis=1, keepdims=True)
    return counts, counts * mean[None, :]


def test_one_row_reweighted_to_its_own_beta_returns_the_plain_mean():
    """g_b is proportional to n_b exp(beta E_b), so the weights at beta are n_b / N: sum_b S_b / N, whatever the sums are."""
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 5000, size=(1, N)).astype(np.float64)
    counts[0, ::7] = 0.0
    sums = rng.normal(size=(1, N)) * counts
    beta = np.array([1.3])
    log_g, _, _ = rw.wham(counts, beta, E)
    got = rw.reweight_observable(log_g, E, beta, sums, counts)
    assert got.shape == (1,) and got[0] == pytest.approx(sums.sum() / counts.sum(), rel=0, abs=1e-12)
    assert rw.reweight_observable(log_g, E, 1.3, sums[0], counts[0]) == pytest.approx(sums.sum() / counts.sum(), rel=0, abs=1e-12)      # scalar beta, one row as 1-d


def test_two_rows_of_the_harmonic_well_give_the_binned_expectation_between_them():
    g, mean = harmonic_bins()
    betas = np.array([1.0, 2.0])
    counts, sums = expected_rows(betas, [3.0e6, 5.0e6], g, mean)
    log_g, f, _ = rw.wham(counts, betas, E)
    for beta in (1.0, 1.4, 2.0, np.array([1.2, 1.7])):
        w = g[None, :] * np.exp(-np.outer(np.atleast_1d(beta), E))
        want = (w @ mean) / w.sum(axis=1)
        got = rw.reweight_observable(log_g, E, beta, sums, counts)
        assert np.shape(got) == np.shape(beta) and np.allclose(got, want.reshape(np.shape(beta)), rtol=0, atol=1e-9)
    # <x^2> = 1 / (2 beta) in the continuum: the bins of width 0.025 come within a few 1e-3 of it
    assert rw.reweight_observable(log_g, E, 1.4, sums, counts) == pytest.approx(1.0 / 2.8, abs=5e-3)


def test_the_constant_observable_returns_one():
    g, _ = harmonic_bins()
    betas = np.array([0.8, 1.6, 3.0])
    counts, _ = expected_rows(betas, [1e5, 2e5, 3e5], g, np.ones(N))
    log_g, _, _ = rw.wham(counts, betas, E)
    got = rw.reweight_observable(log_g, E, np.linspace(0.8, 3.0, 7), counts, counts)
    assert np.allclose(got, 1.0, rtol=0, atol=1e-14)


def test_empty_bins_take_no_part_and_nothing_left_is_nan():
    g, mean = harmonic_bins()
    betas = np.array([1.0, 2.0])
    counts, sums = expected_rows(betas, [1e6, 1e6], g, mean)
    dead = np.zeros(N, dtype=bool)
    dead[150:] = True
    dead[10:14] = True                                    # a hole inside the support and the whole upper end
    counts[:, dead] = 0.0
    sums_dirty = sums.copy()
    sums_dirty[:, dead] = np.nan                          # whatever stands in the sums of an empty bin is never read
    log_g, _, _ = rw.wham(counts, betas, E)
    assert np.all(np.isneginf(log_g[dead]))
    w = np.where(dead, 0.0, g)[None, :] * np.exp(-np.outer([1.5], E))
    want = (w[:, ~dead] @ mean[~dead]) / w.sum(axis=1)
    got = rw.reweight_observable(log_g, E, np.array([1.5]), sums_dirty, counts)
    assert np.isfinite(got[0]) and got[0] == pytest.approx(want[0], rel=0, abs=1e-9)
    # a bin with counts but a density of states the caller has removed takes no part either
    lg2 = log_g.copy()
    lg2[:20] = -np.inf
    keep = ~dead & (np.arange(N) >= 20)
    want2 = (w[0, keep] @ mean[keep]) / w[0, keep].sum()
    assert rw.reweight_observable(lg2, E, 1.5, sums_dirty, counts) == pytest.approx(want2, rel=0, abs=1e-9)
    # nothing left: NaN of the betas' shape, no warning turned error
    none = rw.reweight_observable(np.full(N, -np.inf), E, np.array([1.0, 2.0]), sums, np.zeros_like(counts))
    assert none.shape == (2,) and np.all(np.isnan(none))


def test_shapes_are_checked():
    with pytest.raises(ValueError, match="reweight_observable"):
        rw.reweight_observable(np.zeros(N), E, 1.0, np.zeros((2, N)), np.zeros((3, N)))
    with pytest.raises(ValueError, match="reweight_observable"):
        rw.reweight_observable(np.zeros(N - 1), E, 1.0, np.zeros((2, N)), np.zeros((2, N)))


def test_signed_sums_cross_ranks_as_exact_halves(monkeypatch):
    """EnergyHistogram.moment_sums sends the signed 64-bit cells through the Float64 all-reduce as the two halves of their two's
    complement and puts them together modulo 2^64: two ranks holding the same cells give exactly twice each, negatives and cells
    beyond 2^53 included."""
    from montecarlo_amd import energy_histogram as eh_mod, sharding

    class Met:
        world_size, engine = 2, None

    eh = eh_mod.EnergyHistogram.__new__(eh_mod.EnergyHistogram)
    eh.metropolis = Met()
    monkeypatch.setattr(sharding, "allreduce_sum", lambda values, engine: 2.0 * np.asarray(values, dtype=np.float64))
    local = np.array([[0, 1, -1, 2 ** 32, -(2 ** 32), 2 ** 61 + 12345, -(2 ** 61) - 12345, 2 ** 31 - 1, -(2 ** 31), 987654321987]], dtype=np.int64)
    total = eh._all_ranks(local.view(np.uint64)).view(np.int64)
    assert total.shape == local.shape and np.array_equal(total, 2 * local)
    q = eh_mod.emom_quanta
    for bound, eb in ((4.0, 3), (3.7, 2), (0.3, -1), (1.0, 1), (0.5, 0), (2.0 ** -40, -39)):
        assert q(bound) == {1: 2.0 ** (eb - 32), 2: 2.0 ** (2 * eb - 32), 4: 1.0}, bound
