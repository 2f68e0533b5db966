"""Multiple-histogram reweighting on the host (montecarlo_amd/reweighting.py): exact recovery on a discrete
model, the single-histogram case, invariances, refusals, and EnergyHistogram's max_outside refusal over the engine_factory seam.
No GPU."""
import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd import reweighting as rw

import anneal_twin as A
import ehist_stat as S
import ehist_twin as T

EPS = np.finfo(np.float64).eps


def _model():
    """40 bins, K = 5: g_b, E_b, beta_k, N_k and the exact expected counts N_k g_b exp(-beta_k E_b) / Z_k."""
    e = rw.bin_centres(0.0, 4.0, 40)
    g = 5.0 * np.exp(-0.3 * (e - 2.0) ** 2) * (1.0 + 0.5 * np.sin(3.0 * e))
    betas = np.array([0.5, 0.8, 1.2, 1.7, 2.5])
    z = (g[None, :] * np.exp(-np.outer(betas, e))).sum(axis=1)
    n_k = np.array([1.0e5, 2.0e5, 1.5e5, 1.0e5, 3.0e5])
    counts = n_k[:, None] * g[None, :] * np.exp(-np.outer(betas, e)) / z[:, None]
    return e, g, betas, z, counts


def test_exact_recovery_on_a_discrete_model():
    """With the exact expected counts the WHAM equations hold at the true (g, f): the iteration's fixed point IS the truth, and what is
    left at the stop is the iteration's own error.  The iteration contracts linearly, |d_(n+1)| <= rho |d_n| for the step d_n, so the
    distance to the fixed point at a stop with |d_n| < tol is at most tol rho / (1 - rho).  rho is read off two runs: tightening tol by
    10^-4 costs m more iterations, so rho^m ~ 10^-4; the counts of iterations are integers, hence rho <= 10^(-4 / (m + 1)).  f is
    reported relative to f_0, which carries the same error: a factor 2.  Rounding adds a few ulp of the largest |f|."""
    e, g, betas, z, counts = _model()
    tol = 1e-12
    _, _, it_loose = rw.wham(counts, betas, e, tol=1e-8)
    log_g, f, it = rw.wham(counts, betas, e, tol=tol)
    m = it - it_loose
    assert 1 <= m <= 40, (it_loose, it)
    rho = 10.0 ** (-4.0 / (m + 1))
    truth = -np.log(z / z[0])
    bound = 2.0 * tol * rho / (1.0 - rho) + 64 * EPS * np.max(np.abs(truth))
    print("iterations", it_loose, it, "rho <=", rho, "bound", bound, "max |f - truth|", np.max(np.abs(f - truth)))
    assert f[0] == 0.0
    assert np.max(np.abs(f - truth)) <= bound
    # log g up to ONE additive constant: the spread of the difference is twice the error of a single value at most
    d = log_g - np.log(g)
    assert np.ptp(d) <= 2.0 * bound
    # ... and the constant is the normalisation log Z(beta_0) = 0
    log_z = rw.reweight(log_g, e, betas)[0]
    assert np.max(np.abs(log_z + truth)) <= 2.0 * bound and abs(log_z[0]) <= bound


def test_single_histogram_returns_its_own_moments():
    """K = 1 at the row's own beta: log g_b - beta E_b = log n_b - log N, so the weights are n_b / N up to one log and one exp each --
    relative errors of (|log n_b| + 2) ulp at most -- and the moments are the histogram's own to a few ulp of the sums."""
    rng = np.random.default_rng(5)
    e = rw.bin_centres(0.0, 3.0, 64)
    n = rng.integers(0, 5000, size=64).astype(np.float64)
    n[[3, 40]] = 0.0
    beta = 1.3
    log_g, f, it = rw.wham(n[None, :], [beta], e)
    assert f[0] == 0.0 and it <= 2
    _, m1, m2, c = rw.reweight(log_g, e, beta)
    p = n / n.sum()
    mean = np.sum(p * e)
    var = np.sum(p * (e - mean) ** 2)
    rel = (np.log(n.max()) + beta * e.max() + 4.0) * 4.0 * EPS      # of one weight: a log, an exp and their arguments' roundings
    assert abs(m1 - mean) <= rel * np.sum(p * np.abs(e)) + 4 * EPS * abs(mean)
    assert abs((m2 - m1 * m1) - var) <= 8 * rel * np.sum(p * e * e)
    assert abs(c - beta * beta * var) <= 8 * rel * beta * beta * np.sum(p * e * e)


def test_invariant_under_permuting_the_rows():
    e, g, betas, z, counts = _model()
    perm = np.array([3, 0, 4, 2, 1])
    log_g, f, _ = rw.wham(counts, betas, e, tol=1e-13)
    log_g_p, f_p, _ = rw.wham(counts[perm], betas[perm], e, tol=1e-13)
    # other row first: another normalisation (f_p[0] = 0) of the same solution
    assert np.max(np.abs((f_p - f_p[np.argmax(perm == 0)]) - f[perm])) <= 1e-12
    grid = np.linspace(0.5, 2.5, 9)
    a, b = rw.reweight(log_g, e, grid), rw.reweight(log_g_p, e, grid)
    for i in (1, 2, 3):                             # <e>, <e^2>, C do not see the normalisation
        assert np.max(np.abs(a[i] - b[i])) <= 1e-11 * np.max(np.abs(a[i]))


def test_bins_empty_everywhere_change_nothing():
    e, g, betas, z, counts = _model()
    wide_e = rw.bin_centres(0.0, 5.0, 50)           # the same 40 bins, and 10 more nobody visited
    wide = np.concatenate([counts, np.zeros((5, 10))], axis=1)
    log_g, f, it = rw.wham(counts, betas, e)
    log_g_w, f_w, it_w = rw.wham(wide, betas, wide_e)
    assert np.allclose(wide_e[:40], e, rtol=0, atol=4 * EPS * 5)
    assert np.all(log_g_w[40:] == -np.inf) and np.all(np.isfinite(log_g_w[:40]))
    assert it_w == it and np.max(np.abs(f_w - f)) <= 1e-13 and np.max(np.abs(log_g_w[:40] - log_g)) <= 1e-12
    out = rw.reweight(log_g_w, wide_e, [0.7, 1.9])
    assert all(np.all(np.isfinite(v)) for v in out)


def test_refusals():
    e = rw.bin_centres(0.0, 1.0, 10)
    left, right = np.zeros(10), np.zeros(10)
    left[:4], right[6:] = 10.0, 10.0
    with pytest.raises(ValueError, match="not connected"):
        rw.wham(np.stack([left, right]), [1.0, 2.0], e)
    mid = np.zeros(10)
    mid[3:7] = 5.0
    rw.wham(np.stack([left, right, mid]), [1.0, 2.0, 1.5], e)      # the third row links them
    _, _, betas, _, counts = _model()
    with pytest.raises(ValueError, match="no convergence"):
        rw.wham(counts, betas, rw.bin_centres(0.0, 4.0, 40), tol=1e-15, max_iter=3)
    with pytest.raises(ValueError, match="no count inside"):
        rw.wham(np.stack([left, np.zeros(10)]), [1.0, 2.0], e)
    with pytest.raises(ValueError):
        rw.wham(np.stack([left, right]), [1.0], e)


def test_outside_share():
    c = np.array([[5, 3, 1, 1, 0], [0, 0, 0, 0, 0]], dtype=np.uint64)
    s = rw.outside_share(c)
    assert np.array_equal(s, np.array([[0.1, 0.1, 0.0], [0.0, 0.0, 0.0]]))


class EhistTwinEngine(A.AnnealTwinEngine):
    """anneal_twin.AnnealTwinEngine plus the energy-histogram surface of montecarlo_amd._capi.HipEngine, computed by ehist_twin (no
    ladder: one group)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.potential = kw.get("potential", "harmonic")
        self._ehist = None

    def energy_histogram_accumulate(self, lo, hi, n_bins):
        if self._ehist is None:
            self._ehist = dict(bins=(float(lo), float(hi), int(n_bins)), counts=np.zeros((1, int(n_bins) + 3), dtype=np.uint64), n=0)
        assert self._ehist["bins"] == (float(lo), float(hi), int(n_bins))
        self._ehist["counts"] += T.snapshot(self.potential, self.download_state(want_e=False)[0], lo, hi, n_bins)
        self._ehist["n"] += 1

    def energy_histogram_fetch(self, reset=False):
        h = self._ehist
        if h is None:
            return np.zeros((1, 0), dtype=np.uint64), 0, (0.0, 0.0, 0)
        if reset:
            self._ehist = None
        return h["counts"].copy(), h["n"], h["bins"]

    def set_energy_histogram(self, lo=0.0, hi=0.0, n_bins=0, counts=None, n_snapshots=0):
        self._ehist = None if counts is None or not n_snapshots else dict(
            bins=(float(lo), float(hi), int(n_bins)), counts=np.array(counts, dtype=np.uint64).reshape(1, -1), n=int(n_snapshots))


def _run(hi, max_outside, tmp_path):
    chains = ma.ParticleChains.uniform(64, 2.0)
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=5, engine_factory=EhistTwinEngine),
          dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(8, 0, 2), lo=0.0, hi=hi, n_bins=16,
               max_outside=max_outside)]
    sim = ma.Simulation(chains, al, 8, path=str(tmp_path))
    ma.run(sim)
    return sim.algorithms[1]


def test_energy_histogram_refuses_what_lies_outside(oracle, tmp_path):
    eh = _run(0.05, 0.0, tmp_path / "a")            # nearly every energy lies at or above hi = 0.05
    counts = eh.counts()
    assert counts.shape == (1, 19) and counts.sum() == eh.n_snapshots * 64 and eh.n_snapshots >= 4
    assert counts[0, 17] > 0
    with pytest.raises(ValueError, match=r"rung 0 .*at or above hi.*widen"):
        eh.reweight([2.0])
    with pytest.raises(ValueError, match="at or above hi"):
        eh.free_energies()
    wide = _run(1.0e3, 0.0, tmp_path / "b")         # everything inside: single-histogram reweighting around the shared beta
    log_z, m1, m2, c = wide.reweight(np.array([2.0]))
    p = wide.counts()[0, :16] / wide.counts()[0, :16].sum()
    assert abs(log_z[0]) <= 1e-12 and abs(m1[0] - np.sum(p * wide.energies())) <= 1e-9
    loose = _run(0.05, 1.0, tmp_path / "c")         # a caller who accepts the loss is served
    assert np.all(np.isfinite(loose.reweight([2.0])[1]))


# ---- PopulationAnnealing(energy_histogram=...) over the same seam ---------------------------------------------------------------------------
def _anneal(path, steps, betas, hist, every=2):
    chains = ma.ParticleChains.uniform(96, betas[0], potential="double_well")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=4, engine_factory=EhistTwinEngine),
          dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, every), betas=betas[1:],
               energy_histogram=hist)]
    return ma.Simulation(chains, al, steps, path=str(path))


def test_annealing_keeps_a_histogram_per_temperature(oracle, tmp_path):
    """Every stored row is the twin's histogram of the state in front of that annealing step (here: of a twin stepped by hand), the
    last one of the state at finalise; reweight is finite along the schedule; a checkpoint carries the list without finalise's row."""
    betas = [0.5, 0.8, 1.2, 1.7]
    hist = dict(lo=0.0, hi=64.0, n_bins=32)
    sim = _anneal(tmp_path / "w", 6, betas, hist)
    ma.run(sim)
    pa = sim.algorithms[1]
    b, counts = pa.histograms()
    assert np.array_equal(b, betas) and counts.shape == (4, 35) and counts.dtype == np.uint64
    assert np.array_equal(counts.sum(axis=1), np.full(4, 96, dtype=np.uint64))
    ref = A.AnnealTwinEngine(n_chains=96, potential="double_well", beta=0.5, sigma=[0.5], weight=[1.0], seed=4)
    ref.init_uniform(-2.0, 2.0)
    for i, beta_new in enumerate(betas[1:]):
        ref.sweep(2)
        assert np.array_equal(counts[i], T.snapshot("double_well", ref.download_state(want_e=False)[0], 0.0, 64.0, 32)[0]), i
        ref.anneal(beta_new)
    assert np.array_equal(counts[3], T.snapshot("double_well", ref.download_state(want_e=False)[0], 0.0, 64.0, 32)[0])
    log_z, m1, m2, c = pa.reweight(np.linspace(0.5, 1.7, 7))
    assert all(np.all(np.isfinite(v)) for v in (log_z, m1, m2, c)) and abs(log_z[0]) < 1e-9
    assert sim.algorithms[0].engine.energy_histogram_fetch()[2] == (0.0, 0.0, 0)       # nothing is left in the engine's accumulator
    st = pa.histogram_state()
    assert np.array_equal(st["anneal_hist_betas"], betas[:3]) and st["anneal_hist_counts"].shape == (3, 35)
    # resume: two steps, checkpoint, the rest -- the same list as the whole run's
    first = _anneal(tmp_path / "a", 4, betas, hist)
    ma.run(first)
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    second = _anneal(tmp_path / "b", 2, betas, hist)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    b2, counts2 = second.algorithms[1].histograms()
    assert np.array_equal(b2, b) and np.array_equal(counts2, counts)


def test_annealing_histogram_refusals(oracle, tmp_path):
    betas = [0.5, 1.0]
    with pytest.raises(ValueError, match="energy_histogram.*'n_bins'.*missing"):
        _anneal(tmp_path / "a", 2, betas, dict(lo=0.0, hi=1.0))
    with pytest.raises(ValueError, match="unknown keys"):
        _anneal(tmp_path / "b", 2, betas, dict(lo=0.0, hi=1.0, n_bins=4, bins=3))
    with pytest.raises(ValueError, match="finite lo < hi"):
        _anneal(tmp_path / "c", 2, betas, dict(lo=1.0, hi=1.0, n_bins=4))
    tight = _anneal(tmp_path / "d", 2, betas, dict(lo=0.0, hi=0.01, n_bins=4))
    ma.run(tight)
    with pytest.raises(ValueError, match=r"temperature 0.*at or above hi.*widen"):
        tight.algorithms[1].reweight([0.7])
    plain = _anneal(tmp_path / "e", 2, betas, None)          # without the option nothing is taken
    ma.run(plain)
    with pytest.raises(ValueError, match="needs the histograms"):
        plain.algorithms[1].histograms()
    # an EnergyHistogram beside a PopulationAnnealing points at the option
    chains = ma.ParticleChains.uniform(32, 0.5, potential="double_well")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=4, engine_factory=EhistTwinEngine),
          dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=[2], betas=[1.0]),
          dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), scheduler=[2], lo=0.0, hi=1.0, n_bins=4)]
    with pytest.raises(ValueError, match="energy_histogram=dict"):
        ma.run(ma.Simulation(chains, al, 2, path=str(tmp_path / "f")))


# ---- the exact side of the statistical GPU test (tests/ehist_stat.py) ------------------------------------------------------------------------
def test_the_statistical_tests_bins_hold_every_sample():
    """hi is chosen so that the quadrature probability of e >= hi at the hottest rung, times every sample of the run, is below 1e-6:
    max_outside = 0 then holds for the truth alone.  The exact bin probabilities are probabilities, and the quadrature behind them
    agrees with scipy's on the partition function."""
    from scipy import integrate
    p_tail = S.tail_weight(S.BETAS[0]) / (S.bin_weights(S.BETAS[0]).sum() + S.tail_weight(S.BETAS[0]))
    print("P(e >= hi) at beta", S.BETAS[0], "=", p_tail, "x", S.N_SAMPLES, "samples =", p_tail * S.N_SAMPLES)
    assert S.BETAS[0] == S.BETAS.min() and 0.0 < p_tail * S.N_SAMPLES < 1e-6
    p = S.bin_probabilities()
    assert p.shape == (S.R, S.N_BINS) and np.all(p >= 0) and np.all(np.abs(p.sum(axis=1) - 1.0) <= 1e-13)
    for b in (S.BETAS[0], S.BETAS[-1]):
        z = integrate.quad(lambda x: np.exp(-b * S.potential(x)), -6.0, 6.0, epsabs=1e-14, epsrel=1e-13)[0]
        assert abs(S.bin_weights(b).sum() + S.tail_weight(b) - z) <= 1e-12 * z
    # the large-sample limit of the binned estimator against the continuum: the binning bias at this bin width, recorded in
    # profiles/energy_histogram.md and asserted nowhere
    energies = rw.bin_centres(S.LO, S.HI, S.N_BINS)
    truth = S.theta(p, rw.wham, rw.reweight, energies)
    log_z = S.continuum(S.BETAS)[0]
    print("binning bias, f_r - f_0:", truth[:S.R - 1] + (log_z[1:] - log_z[0]))
    print("binning bias, C:", truth[S.R - 1:] - S.continuum(S.TARGET_BETAS)[2])
