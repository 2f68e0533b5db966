"""``run(...)`` with an ``Autocorrelation`` on the device, end to end: fused and stepwise runs and a checkpointed, resumed run hold the
same records bit for bit, and one check of meaning -- tau_int of the energy from the device's records against plain numpy on the
positions the same run downloaded, and the order of tau_int at two proposal widths."""
import numpy as np
import pytest

import montecarlo_amd as ma

pytestmark = pytest.mark.gpu
M, BETA = 1 << 16, 2.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def equilibrium():
    return np.random.default_rng(77).normal(0.0, np.sqrt(1.0 / (2.0 * BETA)), M)        # harmonic, U = x^2: x ~ N(0, 1 / (2 beta))


class KeepPositions(ma.AriannaAlgorithm):
    """The positions at its scheduled times, downloaded (what a user did before the sums lived on the device)."""

    def __init__(self, chains, dependencies=None, **extras):
        self.metropolis, self.rows = dependencies[0], []

    def make_step(self, simulation):
        self.rows.append(self.metropolis.engine.download_state(want_e=False)[0].copy())


def build(path, steps, scheduler, n_lags, sigma=0.4, origins=1, keep=False, x=None, m=4099):
    chains = ma.ParticleChains(m if x is None else x.size, BETA, "harmonic", x=x, init_uniform=None if x is not None else (-1.0, 1.0))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [sigma], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=9),
          dict(algorithm=ma.Autocorrelation, dependencies=(ma.Metropolis,), scheduler=scheduler, observable="energy", n_lags=n_lags, origins=origins)]
    if keep:
        al.append(dict(algorithm=KeepPositions, dependencies=(ma.Metropolis,), scheduler=scheduler))
    return ma.Simulation(chains, al, steps, path=str(path))


def test_fused_and_stepwise_runs_hold_the_same_records(gpu, tmp_path):
    recs = []
    for fuse in (True, False):
        sim = build(tmp_path / str(fuse), 40, list(range(4, 41, 4)), n_lags=4, origins=2)
        ma.run(sim, fuse=fuse)
        ac = sim.algorithms[1]
        recs.append(ac.records())
        assert ac.origins_done == 2 and np.array_equal(ac.lags(), [0, 4, 8, 12, 16]) and ac.tau_int()[0].shape == (1,)
    assert recs[0].shape == (5, 1, 3, 12) and np.array_equal(bits(recs[0]), bits(recs[1]))


@pytest.mark.parametrize("cut", [10, 20, 26])
def test_a_checkpointed_and_resumed_run_ends_on_the_same_records(gpu, tmp_path, cut):
    sched = list(range(4, 41, 4))
    whole = build(tmp_path / "w", 40, sched, n_lags=4, origins=2)
    ma.run(whole)
    first = build(tmp_path / "a", cut, [t for t in sched if t <= cut], n_lags=4, origins=2)
    ma.run(first)
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    second = build(tmp_path / "b", 40 - cut, [t - cut for t in sched if t > cut], n_lags=4, origins=2)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = second.algorithms[1], whole.algorithms[1]
    assert np.array_equal(bits(a.records()), bits(b.records())) and np.array_equal(a.lags(), b.lags()) and a.origins_done == 2
    assert np.array_equal(bits(second.chains.x), bits(whole.chains.x))


def numpy_rho(rows):
    """rho(k) of the energy by plain numpy from downloaded positions: the estimator of Autocorrelation.rho restated."""
    e = [x * x for x in rows]
    a = e[0]
    out = []
    for o in e:
        cov = np.mean(a * o) - np.mean(a) * np.mean(o)
        out.append(cov / np.sqrt((np.mean(a * a) - np.mean(a) ** 2) * (np.mean(o * o) - np.mean(o) ** 2)))
    return np.array(out)[None, :]


def test_tau_int_means_what_it_says(gpu, tmp_path):
    """M = 2^16 harmonic chains at beta = 2 from equilibrium.  The device's tau_int agrees with numpy's from the same run's positions
    to 1e-12 relative -- a bound on arithmetic (kind-R rounding against numpy's pairwise summation, both good to the last place or
    two), not on statistics -- and the narrow width decorrelates more slowly than the wide one."""
    taus = {}
    for sigma, every, n_lags in ((0.1, 40, 60), (1.0, 1, 40)):
        sched = [every * (k + 1) for k in range(n_lags + 1)]
        sim = build(tmp_path / str(sigma), sched[-1], sched, n_lags, sigma=sigma, keep=True, x=equilibrium())
        ma.run(sim)
        ac, kept = sim.algorithms[1], sim.algorithms[2]
        tau, window, converged = ac.tau_int()
        ref = ma.tau_from_rho(numpy_rho(kept.rows), float(every))
        print("sigma", sigma, "tau", tau[0], "numpy", ref[0][0], "window", window[0], "converged", converged[0])
        assert window[0] == ref[1][0] and converged[0] == ref[2][0]
        assert abs(tau[0] - ref[0][0]) <= 1e-12 * abs(ref[0][0])
        assert np.allclose(ac.rho(), numpy_rho(kept.rows), rtol=0, atol=1e-11)
        taus[sigma] = tau[0]
    assert taus[0.1] > taus[1.0]
