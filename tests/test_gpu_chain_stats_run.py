"""``run(...)`` with a ``Convergence`` on the device, end to end: the diagnostic says what it is meant to say -- cold double-well chains
started in both wells are NOT converged in x although their energies are, harmonic chains past their burn-in are --, a checkpointed
and resumed run holds the uninterrupted one's bits, and ``callback_rhat`` writes its rows."""
import numpy as np
import pytest

import montecarlo_amd as ma

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def build(path, x, beta, potential, sigma, sched, steps, observable="x", n_samples=None, extra=(), seed=9):
    chains = ma.ParticleChains(x.size, beta, potential, x=x)
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [sigma], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=seed),
          dict(algorithm=ma.Convergence, dependencies=(ma.Metropolis,), scheduler=sched, observable=observable,
               n_samples=len(sched) if n_samples is None else n_samples)]
    return ma.Simulation(chains, al + list(extra), steps, path=str(path))


def test_non_convergence_is_detected(gpu, tmp_path):
    """4096 double-well chains at beta = 8, sigma = 0.1, half started at x = -1 and half at x = +1; 32 samples four sweeps apart.  The
    variance within a well is about 1 / (beta V'') = 1/64 and the wells are 2 apart: split R-hat of x is about 8 to 10, and
    crossings at e^-8 per attempt cannot close the gap in 128 sweeps.  The energy is blind to the wells."""
    x0 = np.where(np.arange(4096) % 2 == 0, -1.0, 1.0)
    sched = [4 * (k + 1) for k in range(32)]
    out = {}
    for kind in ("x", "energy"):
        sim = build(tmp_path / kind, x0, 8.0, "double_well", 0.1, sched, sched[-1], observable=kind)
        ma.run(sim)
        cv = sim.algorithms[1]
        assert cv.counts() == (16, 16)
        out[kind] = (cv.rhat()[0], cv.rhat(split=False)[0], cv.tau_int_batch()[0])
        print(kind, "split R-hat", out[kind][0], "unsplit", out[kind][1], "tau_int_batch (samples)", out[kind][2])
    assert out["x"][0] > 2.0 and out["x"][1] > 2.0
    assert out["energy"][0] < 1.2


def test_convergence_is_recognised(gpu, tmp_path):
    """65 536 harmonic chains at beta = 2, sigma = 1, 200 sweeps of burn-in, 64 samples twenty sweeps apart.  For independent samples
    R-hat^2 - 1 has a standard deviation of about 2e-4 here, and the residual correlation at twenty sweeps adds (2 tau - 1) / n; the
    twin engine at 4096 chains stays within 0.005 (tests/test_chain_stats_host.py), so 0.01 is a condition, not a measurement."""
    x0 = np.random.default_rng(11).uniform(-1.0, 1.0, 1 << 16)
    sched = [200 + 20 * (k + 1) for k in range(64)]
    sim = build(tmp_path, x0, 2.0, "harmonic", 1.0, sched, sched[-1])
    ma.run(sim)
    cv = sim.algorithms[1]
    r, tau = cv.rhat()[0], cv.tau_int_batch()[0]
    print("split R-hat", r, "unsplit", cv.rhat(split=False)[0], "tau_int_batch (samples)", tau)
    assert cv.counts() == (32, 32)
    assert abs(r - 1.0) < 0.01


@pytest.mark.parametrize("cut", [10, 22, 30])
def test_a_checkpointed_and_resumed_run_ends_on_the_same_bits(gpu, tmp_path, cut):
    x0 = np.where(np.arange(4099) % 2 == 0, -1.0, 1.0) * (0.8 + 0.4 * ((np.arange(4099) * 0.6180339887498949) % 1.0))
    sched = list(range(4, 41, 4))[:8]
    args = (2.0, "double_well", 0.4)
    whole = build(tmp_path / "w", x0, *args, sched, 40, observable="energy", n_samples=8)
    ma.run(whole)
    first = build(tmp_path / "a", x0, *args, [t for t in sched if t <= cut], cut, observable="energy", n_samples=8)
    ma.run(first)
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    second = build(tmp_path / "b", x0, *args, [t - cut for t in sched if t > cut], 40 - cut, observable="energy", n_samples=8)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = second.algorithms[1], whole.algorithms[1]
    assert a.counts() == b.counts() == (4, 4)
    assert np.array_equal(bits(a.records()), bits(b.records()))
    assert np.array_equal(bits(a.metropolis.engine.chain_stats_sums()), bits(b.metropolis.engine.chain_stats_sums()))
    assert np.array_equal(bits(a.rhat()), bits(b.rhat())) and np.array_equal(bits(second.chains.x), bits(whole.chains.x))


def test_callback_rhat_rows_are_written(gpu, tmp_path):
    R, L = 3, 512
    x0 = np.where(np.arange(R * L) // R % 2 == 0, 1.0, -1.0)
    chains = ma.ParticleChains.ladder(L, [1.0, 4.0, 8.0], potential="double_well", x=x0)
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.3], 1.0),)
    sched = [2 * (k + 1) for k in range(8)]
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=5),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=list(range(1, 21))),
          dict(algorithm=ma.Convergence, dependencies=(ma.Metropolis,), scheduler=sched, observable="x", n_samples=8),
          dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_rhat,), scheduler=[8, 16, 20])]
    sim = ma.Simulation(chains, al, 20, path=str(tmp_path))
    ma.run(sim)
    rows = open(tmp_path / "rhat.dat").read().splitlines()
    assert [r.split()[0] for r in rows] == ["0", "8", "16", "20"]          # (StoreCallbacks writes the row of t = 0 itself)
    # nothing accumulated, then half a window: NaN; the full window: one value per rung, the same at every later time
    assert "NaN" in rows[0] and "NaN" in rows[1] and "NaN" not in rows[2] and rows[2].split(None, 1)[1] == rows[3].split(None, 1)[1]
    assert np.allclose(sim.algorithms[2].rhat(), [float(v) for v in rows[2].split("[")[1].rstrip("]").split(",")])
