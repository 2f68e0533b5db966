"""``run(...)`` with an ``EnergyHistogram`` on the device, end to end: fused and stepwise runs and a checkpointed, resumed run hold the
same counts, integer for integer, the counts equal the host twin applied to the positions the same run downloaded, and the reweighted
curve is finite between the rungs."""
import numpy as np
import pytest

import montecarlo_amd as ma

import ehist_stat as S
import ehist_twin as T

pytestmark = pytest.mark.gpu
R, L = 4, 131
BETAS = 0.5 * 1.5 ** np.arange(R)
BINS = dict(lo=0.0, hi=40.0, n_bins=160)


class KeepPositions(ma.AriannaAlgorithm):
    """The positions at its scheduled times, downloaded."""

    def __init__(self, chains, dependencies=None, **extras):
        self.metropolis, self.rows = dependencies[0], []

    def make_step(self, simulation):
        self.rows.append(self.metropolis.engine.download_state(want_e=False)[0].copy())


def build(path, steps, scheduler, keep=False, ladder=True, max_outside=0.0, hist=True):
    if ladder:
        chains = ma.ParticleChains.ladder(L, BETAS, "double_well", init_uniform=(-1.5, 1.5))
    else:
        chains = ma.ParticleChains(R * L, 1.0, "double_well", init_uniform=(-1.5, 1.5))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.6], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=11)]
    if ladder:
        al.append(dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), n_rungs=R))
    if hist:
        al.append(dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), scheduler=scheduler, max_outside=max_outside, **BINS))
    if keep:
        al.append(dict(algorithm=KeepPositions, dependencies=(ma.Metropolis,), scheduler=scheduler))
    return ma.Simulation(chains, al, steps, path=str(path))


@pytest.mark.parametrize("ladder", [True, False])
def test_fused_and_stepwise_runs_hold_the_same_counts(gpu, tmp_path, ladder):
    sched = list(range(6, 61, 6))
    got = []
    for fuse in (True, False):
        sim = build(tmp_path / str(fuse), 60, sched, keep=not fuse, ladder=ladder)
        ma.run(sim, fuse=fuse)
        eh = sim.algorithms[-2 if not fuse else -1]
        got.append(eh.counts())
        assert eh.n_snapshots == len(sched)
    G = R if ladder else 1
    assert got[0].shape == (G, BINS["n_bins"] + 3) and np.array_equal(got[0], got[1])
    assert np.array_equal(got[0].sum(axis=1), np.full(G, len(sched) * R * L // G, dtype=np.uint64))
    want = sum(T.snapshot("double_well", x, BINS["lo"], BINS["hi"], BINS["n_bins"], G) for x in sim.algorithms[-1].rows)
    assert np.array_equal(got[1], want)
    # the curve between the rungs (single-histogram reweighting around the shared beta without a ladder)
    grid = np.linspace(BETAS[0], BETAS[-1], 9) if ladder else np.linspace(0.9, 1.1, 5)
    log_z, m1, m2, c = eh.reweight(grid)
    assert all(np.all(np.isfinite(v)) for v in (log_z, m1, m2, c)) and np.all(c > 0) and np.all(np.diff(m1) < 0)
    f = eh.free_energies()
    assert f.shape == (G,) and f[0] == 0.0
    if ladder:
        assert np.allclose(eh.reweight(eh.betas())[0], -f, rtol=0, atol=1e-9)      # log Z(beta_r) = -f_r on WHAM's normalisation
    energies, log_g = eh.density_of_states()
    assert energies.shape == log_g.shape == (BINS["n_bins"],)
    eh.restart()
    assert eh.n_snapshots == 0


@pytest.mark.parametrize("cut", [12, 28])
def test_a_checkpointed_and_resumed_run_ends_on_the_same_counts(gpu, tmp_path, cut):
    """(Even cuts, on a snapshot time and between two: the exchange steps fall on every second time step, so the resumed run's
    schedule continues the whole run's.)"""
    sched = list(range(6, 61, 6))
    whole = build(tmp_path / "w", 60, sched)
    ma.run(whole)
    first = build(tmp_path / "a", cut, [t for t in sched if t <= cut])
    ma.run(first)
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    second = build(tmp_path / "b", 60 - cut, [t - cut for t in sched if t > cut])
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = second.algorithms[-1], whole.algorithms[-1]
    assert a.n_snapshots == b.n_snapshots == len(sched) and np.array_equal(a.counts(), b.counts())
    assert np.array_equal(second.chains.x.view(np.uint64), whole.chains.x.view(np.uint64))


def test_a_checkpoint_without_histograms_loads_unchanged(gpu, tmp_path):
    """The section's reader is conditional on its field: a run without an EnergyHistogram writes none, and a run with one resumes
    from such a checkpoint with an empty accumulator."""
    plain = build(tmp_path / "p", 10, [10], hist=False)
    ma.run(plain)
    fn = ma.checkpoint(plain.algorithms[0], str(tmp_path / "ck"))
    assert not [k for k in np.load(fn).files if k.startswith("ehist")]
    second = build(tmp_path / "s", 6, [6])
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    assert second.algorithms[-1].n_snapshots == 1


def test_annealing_keeps_a_histogram_per_temperature(gpu, tmp_path):
    """PopulationAnnealing(energy_histogram=...) at M = 3075 (a prefix tile and a ragged rest): every stored row is the twin's
    histogram of the state in front of that annealing step -- downloaded by an algorithm listed in front of the annealing --, the last
    one of the state at finalise, and reweight is finite along the schedule."""
    betas = [0.5, 0.75, 1.1, 1.6, 2.3]
    hist = dict(lo=0.0, hi=64.0, n_bins=128)
    chains = ma.ParticleChains.uniform(3075, betas[0], potential="double_well")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.6], 1.0),)
    sched = ma.build_schedule(8, 0, 2)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=13),
          dict(algorithm=KeepPositions, dependencies=(ma.Metropolis,), scheduler=sched),
          dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=sched, betas=betas[1:], energy_histogram=hist)]
    sim = ma.Simulation(chains, al, 8, path=str(tmp_path))
    ma.run(sim)
    kept, pa = sim.algorithms[1], sim.algorithms[2]
    b, counts = pa.histograms()
    assert np.array_equal(b, betas) and counts.shape == (5, 131)
    assert np.array_equal(counts.sum(axis=1), np.full(5, 3075, dtype=np.uint64))
    assert len(kept.rows) == 4
    for i, x in enumerate(kept.rows):
        assert np.array_equal(counts[i], T.snapshot("double_well", x, 0.0, 64.0, 128)[0]), i
    x_end = sim.algorithms[0].engine.download_state(want_e=False)[0]
    assert np.array_equal(counts[4], T.snapshot("double_well", x_end, 0.0, 64.0, 128)[0])
    log_z, m1, m2, c = pa.reweight(np.linspace(betas[0], betas[-1], 11))
    assert all(np.all(np.isfinite(v)) for v in (log_z, m1, m2, c)) and np.all(np.diff(m1) < 0)
    assert pa.reweight(np.array(betas[:1]))[0][0] == pytest.approx(0.0, abs=1e-9)      # log Z is 0 at the first temperature


def test_free_energies_and_heat_capacity_against_their_large_sample_limit(gpu):
    """The one statistical test (tests/ehist_stat.py holds the setup): double well, R = 6, beta_r = 0.5 * 1.5^r, 16 handles that are each
    a shard of 256 ladders of one ensemble; a burn-in, then 300 rounds of [2 sweeps; exchange; snapshot].  The 16 shard histograms are
    independent blocks; counts add, so the leave-one-out totals of a delete-one jackknife are exact.  theta = f_r - f_0 (r = 1 .. 5)
    and C at four beta between the rungs; theta_truth = the same wham / reweight applied to the exact bin probabilities by quadrature
    -- the estimator's own large-sample limit, so the binning bias cancels.  |theta - theta_truth| <= 5 se, the project's 5 sigma.
    max_outside = 0 holds for the truth alone (tests/test_reweighting_host.py checks the tail on the CPU), so no count may lie outside."""
    from montecarlo_amd import reweighting as rw
    M = S.LADDERS * S.R
    engines = []
    for s in range(S.SHARDS):
        eng = gpu.HipEngine(n_chains=M, chain_offset=s * M, n_chains_global=S.SHARDS * M, potential="double_well", beta=1.0, sigma=[0.6],
                            weight=[1.0], seed=41)
        eng.init_uniform(-1.5, 1.5)
        eng.upload_state(eng.download_state(want_e=False)[0], np.tile(S.BETAS, S.LADDERS))
        eng.set_ladder(S.R)
        engines.append(eng)
    for eng in engines:                                     # (everything is queued: the handles run side by side)
        eng.sweep_exchange(S.BURN_ROUNDS, S.SWEEPS)
        for _ in range(S.ROUNDS):
            eng.sweep_exchange(1, S.SWEEPS)
            eng.energy_histogram_accumulate(S.LO, S.HI, S.N_BINS)
    shards = []
    for eng in engines:
        counts, n_snap, _ = eng.energy_histogram_fetch()
        assert n_snap == S.ROUNDS and np.array_equal(counts.sum(axis=1), np.full(S.R, S.ROUNDS * S.LADDERS, dtype=np.uint64))
        assert not counts[:, S.N_BINS:].any()               # max_outside = 0: nothing below lo, at or above hi, NaN
        shards.append(counts[:, :S.N_BINS].astype(np.int64))
        eng.close()
    energies = rw.bin_centres(S.LO, S.HI, S.N_BINS)
    theta_of = lambda c: S.theta(c, rw.wham, rw.reweight, energies)
    total = np.sum(shards, axis=0)
    theta = theta_of(total)
    loo = np.array([theta_of(total - h) for h in shards])
    n = len(shards)
    se = np.sqrt((n - 1) / n * np.sum((loo - loo.mean(axis=0)) ** 2, axis=0))
    truth = theta_of(S.bin_probabilities())
    z = (theta - truth) / se
    names = [f"f_{r} - f_0" for r in range(1, S.R)] + [f"C({b:.4f})" for b in S.TARGET_BETAS]
    for name, t, tr, e, zz in zip(names, theta, truth, se, z):
        print(f"{name:12s} theta {t:.6f} truth {tr:.6f} se {e:.2e} z {zz:+.2f}")
    assert np.all(se > 0) and np.all(np.abs(z) <= 5.0), dict(zip(names, z))
