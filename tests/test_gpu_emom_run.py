"""``run(...)`` with an ``EnergyHistogram(moments=...)`` on the device, end to end: fused and stepwise runs and a checkpointed, resumed
run hold the same integers -- counts and sums per bin --, they equal the host twin applied to the positions the same run downloaded,
and the one statistical test of the moments: <x^2> and P(x > 0) reweighted between the rungs against the estimator's own
large-sample limit."""
import numpy as np
import pytest

import montecarlo_amd as ma

import ehist_stat as S
import emom_twin as E

pytestmark = pytest.mark.gpu
R, L = 4, 131
BETAS = 0.5 * 1.5 ** np.arange(R)
BINS = dict(lo=0.0, hi=40.0, n_bins=160)
MOMENTS, X_BOUND = ("x", "x2", "pos"), 3.0            # an in-range energy has |x| <= sqrt(1 + sqrt(40)) < 2.71
MASK = E.X | E.XX | E.POS


class KeepPositions(ma.AriannaAlgorithm):
    """The positions at its scheduled times, downloaded."""

    def __init__(self, chains, dependencies=None, **extras):
        self.metropolis, self.rows = dependencies[0], []

    def make_step(self, simulation):
        self.rows.append(self.metropolis.engine.download_state(want_e=False)[0].copy())


def build(path, steps, scheduler, keep=False, ladder=True, hist=True, moments=MOMENTS):
    if ladder:
        chains = ma.ParticleChains.ladder(L, BETAS, "double_well", init_uniform=(-1.5, 1.5))
    else:
        chains = ma.ParticleChains(R * L, 1.0, "double_well", init_uniform=(-1.5, 1.5))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.6], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=11)]
    if ladder:
        al.append(dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), n_rungs=R))
    if hist:
        extra = dict(moments=moments, x_bound=X_BOUND) if moments else {}
        al.append(dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), scheduler=scheduler, **BINS, **extra))
    if keep:
        al.append(dict(algorithm=KeepPositions, dependencies=(ma.Metropolis,), scheduler=scheduler))
    return ma.Simulation(chains, al, steps, path=str(path))


def integers(eh):
    """(counts[G, n_bins + 4], sums[G, C, n_bins], n_snapshots) as the engine holds them."""
    return eh.metropolis.engine.energy_moments_fetch()[:3]


@pytest.mark.parametrize("ladder", [True, False])
def test_fused_and_stepwise_runs_hold_the_same_integers(gpu, tmp_path, ladder):
    sched = list(range(6, 61, 6))
    got = []
    for fuse in (True, False):
        sim = build(tmp_path / str(fuse), 60, sched, keep=not fuse, ladder=ladder)
        ma.run(sim, fuse=fuse)
        eh = sim.algorithms[-2 if not fuse else -1]
        got.append(integers(eh))
        assert eh.n_snapshots == len(sched)
    G, n = (R if ladder else 1), BINS["n_bins"]
    assert got[0][0].shape == (G, n + 4) and got[0][1].shape == (G, 3, n)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    want_c, want_s = np.zeros((G, n + 4), dtype=np.uint64), np.zeros((G, 3, n), dtype=np.int64)
    for x in sim.algorithms[-1].rows:
        c, s = E.snapshot("double_well", x, BINS["lo"], BINS["hi"], n, MASK, X_BOUND, G)
        want_c += c
        want_s += s
    assert np.array_equal(got[1][0], want_c) and np.array_equal(got[1][1], want_s)
    # the results of the Python layer from those integers
    assert np.array_equal(eh.counts(), want_c[:, :n + 3]) and not eh.beyond_bound().any()
    quanta = np.array([2.0 ** (2 - 32), 2.0 ** (4 - 32), 1.0])                 # x_bound = 3: eb = 2
    assert np.array_equal(eh.moment_sums(), want_s.astype(np.float64) * quanta[None, :, None])
    energies, micro = eh.microcanonical()
    live = want_c[:, :n].sum(axis=0) > 0
    assert micro.shape == (3, n) and np.all(np.isnan(micro[:, ~live])) and np.all(np.isfinite(micro[:, live]))
    assert np.all(micro[1, live] >= 0) and np.all((micro[2, live] >= 0) & (micro[2, live] <= 1))
    grid = np.linspace(BETAS[0], BETAS[-1], 9) if ladder else np.linspace(0.9, 1.1, 5)
    out = eh.reweight_moments(grid)
    assert tuple(out) == MOMENTS and all(v.shape == grid.shape and np.all(np.isfinite(v)) for v in out.values())
    assert np.all(out["x2"] > 0) and np.all((out["pos"] >= 0) & (out["pos"] <= 1)) and np.all(np.abs(out["x"]) <= X_BOUND)
    at_rungs = ma.callback_reweight_moments(sim)
    assert at_rungs.shape == (3, G)
    eh.restart()
    assert eh.n_snapshots == 0


@pytest.mark.parametrize("cut", [12, 28])
def test_a_checkpointed_and_resumed_run_ends_on_the_same_integers(gpu, tmp_path, cut):
    sched = list(range(6, 61, 6))
    whole = build(tmp_path / "w", 60, sched)
    ma.run(whole)
    first = build(tmp_path / "a", cut, [t for t in sched if t <= cut])
    ma.run(first)
    fn = ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    files = np.load(fn).files
    assert {"emom_form", "emom_counts", "emom_sums", "emom_snapshots"} <= set(files) and "ehist_counts" not in files
    second = build(tmp_path / "b", 60 - cut, [t - cut for t in sched if t > cut])
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = integers(second.algorithms[-1]), integers(whole.algorithms[-1])
    assert a[2] == b[2] == len(sched) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(second.chains.x.view(np.uint64), whole.chains.x.view(np.uint64))


def test_checkpoints_without_moments_load_unchanged(gpu, tmp_path):
    """The section's reader is conditional on its fields: a run without an EnergyHistogram, and one with a plain EnergyHistogram, write
    no moments; a run with moments resumes from either with an empty accumulator, and a plain one resumes from a checkpoint that
    holds moments with its own counts empty."""
    for i, kw in enumerate((dict(hist=False), dict(moments=None))):
        plain = build(tmp_path / f"p{i}", 10, [10], **kw)
        ma.run(plain)
        fn = ma.checkpoint(plain.algorithms[0], str(tmp_path / f"ck{i}"))
        assert not [k for k in np.load(fn).files if k.startswith("emom")]
        second = build(tmp_path / f"s{i}", 6, [6])
        ma.restore(second.algorithms[0], str(tmp_path / f"ck{i}"))
        ma.run(second)
        assert second.algorithms[-1].n_snapshots == 1 and integers(second.algorithms[-1])[2] == 1
    with_moments = build(tmp_path / "m", 10, [10])
    ma.run(with_moments)
    ma.checkpoint(with_moments.algorithms[0], str(tmp_path / "ckm"))
    third = build(tmp_path / "t", 6, [6], moments=None)
    ma.restore(third.algorithms[0], str(tmp_path / "ckm"))
    ma.run(third)
    assert third.algorithms[-1].n_snapshots == 1


def test_moments_refuse_what_they_cannot_do(gpu, tmp_path):
    for extra, msg in ((dict(moments=("x",), x_bound=2.0, blocks=4), "jackknife block"), (dict(moments=("x",)), "x_bound"),
                       (dict(moments=("y",), x_bound=2.0), "moments"), (dict(moments=(), x_bound=2.0), "moments"),
                       (dict(x_bound=2.0), "without moments"), (dict(moments=("x",), x_bound=float("inf")), "x_bound")):
        chains = ma.ParticleChains.ladder(L, BETAS, "double_well", init_uniform=(-1.5, 1.5))
        pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.6], 1.0),)
        al = [dict(algorithm=ma.Metropolis, pool=pool, seed=11),
              dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), scheduler=[2], **BINS, **extra)]
        with pytest.raises(ValueError, match=msg):
            ma.Simulation(chains, al, 2, path=str(tmp_path))
    # max_outside covers the fourth cell and names it: a bound inside the wells puts most binned chains beyond it
    chains = ma.ParticleChains.ladder(L, BETAS, "double_well", init_uniform=(-1.5, 1.5))
    al = [dict(algorithm=ma.Metropolis, pool=(ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.6], 1.0),), seed=11),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=[2], n_rungs=R),
          dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), scheduler=[2], moments=("x2",), x_bound=0.5, **BINS)]
    sim = ma.Simulation(chains, al, 2, path=str(tmp_path / "o"))
    ma.run(sim)
    eh = sim.algorithms[-1]
    assert eh.beyond_bound().sum() > 0 and eh.moment_sums().shape == (R, 1, BINS["n_bins"])
    with pytest.raises(ValueError, match="x beyond x_bound"):
        eh.reweight_moments(BETAS)


# ---- the statistical test -----------------------------------------------------------------------------------------------------------------
def _bin_integrals(beta, f):
    """The integral of f(x) exp(-beta U) over {x : U(x) in bin b}, b < N_BINS, by ehist_stat's quadrature: the outer and the inner
    interval of x >= 0 and their mirror images (f is applied to x and to -x)."""
    edges = S.LO + (S.HI - S.LO) / S.N_BINS * np.arange(S.N_BINS + 1)
    ra, rb = np.sqrt(edges[:-1]), np.sqrt(edges[1:])
    g = lambda x: (f(x) + f(-x)) * np.exp(-beta * S.potential(x))
    outer = S._integrate(g, np.sqrt(1.0 + ra), np.sqrt(1.0 + rb))
    inner = S._integrate(g, np.sqrt(np.maximum(1.0 - rb, 0.0)), np.sqrt(np.maximum(1.0 - ra, 0.0)))
    return outer + inner


def test_reweighted_moments_against_their_large_sample_limit(gpu):
    """The setup of the energy histograms' statistical test (tests/ehist_stat.py): double well, R = 6, beta_r = 0.5 * 1.5^r, [0, 80) in
    1600 bins, 16 handles that are each a shard of 256 ladders of one ensemble; a burn-in, then 300 rounds of [2 sweeps; exchange;
    snapshot with the sums of x^2 and [x > 0]].  x_bound = 4: an in-range energy has |x| <= sqrt(1 + sqrt(80)) < 3.2, so the fourth
    cell is empty by construction.  theta = <x^2> and P(x > 0) reweighted to the four beta between the rungs; theta_truth = the same
    wham / reweight_observable applied to the exact bin probabilities and the exact per-bin integrals of x^2 exp(-beta U) and
    [x > 0] exp(-beta U), by the same Gauss-Legendre quadrature -- the estimator's own large-sample limit.  The 16 shards are
    independent blocks; counts and sums add, so the leave-one-out totals of a delete-one jackknife are exact.
    |theta - theta_truth| <= 5 se, the project's 5 sigma."""
    from montecarlo_amd import reweighting as rw
    M = S.LADDERS * S.R
    mask, x_bound = E.XX | E.POS, 4.0
    q_xx = 2.0 ** (2 * 3 - 32)                              # x_bound = 4: eb = 3
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
            eng.energy_moments_accumulate(S.LO, S.HI, S.N_BINS, mask, x_bound)
    shards = []
    for eng in engines:
        counts, sums, n_snap, _ = eng.energy_moments_fetch()
        assert n_snap == S.ROUNDS and np.array_equal(counts.sum(axis=1), np.full(S.R, S.ROUNDS * S.LADDERS, dtype=np.uint64))
        assert not counts[:, S.N_BINS:].any()               # nothing below lo, at or above hi, NaN -- and nothing beyond x_bound
        shards.append((counts[:, :S.N_BINS].astype(np.float64), sums[:, 0].astype(np.float64) * q_xx, sums[:, 1].astype(np.float64)))
        eng.close()
    energies = rw.bin_centres(S.LO, S.HI, S.N_BINS)

    def theta_of(counts, s_xx, s_pos):
        log_g = rw.wham(counts, S.BETAS, energies)[0]
        return np.concatenate([rw.reweight_observable(log_g, energies, S.TARGET_BETAS, s, counts) for s in (s_xx, s_pos)])

    total = [np.sum([sh[i] for sh in shards], axis=0) for i in range(3)]
    theta = theta_of(*total)
    loo = np.array([theta_of(*(t - h for t, h in zip(total, sh))) for sh in shards])
    n = len(shards)
    se = np.sqrt((n - 1) / n * np.sum((loo - loo.mean(axis=0)) ** 2, axis=0))
    # the large-sample limit: expected counts p_kb and expected sums per sample, integral over the bin of o exp(-beta_k U) / Z_k
    p = S.bin_probabilities()
    z = np.array([S.bin_weights(b).sum() + S.tail_weight(b) for b in S.BETAS])
    s_xx = np.stack([_bin_integrals(b, lambda x: x * x) for b in S.BETAS]) / z[:, None]
    s_pos = np.stack([_bin_integrals(b, lambda x: (x > 0).astype(np.float64)) for b in S.BETAS]) / z[:, None]
    assert np.allclose(np.stack([_bin_integrals(b, lambda x: np.ones_like(x)) for b in S.BETAS]) / z[:, None], p, rtol=1e-12, atol=0)
    truth = theta_of(p, s_xx, s_pos)
    zs = (theta - truth) / se
    names = [f"<x^2>({b:.4f})" for b in S.TARGET_BETAS] + [f"P(x>0)({b:.4f})" for b in S.TARGET_BETAS]
    for name, t, tr, e, zz in zip(names, theta, truth, se, zs):
        print(f"{name:16s} theta {t:.6f} truth {tr:.6f} se {e:.2e} z {zz:+.2f}")
    assert np.all(se > 0) and np.all(np.abs(zs) <= 5.0), dict(zip(names, zs))
