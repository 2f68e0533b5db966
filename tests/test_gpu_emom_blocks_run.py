"""``run(...)`` with an ``EnergyHistogram(moments=..., blocks=B)`` on the device, end to end: fused and stepwise runs and a
checkpointed, resumed run hold the same per-block integers -- counts and sums per bin --, they equal the host twin
(tests/emom_blocks_twin.py) applied to the positions the same run downloaded, a run with and without ``blocks`` gives bit-equal
results, and the one statistical test of the error bar.

Statistical: the configuration of tests/test_gpu_ehist_blocks_stat.py -- ehist_stat's double well (R = 6, beta_r = 0.5 * 1.5^r, 1600
bins on [0, 80)) on ONE handle of 2048 ladders in B = 32 blocks of chunk 8, seed 41: 200 burn-in rounds, then 100 rounds of [2 sweeps;
exchange; snapshot]; the trajectory is that test's own, since the pass only observes.  Columns XX | POS, x_bound = 4 (an in-range
energy has |x| <= sqrt(1 + sqrt(80)) < 3.2, so the fourth cell is empty by construction).  theta = <x^2> and P(x > 0) reweighted to
ehist_stat.TARGET_BETAS; the truth is the estimator's own large-sample limit, the same wham / reweight_observable applied to the exact
bin probabilities and the exact per-bin integrals, as in tests/test_gpu_emom_run.py.  |theta - truth| <= 5 se with the se of the
delete-one-block jackknife over the 32 blocks, se > 0 everywhere, and the device's (theta, se) are those of the twin's cells, bit for
bit.  The test prints every pull.

The seed was checked on the CPU before it was committed: this configuration through the engine double of the host tests
(exchange_twin.TwinEngine, the oracle's sweeps and exchange steps) and emom_blocks_twin gives pulls (theta - truth) / se of -0.26,
+0.48, +0.95, +1.15 for <x^2> and -0.83, -0.71, -0.64, -0.64 for P(x > 0) at the four target beta (the occupancies are one
correlated quantity: the same ladders cross the barrier at every beta), so the worst is 1.15: the
reference alone stays inside 3."""
import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd import reweighting as rw
from montecarlo_amd.jackknife import jackknife_integers

import ehist_stat as S
import emom_blocks_twin as EB
import emom_twin as E

pytestmark = pytest.mark.gpu
R, L = 4, 131
BETAS = 0.5 * 1.5 ** np.arange(R)
BINS = dict(lo=0.0, hi=40.0, n_bins=160)
MOMENTS, X_BOUND = ("x", "x2", "pos"), 3.0            # an in-range energy has |x| <= sqrt(1 + sqrt(40)) < 2.71
MASK = E.X | E.XX | E.POS
PART = (4, 5)


class KeepPositions(ma.AriannaAlgorithm):
    """The positions at its scheduled times, downloaded."""

    def __init__(self, chains, dependencies=None, **extras):
        self.metropolis, self.rows = dependencies[0], []

    def make_step(self, simulation):
        self.rows.append(self.metropolis.engine.download_state(want_e=False)[0].copy())


def build(path, steps, scheduler, keep=False, blocks=PART[0]):
    chains = ma.ParticleChains.ladder(L, BETAS, "double_well", init_uniform=(-1.5, 1.5))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.6], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=11),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), n_rungs=R),
          dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), scheduler=scheduler, moments=MOMENTS, x_bound=X_BOUND, blocks=blocks,
               block_chunk=PART[1] if blocks else None, **BINS)]
    if keep:
        al.append(dict(algorithm=KeepPositions, dependencies=(ma.Metropolis,), scheduler=scheduler))
    return ma.Simulation(chains, al, steps, path=str(path))


def integers(eh):
    """(counts[B, G, n_bins + 4], sums[B, G, C, n_bins], n_snapshots) as the engine holds them."""
    return eh.metropolis.engine.energy_moments_fetch_blocks()[:3]


def test_fused_and_stepwise_runs_hold_the_same_integers_per_block(gpu, tmp_path):
    sched = list(range(6, 61, 6))
    got = []
    for fuse in (True, False):
        sim = build(tmp_path / str(fuse), 60, sched, keep=not fuse)
        ma.run(sim, fuse=fuse)
        eh = sim.algorithms[-2 if not fuse else -1]
        got.append(integers(eh))
        assert eh.n_snapshots == len(sched)
    n = BINS["n_bins"]
    assert got[0][0].shape == (PART[0], R, n + 4) and got[0][1].shape == (PART[0], R, 3, n)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    want_c, want_s = np.zeros((PART[0], R, n + 4), dtype=np.uint64), np.zeros((PART[0], R, 3, n), dtype=np.int64)
    for x in sim.algorithms[-1].rows:
        c, s = EB.snapshot("double_well", x, BINS["lo"], BINS["hi"], n, MASK, X_BOUND, R, *PART)
        want_c += c
        want_s += s
    assert np.array_equal(got[1][0], want_c) and np.array_equal(got[1][1], want_s)
    # the results of the Python layer from those integers
    assert np.array_equal(eh.counts_blocks(), want_c[:, :, :n + 3]) and np.array_equal(eh.counts(), want_c.sum(axis=0, dtype=np.uint64)[:, :n + 3])
    quanta = np.array([2.0 ** (2 - 32), 2.0 ** (4 - 32), 1.0])                 # x_bound = 3: eb = 2
    assert np.array_equal(eh.moment_sums_blocks(), want_s.astype(np.float64) * quanta[None, None, :, None])
    assert np.array_equal(eh.moment_sums(), want_s.sum(axis=0).astype(np.float64) * quanta[None, :, None])
    grid = np.linspace(BETAS[0], BETAS[-1], 9)
    plain, pairs = eh.reweight_moments(grid), eh.reweight_moments(grid, error=True)
    for name in MOMENTS:
        assert np.array_equal(pairs[name][0], plain[name]) and pairs[name][1].shape == grid.shape and np.all(pairs[name][1] > 0), name
    out = ma.callback_reweight_moments_error(sim)
    assert out.shape == (3, R) and np.all(np.isfinite(out))
    assert ma.callback_reweight_error(sim).shape == (4, R)          # the counts' curve takes its error bar from the same counts
    eh.restart()
    assert eh.n_snapshots == 0


@pytest.mark.parametrize("cut", [12, 28])
def test_a_checkpointed_and_resumed_run_ends_on_the_same_integers_per_block(gpu, tmp_path, cut):
    sched = list(range(6, 61, 6))
    whole = build(tmp_path / "w", 60, sched)
    ma.run(whole)
    first = build(tmp_path / "a", cut, [t for t in sched if t <= cut])
    ma.run(first)
    fn = ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    files = np.load(fn).files
    assert {"emom_blocks", "emom_block_counts", "emom_block_sums", "emom_block_snapshots", "emom_counts", "emom_sums"} <= set(files)
    assert "ehist_counts" not in files and "ehist_block_counts" not in files
    second = build(tmp_path / "b", 60 - cut, [t - cut for t in sched if t > cut])
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = integers(second.algorithms[-1]), integers(whole.algorithms[-1])
    assert a[2] == b[2] == len(sched) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(second.chains.x.view(np.uint64), whole.chains.x.view(np.uint64))
    if cut == 12:
        other = build(tmp_path / "c", 6, [6], blocks=2)
        with pytest.raises(ValueError, match="under the partition"):
            ma.restore(other.algorithms[0], str(tmp_path / "ck"))
        plain = build(tmp_path / "d", 60 - cut, [t - cut for t in sched if t > cut], blocks=None)      # goes on with the merged plain accumulator
        ma.restore(plain.algorithms[0], str(tmp_path / "ck"))
        ma.run(plain)
        merged = plain.algorithms[-1].metropolis.engine.energy_moments_fetch()
        assert merged[2] == len(sched) and np.array_equal(merged[0], b[0].sum(axis=0, dtype=np.uint64)) and np.array_equal(merged[1], b[1].sum(axis=0))


def test_a_run_with_and_without_blocks_gives_bit_equal_results(gpu, tmp_path):
    sched = list(range(6, 61, 6))
    grid = np.linspace(BETAS[0], BETAS[-1], 9)
    out = []
    for blocks in (PART[0], None):
        sim = build(tmp_path / str(blocks), 60, sched, blocks=blocks)
        ma.run(sim)
        eh = sim.algorithms[-1]
        out.append((eh.counts(), eh.moment_sums(), eh.reweight_moments(grid), sim.chains.x.copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1].view(np.uint64), out[1][1].view(np.uint64))
    assert all(np.array_equal(out[0][2][m].view(np.uint64), out[1][2][m].view(np.uint64)) for m in MOMENTS)
    assert np.array_equal(out[0][3].view(np.uint64), out[1][3].view(np.uint64))


# ---- the statistical test -----------------------------------------------------------------------------------------------------------------
LADDERS, B, CHUNK, BURN_ROUNDS, ROUNDS = 2048, 32, 8, 200, 100
STAT_MASK, STAT_BOUND = E.XX | E.POS, 4.0
Q = np.array([2.0 ** (2 * 3 - 32), 1.0])                   # x_bound = 4: eb = 3; the quanta of XX and POS


def theta_of(log_g, counts, sums, energies):
    """<x^2> and P(x > 0) at the target beta from a density of states, counts[R, N_BINS] and sums[R, 2, N_BINS] (Float64)."""
    return np.concatenate([rw.reweight_observable(log_g, energies, S.TARGET_BETAS, sums[:, c], counts) for c in range(2)])


def theta_and_se(counts_blocks, sums_blocks):
    """(theta, se) from the cells per block: every replicate is the whole of WHAM on its leave-one-out counts, started from the full
    solution, followed by reweight_observable with its leave-one-out sums and counts."""
    energies = rw.bin_centres(S.LO, S.HI, S.N_BINS)
    full = {}

    def fn(counts, sums):
        out = rw.wham(counts[:, :S.N_BINS], S.BETAS, energies, f0=full.get("f"))
        full.setdefault("f", out[1])                        # the total comes first
        return theta_of(out[0], counts[:, :S.N_BINS], sums.astype(np.float64) * Q[None, :, None], energies)

    return jackknife_integers([counts_blocks, sums_blocks], fn)


def _bin_integrals(beta, f):
    """The integral of f(x) exp(-beta U) over {x : U(x) in bin b}, b < N_BINS, by ehist_stat's quadrature: the outer and the inner
    interval of x >= 0 and their mirror images (f is applied to x and to -x)."""
    edges = S.LO + (S.HI - S.LO) / S.N_BINS * np.arange(S.N_BINS + 1)
    ra, rb = np.sqrt(edges[:-1]), np.sqrt(edges[1:])
    g = lambda x: (f(x) + f(-x)) * np.exp(-beta * S.potential(x))
    outer = S._integrate(g, np.sqrt(1.0 + ra), np.sqrt(1.0 + rb))
    inner = S._integrate(g, np.sqrt(np.maximum(1.0 - rb, 0.0)), np.sqrt(np.maximum(1.0 - ra, 0.0)))
    return outer + inner


def truth():
    """The large-sample limit: expected counts p_kb and expected sums per sample, the integral over the bin of o exp(-beta_k U) / Z_k."""
    energies = rw.bin_centres(S.LO, S.HI, S.N_BINS)
    p = S.bin_probabilities()
    z = np.array([S.bin_weights(b).sum() + S.tail_weight(b) for b in S.BETAS])
    s_xx = np.stack([_bin_integrals(b, lambda x: x * x) for b in S.BETAS]) / z[:, None]
    s_pos = np.stack([_bin_integrals(b, lambda x: (x > 0).astype(np.float64)) for b in S.BETAS]) / z[:, None]
    assert np.allclose(np.stack([_bin_integrals(b, lambda x: np.ones_like(x)) for b in S.BETAS]) / z[:, None], p, rtol=1e-12, atol=0)
    return theta_of(rw.wham(p, S.BETAS, energies)[0], p, np.stack([s_xx, s_pos], axis=1), energies)


NAMES = [f"<x^2>({b:.4f})" for b in S.TARGET_BETAS] + [f"P(x>0)({b:.4f})" for b in S.TARGET_BETAS]


def test_the_moments_lie_within_five_standard_errors_and_the_device_matches_the_twin(gpu):
    M = LADDERS * S.R
    eng = gpu.HipEngine(n_chains=M, potential="double_well", beta=1.0, sigma=[0.6], weight=[1.0], seed=41)
    eng.init_uniform(-1.5, 1.5)
    eng.upload_state(eng.download_state(want_e=False)[0], np.tile(S.BETAS, LADDERS))
    eng.set_ladder(S.R)
    eng.sweep_exchange(BURN_ROUNDS, S.SWEEPS)
    eng.set_blocks(B, CHUNK)
    twin = [np.zeros((B, S.R, S.N_BINS + 4), dtype=np.uint64), np.zeros((B, S.R, 2, S.N_BINS), dtype=np.int64)]
    for _ in range(ROUNDS):
        eng.sweep_exchange(1, S.SWEEPS)
        eng.energy_moments_accumulate_blocks(S.LO, S.HI, S.N_BINS, STAT_MASK, STAT_BOUND)
        x, e = eng.download_state()
        c, s = EB.moments(e, x, S.LO, S.HI, S.N_BINS, STAT_MASK, STAT_BOUND, S.R, B, CHUNK)
        twin[0] += c
        twin[1] += s
    counts, sums, n_snap, _ = eng.energy_moments_fetch_blocks()
    eng.close()
    assert n_snap == ROUNDS and np.array_equal(counts, twin[0]) and np.array_equal(sums, twin[1])
    assert not counts[:, :, S.N_BINS:].any()                # nothing below lo, at or above hi, NaN -- and nothing beyond x_bound
    theta, se = theta_and_se(counts, sums)
    theta_t, se_t = theta_and_se(*twin)
    assert np.array_equal(theta, theta_t) and np.array_equal(se, se_t)
    want = truth()
    z = (theta - want) / se
    for name, t, tr, err, zz in zip(NAMES, theta, want, se, z):
        print(f"{name:16s} theta {t:.6f} truth {tr:.6f} se {err:.2e} z {zz:+.2f}")
    assert np.all(se > 0) and np.all(np.abs(z) <= 5.0), dict(zip(NAMES, z))
