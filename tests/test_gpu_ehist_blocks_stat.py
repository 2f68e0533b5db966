"""The error bar of the reweighted curve end to end, and a checkpointed run with blocks.

Statistical: ehist_stat's double well (R = 6, beta_r = 0.5 * 1.5^r, 1600 bins on [0, 80)) on ONE handle of 2048 ladders in B = 32
blocks of chunk 8: 200 burn-in rounds, then 100 rounds of [2 sweeps; exchange; snapshot].  For the nine quantities of ehist_stat.theta
-- f_r - f_0, r = 1 .. 5, and C at four beta between the rungs -- |theta(counts) - theta(exact bin probabilities)| <= 5 se with the
se of jackknife_counts over the 32 blocks: the exact side goes through the same binned estimator, so the binning bias cancels, and
with 31 degrees of freedom a correct error bar misses 5 se with a probability of about 2e-5 per estimate.  se > 0 everywhere, and the
device's (theta, se) are those of the twin's block counts (tests/ehist_blocks_twin.py on the energies downloaded behind every
snapshot), bit for bit.  The test prints every pull.

The seed was checked on the CPU before it was committed: this configuration through the engine double of the host tests
(exchange_twin.TwinEngine, the oracle's sweeps and exchange steps) and ehist_blocks_twin gives the figures the device gives; its pulls
(theta - truth) / se are -2.17, -2.25, -2.23, -2.19, -2.16 for f_1 .. f_5 (one correlated quantity: they share the rungs below them)
and -1.39, -1.85, -1.72, -1.51 for C, so the worst is 2.25: the reference alone stays inside 3."""
import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd import reweighting as rw
from montecarlo_amd.jackknife import jackknife_counts

import ehist_blocks_twin as KB
import ehist_stat as S

pytestmark = pytest.mark.gpu
LADDERS, B, CHUNK, BURN_ROUNDS, ROUNDS = 2048, 32, 8, 200, 100


def theta_and_se(blocks):
    energies = rw.bin_centres(S.LO, S.HI, S.N_BINS)
    full = {}

    def wham(*args):                                        # the total comes first: the replicates start from its solution
        out = rw.wham(*args, f0=full.get("f"))
        full.setdefault("f", out[1])
        return out

    def fn(counts):
        return S.theta(counts[:, :S.N_BINS], wham, rw.reweight, energies)

    return jackknife_counts(blocks, fn)


def test_the_curve_lies_within_five_standard_errors_and_the_device_matches_the_twin(gpu):
    M = LADDERS * S.R
    eng = gpu.HipEngine(n_chains=M, potential="double_well", beta=1.0, sigma=[0.6], weight=[1.0], seed=41)
    eng.init_uniform(-1.5, 1.5)
    eng.upload_state(eng.download_state(want_e=False)[0], np.tile(S.BETAS, LADDERS))
    eng.set_ladder(S.R)
    eng.sweep_exchange(BURN_ROUNDS, S.SWEEPS)
    eng.set_blocks(B, CHUNK)
    twin = np.zeros((B, S.R, S.N_BINS + 3), dtype=np.uint64)
    for _ in range(ROUNDS):
        eng.sweep_exchange(1, S.SWEEPS)
        eng.energy_histogram_accumulate_blocks(S.LO, S.HI, S.N_BINS)
        twin += KB.histogram(eng.download_state()[1], S.LO, S.HI, S.N_BINS, S.R, B, CHUNK)
    got, n_snap, _ = eng.energy_histogram_fetch_blocks()
    eng.close()
    assert n_snap == ROUNDS and np.array_equal(got, twin)
    assert not got[:, :, S.N_BINS:].any()                   # max_outside = 0: nothing below lo, at or above hi, NaN
    theta, se = theta_and_se(got)
    theta_t, se_t = theta_and_se(twin)
    assert np.array_equal(theta, theta_t) and np.array_equal(se, se_t)
    energies = rw.bin_centres(S.LO, S.HI, S.N_BINS)
    truth = S.theta(S.bin_probabilities(), rw.wham, rw.reweight, energies)
    z = (theta - truth) / se
    names = [f"f_{r} - f_0" for r in range(1, S.R)] + [f"C({b:.4f})" for b in S.TARGET_BETAS]
    for name, t, tr, e, zz in zip(names, theta, truth, se, z):
        print(f"{name:12s} theta {t:.6f} truth {tr:.6f} se {e:.2e} z {zz:+.2f}")
    assert np.all(se > 0) and np.all(np.abs(z) <= 5.0), dict(zip(names, z))


# ---- a checkpointed run -------------------------------------------------------------------------------------------------------------------
R, L = 4, 131
BETAS = 0.5 * 1.5 ** np.arange(R)
BINS = dict(lo=0.0, hi=40.0, n_bins=160)


def build(path, steps, scheduler, blocks=4):
    chains = ma.ParticleChains.ladder(L, BETAS, "double_well", init_uniform=(-1.5, 1.5))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.6], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=11),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), n_rungs=R),
          dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), scheduler=scheduler, blocks=blocks,
               block_chunk=5 if blocks else None, **BINS)]
    return ma.Simulation(chains, al, steps, path=str(path))


def test_a_checkpointed_and_resumed_run_ends_on_the_same_block_counts(gpu, tmp_path):
    sched = list(range(6, 31, 6))
    whole = build(tmp_path / "w", 36, sched + [36])
    ma.run(whole)
    first = build(tmp_path / "a", 30, sched)
    ma.run(first)
    fn = ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    assert np.array_equal(np.load(fn)["ehist_blocks"], [4, 5]) and np.load(fn)["ehist_block_counts"].shape == (4, R, 163)
    second = build(tmp_path / "b", 6, [6])                 # one more snapshot
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = second.algorithms[-1], whole.algorithms[-1]
    assert a.n_snapshots == b.n_snapshots == 6
    assert np.array_equal(a.counts_blocks(), b.counts_blocks()) and np.array_equal(a.counts(), b.counts())
    assert np.array_equal(a.counts_blocks().sum(axis=0, dtype=np.uint64), a.counts())
    # the curve with its error bar, and the refusals of the Python surface
    grid = np.linspace(BETAS[0], BETAS[-1], 5)
    values = b.reweight(grid)
    pairs = b.reweight(grid, error=True)
    assert all(np.array_equal(p[0], v) and p[1].shape == v.shape and np.all(p[1][1:] > 0) for p, v in zip(pairs, values))
    f, f_se = b.free_energies(error=True)
    assert np.array_equal(f, b.free_energies()) and f_se[0] == 0.0 and np.all(f_se[1:] > 0)
    energies, (log_g, log_g_se) = b.density_of_states(error=True)
    assert np.array_equal(log_g, b.density_of_states()[1]) and log_g_se.shape == log_g.shape
    assert np.all(np.isnan(log_g_se[~np.isfinite(log_g)]))
    assert ma.callback_reweight_error(whole).shape == (4, R)
    other = build(tmp_path / "c", 6, [6], blocks=2)
    with pytest.raises(ValueError, match="under the partition"):
        ma.restore(other.algorithms[0], str(tmp_path / "ck"))
    plain = build(tmp_path / "d", 6, [6], blocks=None)
    with pytest.raises(ValueError, match="needs blocks"):
        plain.algorithms[-1].reweight(grid, error=True)
