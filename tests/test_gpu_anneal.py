"""Population annealing on the device (include/amc.h amc_anneal .. amc_upload_families) against its host twin
(tests/anneal_twin.py), bit for bit: positions, energies, beta, the annealing step index, the records and the families -- and the Move
counters and the MH step, which annealing leaves alone -- over sequences that interleave sweeps and annealing steps.  Shapes are the
smallest at which the kernels take another path: one chain, wave (64) and block (256) boundaries, the tile of the prefix passes
(1024 chains) and several tiles, odd sizes, and one ensemble that walks a one-block-per-CU grid more than once."""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd.system import CustomPotential

import anneal_twin as A
import oracle_lib as O

pytestmark = pytest.mark.gpu
POOLS = {1: ([0.5], [1.0]), 2: ([0.5, 0.25], [0.625, 0.375])}
CUSTOM = "x*x*x*x - 2.0*x*x + 0.25*x"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def start_x(M):
    ids = np.arange(M)
    return 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)


def make_pair(gpu, M, *, x=None, beta=0.5, potential="harmonic", K=1, dtype="f64", families=False, seed=23, counters=True):
    """(HipEngine, AnnealTwin over the matching OracleSim), both holding the same start state at the same shared beta."""
    sigma, weight = POOLS[K]
    x = start_x(M) if x is None else np.asarray(x, dtype=np.float64)
    if dtype == "f32":
        x = x.astype(np.float32).astype(np.float64)
    eng = gpu.HipEngine(n_chains=M, potential=potential, beta=beta, sigma=sigma, weight=weight, seed=seed, dtype=dtype, per_chain_counters=counters)
    eng.upload_state(x)
    sim = O.OracleSim(M, potential=potential, beta=beta, sigma=sigma, weight=weight, seed=seed, dtype=dtype)
    sim.set_x(x)
    tw = A.AnnealTwin(sim, beta, seed=seed, potential=potential, f32=dtype == "f32", families=families)
    if families:
        eng.set_anneal_families(True)
    return eng, tw


def compare(eng, tw, counters=True):
    x, e = eng.download_state()
    xo, eo = tw.sim.state()
    assert np.array_equal(bits(x), bits(xo)), ("positions differ from the twin", np.flatnonzero(bits(x) != bits(xo))[:8])
    assert np.array_equal(bits(e), bits(eo)), "energies differ from the twin"
    assert eng.beta == tw.beta and eng.anneal_step == tw.t_a
    rec = eng.anneal_records()
    assert np.array_equal(rec, tw.records_array()), ("records differ from the twin", rec.tolist(), tw.records)
    if tw.fam is not None:
        assert np.array_equal(eng.download_families(), tw.fam), "families differ from the twin"
        assert eng.anneal_family_stats() == tw.family_stats()
    ao, to = tw.sim.counters()
    if counters:
        acc, tot = eng.download_counters()
        assert np.array_equal(acc, ao) and np.array_equal(tot, to), "Move counters differ from the twin"
    assert eng.step == tw.sim.step


def interleave(eng, tw, counters=True):
    """sweep(1), cool, sweep(2), cool, heat, the identity, sweep(1) on both; compared after the first step and at the end."""
    for o in (eng, tw):
        o.sweep(1); o.anneal(0.9)
    compare(eng, tw, counters)
    for o in (eng, tw):
        o.sweep(2); o.anneal(2.0); o.anneal(1.25); o.anneal(1.25); o.sweep(1)
    compare(eng, tw, counters)
    assert eng.estimator_step == 0


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3075])
def test_anneal_matches_the_twin(gpu, M, potential):
    eng, tw = make_pair(gpu, M, potential=potential, families=True)
    interleave(eng, tw)
    eng.close()


@pytest.mark.parametrize("K,counters", [(1, False), (2, True)])
def test_anneal_with_other_pools(gpu, K, counters):
    eng, tw = make_pair(gpu, 1025, potential="double_well", K=K, counters=counters)
    interleave(eng, tw, counters)
    eng.close()


@pytest.mark.parametrize("potential", ["harmonic", "double_well", CustomPotential(CUSTOM)])
def test_anneal_with_float32_state(gpu, potential):
    eng, tw = make_pair(gpu, 1025, potential=potential, dtype="f32", families=True)
    interleave(eng, tw)
    x = eng.download_state()[0]
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    eng.close()


def test_anneal_with_a_custom_potential(gpu):
    eng, tw = make_pair(gpu, 1025, potential=CustomPotential(CUSTOM), families=True)
    interleave(eng, tw)
    eng.close()


@pytest.mark.parametrize("where", [0, 2499, 1300])
def test_one_dominant_chain(gpu, where):
    """Every child from one parent, placed first, last and in the middle of a block: e = 900 against e = 0 under delta = 1.5."""
    M = 2500
    x = np.full(M, 30.0)
    x[where] = 0.0
    eng, tw = make_pair(gpu, M, x=x, families=True)
    for o in (eng, tw):
        o.anneal(2.0)
    compare(eng, tw)
    rec = eng.anneal_records()[0]
    assert rec.tolist()[4:] == [2 ** 30, rec[5], 1, M] and np.all(eng.download_families() == where)
    assert np.all(eng.download_state()[0] == 0.0) and eng.anneal_family_stats() == (1, M * M, M)
    eng.close()


def test_a_long_run_of_chains_without_weight(gpu):
    """700 consecutive zero-weight chains, [700, 1400), across block boundaries and the tile boundary at 1024, flanked by survivors;
    NaN positions among the survivors."""
    M = 2300
    x = start_x(M)
    x[700:1400] = 30.0
    x[[5, 1500, 2299]] = np.nan
    eng, tw = make_pair(gpu, M, x=x, families=True)
    for o in (eng, tw):
        o.anneal(2.0)
    compare(eng, tw)
    fam = eng.download_families()
    assert not np.any((fam >= 700) & (fam < 1400)) and not np.any(np.isin(fam, [5, 1500, 2299]))
    assert (fam < 700).any() and (fam >= 1400).any() and not np.isnan(eng.download_state()[0]).any()
    for o in (eng, tw):
        o.sweep(2); o.anneal(0.7)                # heating on
    compare(eng, tw)
    eng.close()


def test_statuses(gpu):
    M = 1030
    x = np.full(M, np.nan)
    eng, tw = make_pair(gpu, M, x=x, beta=1.0, families=True)
    for o in (eng, tw):
        o.anneal(2.0)
    compare(eng, tw)
    rec = eng.anneal_records()[0].tolist()
    assert rec == [1, A.f64_bits(1.0), A.f64_bits(2.0), 0x7FF8000000000000, 0, 0, 0, 0] and eng.beta == 2.0
    assert np.isnan(eng.download_state()[0]).all() and np.array_equal(eng.download_families(), np.arange(M))
    eng.close()
    x = start_x(M)
    x[3] = np.inf                                  # e = +Inf: heating gives it a = +Inf
    eng, tw = make_pair(gpu, M, x=x, beta=2.0, families=True)
    for o in (eng, tw):
        o.anneal(1.0)
    compare(eng, tw)
    assert eng.anneal_records()[0].tolist()[0] == 2 and np.array_equal(bits(eng.download_state()[0]), bits(x))
    for o in (eng, tw):
        o.anneal(3.0)                              # cooling: the chain has no weight and no child; the log goes on
    compare(eng, tw)
    assert 3 not in eng.download_families()
    eng.close()
    eng, tw = make_pair(gpu, 6, x=np.full(6, np.inf), beta=1.0)
    for o in (eng, tw):
        o.anneal(2.0)
    compare(eng, tw)
    assert eng.anneal_records()[0].tolist()[0] == 3
    eng.close()


def test_grid_independence_and_a_grid_walked_twice(gpu, monkeypatch):
    """300 001 chains: with one block per CU both the chain passes (256 x 256 threads) and the tile passes (256 x 1024 chains) walk
    their grid more than once.  The same bits under two AMC_BLOCKS_PER_CU settings, and those of the twin."""
    M = 300001
    out = []
    for bpc in ("1", "3"):
        monkeypatch.setenv("AMC_BLOCKS_PER_CU", bpc)
        eng, tw = make_pair(gpu, M, potential="double_well", families=True)
        monkeypatch.delenv("AMC_BLOCKS_PER_CU")
        eng.sweep(1); eng.anneal(1.1); eng.sweep(1); eng.anneal(0.8)
        out.append((bits(eng.download_state()[0]), eng.anneal_records(), eng.download_families(), eng.anneal_family_stats()))
        if bpc == "1":
            tw.sweep(1); tw.anneal(1.1); tw.sweep(1); tw.anneal(0.8)
            compare(eng, tw)
        eng.close()
    assert all(np.array_equal(a, b) for a, b in zip(out[0][:3], out[1][:3])) and out[0][3] == out[1][3]


def test_resume_at_the_engine(gpu):
    """x, beta, t_a, the records and the families put back into a fresh handle: it anneals on to the same bits."""
    a, tw = make_pair(gpu, 1025, potential="double_well", families=True)
    for o in (a, tw):
        o.sweep(1); o.anneal(0.9); o.sweep(1); o.anneal(1.4)
    b = gpu.HipEngine(n_chains=1025, potential="double_well", beta=0.5, sigma=[0.5], weight=[1.0], seed=23)
    b.upload_state(a.download_state()[0])
    b.beta, b.anneal_step, b.step = a.beta, a.anneal_step, a.step
    b.set_anneal_records(a.anneal_records())
    b.set_anneal_families(True)
    b.upload_families(a.download_families())
    b.upload_counters(*a.download_counters())
    for o in (a, b, tw):
        o.sweep(2); o.anneal(2.2)
    compare(a, tw); compare(b, tw)
    assert b.anneal_records(reset=True).shape == (3, 8) and b.anneal_records().shape == (0, 8) and b.anneal_step == 3
    a.close(); b.close()


def test_checkpoint_and_resume_through_run(gpu, tmp_path):
    betas = [0.5, 0.7, 1.0, 1.4, 2.0, 2.8, 4.0]

    def build(path, steps):
        chains = ma.ParticleChains.uniform(1025, betas[0], potential="double_well")
        pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
        al = [dict(algorithm=ma.Metropolis, pool=pool, seed=4, per_chain_counters=True),
              dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), betas=betas[1:], families=True),
              dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_energy, ma.callback_anneal_beta, ma.callback_anneal_log_z, ma.callback_rho_t),
                   scheduler=ma.build_schedule(steps, 0, 2))]
        return ma.Simulation(chains, al, steps, path=str(path))
    whole = build(tmp_path / "w", 12)
    ma.run(whole)
    first = build(tmp_path / "a", 6)
    ma.run(first)
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    second = build(tmp_path / "b", 6)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    e1, e2 = whole.algorithms[0].engine, second.algorithms[0].engine
    assert np.array_equal(bits(e1.download_state()[0]), bits(e2.download_state()[0]))
    assert np.array_equal(whole.algorithms[1].records(), second.algorithms[1].records()) and e1.anneal_step == e2.anneal_step == 6
    assert np.array_equal(e1.download_families(), e2.download_families()) and e1.beta == e2.beta == 4.0
    assert all(np.array_equal(a, b) for a, b in zip(e1.download_counters(), e2.download_counters()))
    assert np.array_equal(whole.algorithms[1].log_z(), second.algorithms[1].log_z()) and np.all(np.isfinite(whole.algorithms[1].log_z()))
    assert whole.algorithms[1].rho_t() >= 1.0


def test_the_buffers_are_allocated_at_the_first_step(gpu):
    """hipMemGetInfo around the first annealing step of a handle that has swept and reduced: the second position buffer and the word
    per chain (16 bytes per chain) appear then, not at amc_create -- a handle that never anneals never pays for them.  (Free memory
    of the whole device: another process allocating meanwhile only widens the drop.)"""
    hip = C.CDLL(gpu.runtime_info()["hip_runtime"])
    free, total = C.c_size_t(0), C.c_size_t(0)

    def free_bytes():
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    M = 1 << 22
    eng = gpu.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=3, per_chain_counters=False)
    eng.init_uniform(-2.0, 2.0)
    eng.sweep(2); eng.reduce(); eng.sync()
    assert eng.anneal_records().shape == (0, 8)              # asking for the records allocates nothing either
    before = free_bytes()
    eng.anneal(1.5); eng.sync()
    after = free_bytes()
    print(f"free before the first annealing step {before}, after {after}: {before - after} bytes")
    assert before - after >= 16 * M
    eng.close()


def test_refusals_leave_the_handle_as_it_was(gpu):
    kw = dict(potential="harmonic", sigma=[0.5], weight=[1.0], seed=23)
    M = 300
    x = start_x(M)
    with_beta = gpu.HipEngine(n_chains=M, beta=1.0, **kw)
    with_beta.upload_state(x, np.full(M, 1.0))
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*per-chain beta"):
        with_beta.anneal(2.0)
    with_beta.set_ladder(3)
    with pytest.raises(gpu.AmcError, match=r"amc error -5"):
        with_beta.anneal(2.0)
    with_beta.close()
    for off, glob in [(0, M + 2), (2, M + 2)]:
        part = gpu.HipEngine(n_chains=M, chain_offset=off, n_chains_global=glob, beta=1.0, **kw)
        part.upload_state(x)
        with pytest.raises(gpu.AmcError, match=r"amc error -5.*whole ensemble"):
            part.anneal(2.0)
        part.close()
    eng, tw = make_pair(gpu, M, beta=1.0)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(gpu.AmcError, match=r"amc error -1.*not finite"):
            eng.anneal(bad)
        with pytest.raises(gpu.AmcError, match=r"amc error -1.*not finite"):
            eng.beta = bad
    for call in (eng.anneal_family_stats, eng.download_families, lambda: eng.upload_families(np.zeros(M, dtype=np.uint32))):
        with pytest.raises(gpu.AmcError, match=r"amc error -5.*families are off"):
            call()
    eng.set_anneal_families(True)
    with pytest.raises(gpu.AmcError, match=r"amc error -1.*family id 300 >= n_chains"):
        eng.upload_families(np.full(M, M, dtype=np.uint32))
    eng.set_anneal_families(False)
    with pytest.raises(gpu.AmcError, match=r"amc error -1"):
        eng.anneal_step = 1 << 48
    full = np.zeros((gpu.AMC_ANNEAL_MAX_RECORDS, 8), dtype=np.uint64)
    eng.set_anneal_records(full)
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*record log is full"):
        eng.anneal(2.0)
    assert eng.beta == 1.0 and eng.anneal_step == 0
    eng.set_anneal_records(np.zeros((0, 8), dtype=np.uint64))
    # the refused handle still sweeps and anneals, and matches the twin
    for o in (eng, tw):
        o.sweep(2); o.anneal(2.0); o.sweep(1)
    compare(eng, tw)
    eng.close()
