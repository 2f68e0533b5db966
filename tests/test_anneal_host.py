"""Population annealing without a GPU: the host twin's own properties, the statuses, log Z of the harmonic
well against the exact value, the argument checks of the C ABI, and the Python layer (PopulationAnnealing over the engine_factory
seam: refusals, records, checkpoint / resume)."""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlo_amd as ma

import anneal_twin as A
import oracle_lib as O

POOL = lambda s=0.8: (ma.Move(ma.Displacement(), ma.StandardGaussian(), [s], 1.0),)


def make_twin(M, beta, x, *, seed=5, potential="harmonic", dtype="f64", families=False, sigma=0.8):
    sim = O.OracleSim(M, potential=potential, beta=beta, sigma=[sigma], weight=[1.0], seed=seed, dtype=dtype)
    sim.set_x(np.asarray(x, dtype=np.float64))
    return A.AnnealTwin(sim, beta, seed=seed, potential=potential, f32=dtype == "f32", families=families)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("M", [1, 2, 65, 257, 1000])
def test_children_counts_are_floor_or_ceil(oracle, M, dtype):
    x = 1.6 * np.sin(0.731 * np.arange(M) + 0.2)
    x[::7] = 40.0                                  # exp(-1.5 * 1600) = 0: chains without a weight
    if dtype == "f32":
        x = x.astype(np.float32).astype(np.float64)
    tw = make_twin(M, 0.5, x, dtype=dtype)
    tw.anneal(2.0)
    rec = tw.records[-1]
    if M == 1:
        assert rec[0] == A.OK and rec[6] == 1 and rec[7] == 1       # the one chain is its own child whatever its weight
        return
    W, counts, T_w = tw.last["W"], tw.last["counts"], rec[4]
    assert max(W) == 2 ** 30 and T_w == sum(W) and 0 <= rec[5] < T_w
    for w, n in zip(W, counts):
        assert (M * w) // T_w <= n <= -((-M * w) // T_w)
        assert w > 0 or n == 0
    assert any(w == 0 for w in W) and counts.sum() == M
    assert np.all(np.diff(tw.last["parents"]) >= 0)


def test_equal_beta_is_the_identity(oracle):
    x = 1.6 * np.sin(0.731 * np.arange(300) + 0.2)
    tw = make_twin(300, 1.25, x, families=True)
    for _ in range(3):                             # three different offsets U
        tw.anneal(1.25)
        assert np.array_equal(tw.x().view(np.uint64), x.view(np.uint64)) and np.array_equal(tw.fam, np.arange(300))
        assert tw.records[-1][0] == A.OK and tw.records[-1][4] == 300 * 2 ** 30 and tw.records[-1][6:] == [300, 1]
    assert tw.t_a == 3 and len({r[5] for r in tw.records}) == 3


def test_statuses(oracle):
    x = np.full(10, np.nan)
    tw = make_twin(10, 1.0, x)
    tw.anneal(2.0)
    assert tw.records[-1] == [A.ALL_NAN, A.f64_bits(1.0), A.f64_bits(2.0), 0x7FF8000000000000, 0, 0, 0, 0]
    assert np.all(np.isnan(tw.x())) and tw.beta == 2.0 and tw.t_a == 1
    x = np.linspace(-1, 1, 10)
    x[3] = np.inf                                  # e = +Inf: heating gives it a = +Inf, cooling a = -Inf (no weight)
    tw = make_twin(10, 2.0, x)
    tw.anneal(1.0)
    assert tw.records[-1][0] == A.INF and tw.records[-1][3] == A.f64_bits(math.inf) and tw.records[-1][4:] == [0, 0, 0, 0]
    assert np.array_equal(tw.x().view(np.uint64), x.view(np.uint64)) and tw.beta == 1.0
    tw.anneal(3.0)
    assert tw.records[-1][0] == A.OK and 3 not in tw.last["parents"]
    tw = make_twin(4, 1.0, np.full(4, np.inf))
    tw.anneal(2.0)
    assert tw.records[-1][0] == A.NO_WEIGHT and tw.records[-1][3] == A.f64_bits(-math.inf)


# ---- log Z of the harmonic well -----------------------------------------------------------------------------------------------------
LOGZ_M, LOGZ_SWEEPS = 2000, 4
LOGZ_BETAS = [0.5 * 8.0 ** (i / 8.0) for i in range(9)]        # 0.5 .. 4 in 8 geometric steps
LOGZ_SPREAD = 0.01025                                           # measured, see the test's docstring
LOGZ_TOL = 5.0 * LOGZ_SPREAD


def harmonic_log_z(seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, math.sqrt(1.0 / (2.0 * LOGZ_BETAS[0])), LOGZ_M)      # equilibrium at the first beta: e = x^2
    tw = make_twin(LOGZ_M, LOGZ_BETAS[0], x, seed=seed)
    for b in LOGZ_BETAS[1:]:
        tw.anneal(b)
        tw.sweep(LOGZ_SWEEPS)
    return float(A.log_z_ratios(tw.records, LOGZ_M).sum())


@pytest.mark.parametrize("seed", [101, 202])
def test_log_z_of_the_harmonic_well(oracle, seed):
    """log(Z(4) / Z(0.5)) = log(0.5 / 4) / 2 for e = x^2, from one annealing run of 2000 chains over 8 geometric steps with 4 sweeps
    (sigma = 0.8) behind each.  The tolerance is the twin's own spread: over the 24 seeds 1 .. 24 at this population size the estimate
    has mean -1.03583 (exact: -1.03972) and standard deviation 0.01025 (sample, n - 1); five standard deviations, 0.05125, so that a correct twin fails
    about once in 10^6 runs.  (profiles/population_annealing.md holds the same figures.)"""
    got, want = harmonic_log_z(seed), 0.5 * math.log(LOGZ_BETAS[0] / LOGZ_BETAS[-1])
    print(f"log Z estimate {got!r}, exact {want!r}, tolerance {LOGZ_TOL}")
    assert abs(got - want) <= LOGZ_TOL


# ---- the C ABI's argument checks (no device is touched) ----------------------------------------------------------------------------------
def test_new_entries_refuse_a_null_handle(amc):
    lib = amc.load()
    for name in ("amc_anneal", "amc_anneal_fetch", "amc_set_anneal_records", "amc_get_anneal_step", "amc_set_anneal_step", "amc_get_beta",
                 "amc_set_beta", "amc_set_anneal_families", "amc_anneal_family_stats", "amc_download_families", "amc_upload_families"):
        res, args = amc.SIGNATURES[name]
        vals = [None] + [0 if t in (C.c_int, C.c_uint64) else 0.0 if t is C.c_double else None for t in args[1:]]
        assert getattr(lib, name)(*vals) == -1 and name.encode() in lib.amc_last_error()


# ---- the Python layer over the engine_factory seam ----------------------------------------------------------------------------------------
def build(path, steps, betas, *, every=2, families=False, M=64, callbacks=(), factory=A.AnnealTwinEngine, chains=None, extra=()):
    chains = chains or ma.ParticleChains.uniform(M, betas[0], potential="double_well")
    al = [dict(algorithm=ma.Metropolis, pool=POOL(0.5), seed=4, engine_factory=factory),
          dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, every), betas=betas[1:],
               families=families)]
    al += list(extra)
    if callbacks:
        al.append(dict(algorithm=ma.StoreCallbacks, callbacks=tuple(callbacks), scheduler=ma.build_schedule(steps, 0, every)))
    return ma.Simulation(chains, al, steps, path=str(path))


def test_run_anneals_through_the_list(oracle, tmp_path):
    betas = [0.5, 0.8, 1.2, 1.7, 2.5]
    sim = build(tmp_path, 8, betas, families=True, callbacks=(ma.callback_anneal_beta, ma.callback_anneal_log_z, ma.callback_rho_t))
    ma.run(sim)
    pa, eng = sim.algorithms[1], sim.algorithms[0].engine
    rec = pa.records()
    assert rec.shape == (4, 8) and eng.anneal_step == 4 and pa.beta == 2.5 and sim.chains.beta == 2.5
    assert [A.bits_f64(b) for b in rec[:, 2]] == betas[1:] and np.array_equal(pa.betas_done(), betas[1:])
    assert np.array_equal(pa.log_z_ratios(), A.log_z_ratios(rec, 64)) and np.array_equal(pa.log_z(), np.cumsum(pa.log_z_ratios()))
    assert np.array_equal(pa.survival(), rec[:, 6] / 64.0) and np.all(pa.survival() <= 1.0)
    alive, sq, largest = pa.family_stats()
    assert alive <= 64 and sq >= 64 and pa.rho_t() == sq / 64.0 and largest >= 1
    rows = [ln.split() for ln in open(tmp_path / "anneal_beta.dat").read().splitlines()]
    assert [float(r[-1]) for r in rows[-4:]] == betas[1:]
    assert float(open(tmp_path / "anneal_log_z.dat").read().splitlines()[-1].split()[-1]) == pytest.approx(pa.log_z()[-1])
    # the same schedule stepped by hand on a twin of its own
    ref = A.AnnealTwinEngine(n_chains=64, potential="double_well", beta=0.5, sigma=[0.5], weight=[1.0], seed=4)
    ref.init_uniform(-2.0, 2.0)
    for b in betas[1:]:
        ref.sweep(2); ref.anneal(b)
    assert np.array_equal(ref.download_state()[0].view(np.uint64), eng.download_state()[0].view(np.uint64))


def test_refusals_of_the_python_layer(oracle, tmp_path, monkeypatch):
    betas = [0.5, 1.0, 2.0]
    ladder = ma.ParticleChains.ladder(8, [0.5, 1.0], potential="harmonic")
    with pytest.raises(ValueError, match="PopulationAnnealing: the chains carry a per-chain beta array"):
        build(tmp_path / "a", 4, betas, chains=ladder)
    with pytest.raises(ValueError, match=r"PopulationAnnealing: this engine has no annealing step \(streams > 1"):
        build(tmp_path / "b", 4, betas, factory=O.OracleEngine)
    with pytest.raises(ValueError, match="PopulationAnnealing: betas is missing"):
        build(tmp_path / "c", 4, betas[:1])
    with pytest.raises(ValueError, match=r"PopulationAnnealing: betas\[1\] = nan is not finite"):
        build(tmp_path / "d", 4, [0.5, 1.0, math.nan])
    from montecarlo_amd import sharding
    monkeypatch.setattr(sharding, "world", lambda: (0, 2))
    monkeypatch.setattr(sharding, "connect_engine", lambda eng: False)
    with pytest.raises(ValueError, match="PopulationAnnealing: 2 ranks"):
        build(tmp_path / "e", 4, betas, M=128)
    monkeypatch.undo()
    sim = build(tmp_path / "f", 6, betas)                 # three calls are due, the list holds two
    with pytest.raises(ValueError, match="PopulationAnnealing: annealing step 3 is due and betas holds 2 values"):
        ma.run(sim)
    with pytest.raises(ValueError, match="PopulationAnnealing.family_stats needs the families"):
        sim.algorithms[1].family_stats()


def test_a_replica_exchange_in_the_same_list_is_refused(oracle, tmp_path):
    class FakeExchange(ma.ReplicaExchange):
        def __init__(self, chains, **kw):
            pass
    sim = build(tmp_path, 4, [0.5, 1.0, 2.0], extra=[dict(algorithm=FakeExchange)])
    with pytest.raises(ValueError, match="PopulationAnnealing: the algorithm list holds a ReplicaExchange"):
        ma.run(sim)


def test_checkpoint_carries_the_annealing_state(oracle, tmp_path):
    betas = [0.5, 0.7, 1.0, 1.4, 2.0, 2.8, 4.0]
    whole = build(tmp_path / "w", 12, betas, families=True)
    ma.run(whole)
    first = build(tmp_path / "a", 6, betas, families=True)
    ma.run(first)
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    assert first.algorithms[1].records().shape == (3, 8)          # the checkpoint left the records where they were
    second = build(tmp_path / "b", 6, betas, families=True)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    assert second.algorithms[1].beta == 1.4 and second.algorithms[0].engine.anneal_step == 3
    ma.run(second)
    e1, e2 = whole.algorithms[0].engine, second.algorithms[0].engine
    assert np.array_equal(e1.download_state()[0].view(np.uint64), e2.download_state()[0].view(np.uint64))
    assert np.array_equal(whole.algorithms[1].records(), second.algorithms[1].records())
    assert np.array_equal(e1.download_families(), e2.download_families()) and e1.anneal_step == e2.anneal_step == 6
    assert all(np.array_equal(a, b) for a, b in zip(e1.download_counters(), e2.download_counters()))
