"""Weight sums per block of families on the device (DESIGN.md section 3.14 "Error bars"; include/amc.h amc_set_anneal_blocks ..
amc_anneal_block_counts) against the host twin (tests/anneal_blocks_twin.py), bit for bit: the block records under every partition,
beside positions, records and families, which the partition must leave alone.  Shapes: one and two chains, below, at and past one
ANNEAL_TILE (1024 chains) and several tiles; 2, 3 and 64 blocks; a chunk of 1 (every lane of a wave in another block), the default
(a block is a contiguous range) and one above M (every chain in block 0).  The twin runs once per (M, potential, type): the resampling
does not depend on the partition, so its weights give the block records under any of them."""
import math

import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd import jackknife
from montecarlo_amd.system import CustomPotential

import anneal_blocks_twin as AB
import oracle_lib as O

pytestmark = pytest.mark.gpu
CUSTOM = "x*x*x*x - 2.0*x*x + 0.25*x"
SIGMA, WEIGHT, SEED = [0.5], [1.0], 23
STEPS = ((1, 0.9), (2, 2.0), (1, 1.25))          # (sweeps in front, beta): three steps, cooling and heating


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def start_x(M, dtype="f64"):
    ids = np.arange(M)
    x = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)
    return x.astype(np.float32).astype(np.float64) if dtype == "f32" else x


def engine(gpu, M, potential="harmonic", dtype="f64", beta=0.5, x=None):
    eng = gpu.HipEngine(n_chains=M, potential=potential, beta=beta, sigma=SIGMA, weight=WEIGHT, seed=SEED, dtype=dtype)
    eng.upload_state(start_x(M, dtype) if x is None else x)
    return eng


def twin(M, potential="harmonic", dtype="f64", beta=0.5, x=None, fam=None, steps=STEPS):
    sim = O.OracleSim(M, potential=potential, beta=beta, sigma=SIGMA, weight=WEIGHT, seed=SEED, dtype=dtype)
    sim.set_x(start_x(M, dtype) if x is None else x)
    tw = AB.AnnealBlocksTwin(sim, beta, blocks=2, seed=SEED, potential=potential, f32=dtype == "f32")
    if fam is not None:
        tw.fam = np.asarray(fam, dtype=np.uint32).copy()
    for sweeps, b in steps:
        if sweeps:
            tw.sweep(sweeps)
        tw.anneal(b)
    return tw


_TWINS = {}


def shared_twin(M, potential="harmonic", dtype="f64"):
    """The reference of (M, potential, type), computed once and left unchanged."""
    key = (M, str(potential), dtype)
    if key not in _TWINS:
        _TWINS[key] = twin(M, potential, dtype)
    return _TWINS[key]


def run_steps(eng, steps=STEPS):
    for sweeps, b in steps:
        if sweeps:
            eng.sweep(sweeps)
        eng.anneal(b)


def restart(eng, M, dtype, B, chunk):
    """The engine back at the start state with families afresh and the partition (B, chunk)."""
    eng.upload_state(start_x(M, dtype))
    eng.beta, eng.step, eng.anneal_step = 0.5, 0, 0
    eng.anneal_records(reset=True)
    eng.set_anneal_families(True)
    eng.set_anneal_blocks(B, chunk)


def compare(eng, tw, B, chunk):
    c = chunk or AB.default_chunk(tw.M, B)
    want = AB.block_records_under(tw.weights, B, c)
    got = eng.anneal_block_records()
    assert got.shape == want.shape and np.array_equal(got, want), ("block records differ from the twin", B, chunk, got.tolist(), want.tolist())
    rec = eng.anneal_records()
    assert np.array_equal(rec, tw.records_array()), "records differ from the twin"
    assert np.all(got[:, 0].sum(axis=1) == tw.M) and np.array_equal(got[:, 1].sum(axis=1), rec[:, 4])
    assert np.array_equal(bits(eng.download_state()[0]), bits(tw.x())), "positions differ from the twin"
    assert np.array_equal(eng.download_families(), tw.fam), "families differ from the twin"
    assert np.array_equal(eng.anneal_block_counts(), np.bincount(AB.block_of(tw.fam, B, c), minlength=B))


@pytest.mark.parametrize("B", [2, 3, 64])
@pytest.mark.parametrize("M", [1, 2, 255, 1024, 1025, 4099])
def test_block_records_match_the_twin(gpu, M, B):
    tw = shared_twin(M)
    eng = engine(gpu, M)
    for chunk in (1, 0, M + 7):
        restart(eng, M, "f64", B, chunk)
        run_steps(eng)
        compare(eng, tw, B, chunk)
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("potential", ["harmonic", "double_well", CustomPotential(CUSTOM)], ids=["harmonic", "double_well", "custom"])
def test_potentials_and_float32_state(gpu, potential, dtype):
    M = 1025
    tw = shared_twin(M, potential, dtype)
    eng = engine(gpu, M, potential, dtype)
    for B, chunk in ((3, 1), (64, 0), (2, M + 7)):
        restart(eng, M, dtype, B, chunk)
        run_steps(eng)
        compare(eng, tw, B, chunk)
    eng.close()


@pytest.mark.parametrize("B,chunk", [(3, 0), (64, 1), (5, 7)])
def test_family_ids_in_any_order(gpu, B, chunk):
    """Ids put in through upload_families, a permutation that is not monotone: nothing may rest on the order."""
    M = 1025
    fam = (np.arange(M, dtype=np.int64) * 389) % M            # 389 and 1025 are coprime
    tw = twin(M, fam=fam)
    eng = engine(gpu, M)
    eng.set_anneal_families(True)
    eng.set_anneal_blocks(B, chunk)
    eng.upload_families(fam.astype(np.uint32))                # (an upload leaves the partition standing)
    run_steps(eng)
    compare(eng, tw, B, chunk)
    eng.close()


def test_one_chain_takes_nearly_all_the_weight(gpu):
    """e = 900 against e = 0 under delta = 1.5: every child from chain 1300, every block but its own dies; the next step sees one
    block with all M chains."""
    M, B = 2500, 8
    x = np.full(M, 30.0)
    x[1300] = 0.0
    steps = ((0, 2.0), (1, 2.5))
    tw = twin(M, x=x, steps=steps)
    eng = engine(gpu, M, x=x)
    eng.set_anneal_families(True)
    eng.set_anneal_blocks(B)
    run_steps(eng, steps)
    compare(eng, tw, B, 0)
    blk = eng.anneal_block_records()
    b = 1300 // AB.default_chunk(M, B)
    assert blk[0, 1].tolist() == [2 ** 30 if k == b else 0 for k in range(B)] and blk[1, 0].tolist() == [M if k == b else 0 for k in range(B)]
    value, se, rep = jackknife.anneal_log_z(eng.anneal_records(), blk, M)
    assert np.isfinite(value).all() and np.isnan(rep[:, b]).all() and np.isnan(se).all()
    eng.close()


def test_a_step_on_nan_positions(gpu):
    """Status 1: n_b is counted, T_b reads 0, and the log goes on."""
    M, B = 1030, 3
    eng = engine(gpu, M, beta=1.0, x=np.full(M, np.nan))
    eng.set_anneal_families(True)
    eng.set_anneal_blocks(B)
    eng.anneal(2.0)
    blk = eng.anneal_block_records()
    assert eng.anneal_records()[0, 0] == 1 and blk.shape == (1, 2, B)
    assert blk[0, 0].tolist() == [344, 344, 342] and blk[0, 1].tolist() == [0, 0, 0]
    eng.close()


def test_the_partition_leaves_the_run_alone(gpu):
    M = 4099
    out = []
    for B in (0, 64):
        eng = engine(gpu, M, "double_well")
        eng.set_anneal_families(True)
        if B:
            eng.set_anneal_blocks(B)
        run_steps(eng)
        out.append((bits(eng.download_state()[0]), eng.anneal_records(), eng.download_families()))
        eng.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out))


def test_grid_independence_and_a_grid_walked_twice(gpu, monkeypatch):
    """300 001 chains under one block per CU: the pass (4 x 256 chains per block and trip) walks its grid more than once.  The same
    block records under two AMC_BLOCKS_PER_CU settings; n_b of the first step in closed form; the sums add up."""
    M, B = 300001, 64
    out = []
    for bpc in ("1", "3"):
        monkeypatch.setenv("AMC_BLOCKS_PER_CU", bpc)
        eng = engine(gpu, M, "double_well")
        monkeypatch.delenv("AMC_BLOCKS_PER_CU")
        eng.set_anneal_families(True)
        eng.set_anneal_blocks(B)
        eng.sweep(1); eng.anneal(1.1); eng.sweep(1); eng.anneal(0.8)
        out.append((eng.anneal_block_records(), eng.anneal_records(), eng.download_families(), eng.anneal_block_counts()))
        eng.close()
    blk, rec, fam, now = out[0]
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1]))
    c = AB.default_chunk(M, B)
    assert np.array_equal(blk[0, 0], np.bincount(np.arange(M) // c, minlength=B)) and np.array_equal(now, np.bincount(fam // c, minlength=B))
    assert np.all(blk[:, 0].sum(axis=1) == M) and np.array_equal(blk[:, 1].sum(axis=1), rec[:, 4])


def test_fetch_reset_and_set(gpu):
    M, B = 1025, 3
    eng = engine(gpu, M)
    eng.set_anneal_families(True)
    eng.set_anneal_blocks(B, 10)
    assert eng.anneal_block_records().shape == (0, 2, B)
    run_steps(eng)
    a = eng.anneal_block_records()
    assert a.shape == (3, 2, B) and np.array_equal(eng.anneal_block_records(reset=True), a) and eng.anneal_block_records().shape == (0, 2, B)
    assert eng.anneal_records().shape == (3, 8)                 # the records' log is a log of its own
    eng.set_anneal_block_records(a[:2])
    assert np.array_equal(eng.anneal_block_records(), a[:2])
    eng.anneal(1.5)
    got = eng.anneal_block_records()
    assert got.shape == (3, 2, B) and np.array_equal(got[:2], a[:2]) and got[2, 0].sum() == M
    with pytest.raises(gpu.AmcError, match="n_blocks = 4, the partition has 3 blocks"):
        eng.set_anneal_block_records(np.zeros((1, 2, 4), dtype=np.uint64))
    eng.set_anneal_block_records(np.zeros((0, 2, B), dtype=np.uint64))
    assert eng.anneal_block_records().shape == (0, 2, B)
    eng.close()


def test_states_that_are_refused(gpu):
    M = 300
    eng = engine(gpu, M)
    with pytest.raises(gpu.AmcError, match="amc_set_anneal_blocks: families are off"):
        eng.set_anneal_blocks(4)
    eng.set_anneal_blocks(0)                                    # off is never refused
    for call in (eng.anneal_block_records, eng.anneal_block_counts):
        with pytest.raises(gpu.AmcError, match="no partition over the families is set"):
            call()
    eng.set_anneal_families(True)
    for bad in (1, 65, -2):
        with pytest.raises(gpu.AmcError, match="amc_set_anneal_blocks: n_blocks"):
            eng.set_anneal_blocks(bad)
    with pytest.raises(gpu.AmcError, match="amc_set_anneal_blocks: chunk"):
        eng.set_anneal_blocks(4, -1)
    eng.set_blocks(4)
    with pytest.raises(gpu.AmcError, match="a partition over the ladders is set"):
        eng.set_anneal_blocks(4)
    with pytest.raises(gpu.AmcError, match="amc_anneal: a partition is set"):
        eng.anneal(1.0)                                         # amc_set_blocks keeps refusing
    eng.set_blocks(0)
    eng.set_anneal_blocks(4)
    with pytest.raises(gpu.AmcError, match="a partition over the annealing families is set"):
        eng.set_blocks(4)
    eng.anneal(1.0)
    assert eng.anneal_block_records().shape == (1, 2, 4)
    eng.set_anneal_blocks(5, 3)                                 # another partition: the log starts afresh
    assert eng.anneal_block_records().shape == (0, 2, 5) and eng.anneal_block_counts().tolist() != []
    eng.set_anneal_families(True)                               # families afresh: the partition goes
    with pytest.raises(gpu.AmcError, match="no partition over the families is set"):
        eng.anneal_block_records()
    eng.set_anneal_blocks(4)
    eng.set_anneal_families(False)
    with pytest.raises(gpu.AmcError, match="no partition over the families is set"):
        eng.anneal_block_counts()
    eng.anneal(1.5)                                             # and the handle anneals on
    assert eng.anneal_records().shape == (2, 8)
    eng.close()


# ---- the energy histogram per block of families ---------------------------------------------------------------------------------------
def histogram_checks(eng, tw, B, chunk, lo, hi, n):
    """One snapshot under the partition: against the twin, against its own sum, against the plain pass of the same state."""
    c = chunk or AB.default_chunk(tw.M, B)
    eng.energy_histogram_accumulate_blocks(lo, hi, n)
    got, snaps, bins = eng.energy_histogram_fetch_blocks()
    want = AB.histogram_by_block(tw.potential, tw.x(), tw.fam, B, c, lo, hi, n, tw.f32)
    assert got.shape == (B, 1, n + 3) and snaps == 1 and bins == (lo, hi, n)
    assert np.array_equal(got[:, 0], want), ("the histogram per block differs from the twin", B, chunk, n)
    summed, snaps, _ = eng.energy_histogram_fetch(reset=True)          # the sum over the blocks, formed by the engine
    assert snaps == 1 and np.array_equal(summed[0], got[:, 0].sum(axis=0, dtype=np.uint64))
    eng.set_anneal_blocks(0)
    eng.energy_histogram_accumulate(lo, hi, n)
    plain = eng.energy_histogram_fetch(reset=True)[0]
    assert np.array_equal(plain, summed), "the sum over the blocks is not the plain histogram"
    eng.set_anneal_blocks(B, chunk)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("potential", ["harmonic", "double_well", CustomPotential(CUSTOM)], ids=["harmonic", "double_well", "custom"])
def test_histogram_per_block_matches_the_twin(gpu, potential, dtype):
    M = 1025
    tw = shared_twin(M, potential, dtype)
    eng = engine(gpu, M, potential, dtype)
    restart(eng, M, dtype, 3, 1)
    run_steps(eng)
    for B, chunk, n in ((3, 1, 40), (64, 0, 188), (64, 7, 190), (2, M + 7, 7)):      # 64 x 191 = 12 224 cells in LDS, 64 x 193 = 12 352 beyond
        eng.set_anneal_blocks(B, chunk)
        histogram_checks(eng, tw, B, chunk, -1.5, 3.0, n)
    eng.close()


@pytest.mark.parametrize("M", [1, 255, 4099])
def test_histogram_per_block_at_other_sizes(gpu, M):
    tw = shared_twin(M)
    eng = engine(gpu, M)
    restart(eng, M, "f64", 2, 0)
    run_steps(eng)
    for B, chunk, n in ((2, 0, 5), (64, 1, 188), (64, 1, 190)):
        eng.set_anneal_blocks(B, chunk)
        histogram_checks(eng, tw, B, chunk, 0.0, 2.0, n)
    eng.close()


def test_histogram_per_block_accumulates_restores_and_folds(gpu):
    M, B = 1025, 5
    eng = engine(gpu, M, "double_well")
    eng.set_anneal_families(True)
    eng.set_anneal_blocks(B, 3)
    run_steps(eng)
    eng.energy_histogram_accumulate_blocks(0.0, 2.0, 30)
    one = eng.energy_histogram_fetch_blocks()[0]
    eng.sweep(1)
    eng.energy_histogram_accumulate_blocks(0.0, 2.0, 30)
    two, snaps, bins = eng.energy_histogram_fetch_blocks(reset=True)
    assert snaps == 2 and np.all(two >= one) and two.sum() == 2 * M
    with pytest.raises(gpu.AmcError, match="no accumulator kept per jackknife block stands"):
        eng.energy_histogram_fetch_blocks()
    eng.set_energy_histogram_blocks(0.0, 2.0, 30, two, 2)              # what a checkpoint puts back
    back, snaps, _ = eng.energy_histogram_fetch_blocks()
    assert snaps == 2 and np.array_equal(back, two)
    with pytest.raises(gpu.AmcError, match="the cells do not sum to n_snapshots"):
        eng.set_energy_histogram_blocks(0.0, 2.0, 30, two, 3)
    eng.set_energy_histogram_blocks(0.0, 2.0, 30, two, 2)
    eng.set_anneal_blocks(0)                                           # the partition goes: folded into a plain accumulator, nothing lost
    plain, snaps, _ = eng.energy_histogram_fetch(reset=True)
    assert snaps == 2 and np.array_equal(plain[0], two[:, 0].sum(axis=0, dtype=np.uint64))
    with pytest.raises(gpu.AmcError, match="no partition is set"):
        eng.energy_histogram_accumulate_blocks(0.0, 2.0, 30)
    eng.close()


# ---- the Python layer on the device ------------------------------------------------------------------------------------------------------
POOL = lambda s=0.5: (ma.Move(ma.Displacement(), ma.StandardGaussian(), [s], 1.0),)


def build(path, steps, betas, *, every=2, M=1025, potential="double_well", x=None, sigma=0.5, **pa):
    chains = ma.ParticleChains.uniform(M, betas[0], potential=potential) if x is None else ma.ParticleChains(M, betas[0], potential, x=x)
    al = [dict(algorithm=ma.Metropolis, pool=POOL(sigma), seed=4),
          dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, every), betas=betas[1:], **pa)]
    return ma.Simulation(chains, al, steps, path=str(path))


def test_checkpoint_in_mid_run(gpu, tmp_path):
    betas = [0.5, 0.7, 1.0, 1.4, 2.0, 2.8, 4.0]
    hist = dict(lo=0.0, hi=12.0, n_bins=120, max_outside=0.01)      # (the uniform start reaches past x = 2.1, e > 12, at beta = 0.5)
    whole = build(tmp_path / "w", 12, betas, blocks=8, energy_histogram=hist)
    ma.run(whole)
    first = build(tmp_path / "a", 6, betas, blocks=8, energy_histogram=hist)
    ma.run(first)
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    second = build(tmp_path / "b", 6, betas, blocks=8, energy_histogram=hist)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    pw, ps = whole.algorithms[1], second.algorithms[1]
    hw, hs = pw.histograms_blocks(), ps.histograms_blocks()
    assert hw[1].shape == (7, 8, 123) and np.array_equal(hw[1], hs[1]) and np.array_equal(hw[1].sum(axis=1), pw.histograms()[1])
    rw, rs = pw.reweight([1.0, 3.0], error=True), ps.reweight([1.0, 3.0], error=True)
    assert all(np.array_equal(x, y) for x, y in zip(rw[0] + rw[1], rs[0] + rs[1])) and all(np.all(v > 0) for v in rw[1])
    assert ps.block_records().shape == (6, 2, 8) and np.array_equal(pw.block_records(), ps.block_records())
    assert np.array_equal(pw.records(), ps.records())
    a, b = pw.log_z(error=True), ps.log_z(error=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.all(a[1] > 0)
    e1, e2 = whole.algorithms[0].engine, second.algorithms[0].engine
    assert np.array_equal(bits(e1.download_state()[0]), bits(e2.download_state()[0]))
    assert np.array_equal(e1.download_families(), e2.download_families())


# The spread of log Z over 64 seeds that tests/test_anneal_blocks_host.py measures on the twin at M = 4096 for this very schedule
# (profiles/population_annealing_blocks.md): the standard deviation of an estimate falls as 1 / sqrt(M).
CAL_M, CAL_STD = 4096, 0.0060798


def test_a_run_of_65536_chains(gpu, tmp_path):
    """M = 65 536 harmonic (e = x^2), B = 32, beta 1 -> 4 in six geometric steps with 5 sweeps (sigma = 0.8) in front of each, from
    equilibrium at beta = 1: log Z within 5 se of log(1 / 4) / 2, and the se inside the CPU calibration's interval
    (test_anneal_blocks_host.calibration_interval: the chi^2_63 quantiles at the 10^-3 level, widened by 2.5 %) of the spread predicted
    there, 0.0060798 sqrt(4096 / 65 536) = 0.00152."""
    from scipy.stats import chi2
    M, B = 65536, 32
    betas = [4.0 ** (i / 6.0) for i in range(7)]
    x = np.random.default_rng(7).normal(0.0, math.sqrt(0.5), M)
    sim = build(tmp_path, 30, betas, every=5, M=M, potential="harmonic", x=x, sigma=0.8, blocks=B)
    ma.run(sim)
    pa = sim.algorithms[1]
    value, se = pa.log_z(error=True)
    exact, predicted = 0.5 * math.log(betas[0] / betas[-1]), CAL_STD * math.sqrt(CAL_M / M)
    lo, hi = (1 - 0.025) / math.sqrt(chi2.ppf(1 - 5e-4, 63) / 63), (1 + 0.025) / math.sqrt(chi2.ppf(5e-4, 63) / 63)
    print(f"log Z {value[-1]!r} +- {se[-1]!r}, exact {exact!r}, predicted spread {predicted!r}, se / predicted {se[-1] / predicted!r} in [{lo!r}, {hi!r}]")
    assert value.shape == (6,) and pa.block_records().shape == (6, 2, B)
    assert abs(value[-1] - exact) <= 5.0 * se[-1]
    assert lo * predicted <= se[-1] <= hi * predicted
