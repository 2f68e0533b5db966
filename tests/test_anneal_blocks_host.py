"""Error bars for population annealing without a GPU (DESIGN.md section 3.14 "Error bars"): the block records of the host twin
(tests/anneal_blocks_twin.py) and their invariants, jackknife.anneal_log_z against a brute-force leave-one-block-out recomputation
from the chains' own weights, blocks that die out, the NaN-replicate rule, the calibration of the error bar over 64 seeds, the C ABI's
argument checks, and the Python layer (PopulationAnnealing(blocks=B) over the engine_factory seam: records, callback, refusals,
checkpoint / resume)."""
import ctypes as C
import math

import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd import jackknife, reweighting

import anneal_blocks_twin as AB
import anneal_twin as A
import ehist_twin as E
import oracle_lib as O

POOL = lambda s=0.8: (ma.Move(ma.Displacement(), ma.StandardGaussian(), [s], 1.0),)


def make_twin(M, beta, x, *, blocks, chunk=0, seed=5, potential="harmonic", dtype="f64", sigma=0.8):
    sim = O.OracleSim(M, potential=potential, beta=beta, sigma=[sigma], weight=[1.0], seed=seed, dtype=dtype)
    sim.set_x(np.asarray(x, dtype=np.float64))
    return AB.AnnealBlocksTwin(sim, beta, blocks=blocks, chunk=chunk, seed=seed, potential=potential, f32=dtype == "f32")


def same(a, b):
    return np.allclose(a, b, rtol=1e-13, atol=1e-13, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))


# ---- the block records and the jackknife formula ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,chunk", [(2, 0), (3, 1), (8, 0), (5, 7), (64, 0)])
def test_block_records_add_up_and_the_jackknife_matches_brute_force(oracle, B, chunk):
    M = 301
    x = 1.6 * np.sin(0.731 * np.arange(M) + 0.2)
    tw = make_twin(M, 0.5, x, blocks=B, chunk=chunk, potential="double_well")
    for beta in (0.8, 1.3, 2.1, 1.7):
        tw.sweep(2)
        tw.anneal(beta)
    rec, blk = tw.records_array(), tw.block_records_array()
    assert blk.shape == (4, 2, B)
    assert np.all(blk[:, 0].sum(axis=1) == M) and np.array_equal(blk[:, 1].sum(axis=1), rec[:, 4])      # sum n_b = M, sum T_b = T_w
    c = tw.chunk
    assert np.array_equal(blk[0, 0], np.bincount((np.arange(M) // c) % B, minlength=B))                 # fam[c] = c at the first step
    assert np.array_equal(tw.block_counts(), np.bincount(AB.block_of(tw.fam, B, c), minlength=B))
    value, se, rep = jackknife.anneal_log_z(rec, blk, M)
    v0, se0, rep0 = AB.brute_force_log_z(tw.weights, M, B)
    assert same(value, v0) and same(rep, rep0) and same(se, se0)
    assert np.array_equal(AB.block_records_under(tw.weights, B, c), blk)
    assert np.array_equal(value, np.cumsum(A.log_z_ratios(rec, M))) and np.all(np.isfinite(se)) and np.all(se > 0)
    # per step: the same replicates, not accumulated
    v1, se1, rep1 = jackknife.anneal_log_z(rec, blk, M, cumulative=False)
    assert np.array_equal(v1, A.log_z_ratios(rec, M)) and same(np.cumsum(rep1, axis=0), rep)
    assert se1[0] == se[0] and not same(se1[1:], se[1:])          # the replicate of the sum, not a sum of per-step errors


def test_blocks_that_die_out_stay_replicates(oracle):
    """The chains of block 0 sit far up the well and leave no child: the block is empty from the second step on, its replicate is
    the full estimate's term there, and it still counts among the B' = 4 of the variance."""
    M, B = 200, 4
    x = 0.9 * np.sin(0.731 * np.arange(M) + 0.2)
    x[:50] = 30.0
    tw = make_twin(M, 0.5, x, blocks=B)
    for beta in (2.0, 3.0):
        tw.anneal(beta)
        tw.sweep(1)
    blk = tw.block_records_array()
    assert blk[0, 0].tolist() == [50, 50, 50, 50] and blk[0, 1, 0] == 0 and blk[1, 0, 0] == 0 and blk[1, 1, 0] == 0
    value, se, rep = jackknife.anneal_log_z(tw.records_array(), blk, M)
    v0, se0, rep0 = AB.brute_force_log_z(tw.weights, M, B)
    assert same(rep, rep0) and same(se, se0) and np.all(np.isfinite(rep)) and np.all(se > 0)
    assert rep[1, 0] - rep[0, 0] == value[1] - value[0]           # without the dead block nothing is left out at step 2
    th = rep[1]
    assert se[1] == pytest.approx(math.sqrt(3 / 4 * ((th - th.mean()) ** 2).sum()), rel=1e-13)


def test_a_replicate_whose_argument_is_zero_is_nan_from_that_step_on(oracle):
    """One chain takes all the weight: every child belongs to its family, so at the NEXT step its block holds all M chains and the
    replicate without it has no chain left -- NaN from there on, and the se with it.  At the first step the replicate without the
    dominant block has chains and no weight: NaN at once."""
    M, B = 120, 3
    x = np.full(M, 30.0)
    x[70] = 0.0                                     # block 1 of 3 (chunk 40)
    tw = make_twin(M, 0.5, x, blocks=B)
    tw.anneal(2.0)
    _, se, rep = jackknife.anneal_log_z(tw.records_array(), tw.block_records_array(), M)
    assert np.isnan(rep[0, 1]) and np.isfinite(rep[0, [0, 2]]).all() and np.isnan(se[0])       # T_w - T_1 = 0
    x = 0.9 * np.sin(0.731 * np.arange(M) + 0.2)
    tw = make_twin(M, 0.5, x, blocks=B)
    tw.anneal(0.7)
    tw.sim.set_x(np.where(np.arange(M) == 5, 0.0, 30.0))          # the next step leaves family-of-slot-5's block alone
    tw.anneal(2.0)
    tw.sweep(1)
    tw.anneal(2.5)
    tw.anneal(3.0)
    rec, blk = tw.records_array(), tw.block_records_array()
    b = int(AB.block_of(tw.fam[:1], B, tw.chunk)[0])
    assert blk[2, 0, b] == M and blk[3, 0, b] == M
    value, se, rep = jackknife.anneal_log_z(rec, blk, M)
    v0, se0, rep0 = AB.brute_force_log_z(tw.weights, M, B)
    assert same(rep, rep0) and same(se, se0) and np.all(np.isfinite(value))
    assert np.isfinite(rep[0]).all() and np.isfinite(se[0]) and np.isnan(rep[2:, b]).all() and np.isnan(se[2:]).all()


def test_a_step_that_does_not_resample_counts_and_sums_nothing(oracle):
    M, B = 70, 4
    tw = make_twin(M, 1.0, np.full(M, np.nan), blocks=B)
    tw.anneal(2.0)
    blk = tw.block_records_array()
    assert tw.records[-1][0] == A.ALL_NAN and blk[0, 0].tolist() == [18, 18, 18, 16] and blk[0, 1].tolist() == [0, 0, 0, 0]
    value, se, rep = jackknife.anneal_log_z(tw.records_array(), blk, M)
    assert np.isnan(value).all() and np.isnan(rep).all() and np.isnan(se).all()


def test_the_jackknife_refuses_logs_that_do_not_belong_together(oracle):
    M, B = 64, 4
    tw = make_twin(M, 0.5, 0.9 * np.sin(np.arange(M)), blocks=B)
    tw.anneal(1.0); tw.anneal(1.5)
    rec, blk = tw.records_array(), tw.block_records_array()
    with pytest.raises(ValueError, match="anneal_log_z: 2 records beside block records of shape"):
        jackknife.anneal_log_z(rec, blk[:1], M)
    bad = blk.copy()
    bad[1, 1, 0] += np.uint64(1)
    with pytest.raises(ValueError, match="the block record of step 1 does not add up"):
        jackknife.anneal_log_z(rec, bad, M)
    value, se, _ = jackknife.anneal_log_z(rec[:0], blk[:0], M)
    assert value.shape == se.shape == (0,)
    # every family in one block (a chunk above M): one replicate, no variance
    tw = make_twin(M, 0.5, 0.9 * np.sin(np.arange(M)), blocks=B, chunk=1000)
    tw.anneal(1.0)
    assert np.isnan(jackknife.anneal_log_z(tw.records_array(), tw.block_records_array(), M)[1]).all()


# ---- calibration: the error bar against the spread over seeds ------------------------------------------------------------------------
CAL_M, CAL_B, CAL_SWEEPS, CAL_SEEDS = 4096, 16, 5, 64
CAL_BETAS = [4.0 ** (i / 6.0) for i in range(7)]               # 1 -> 4 in six geometric steps
CAL_EXACT = 0.5 * math.log(CAL_BETAS[0] / CAL_BETAS[-1])       # e = x^2: log(Z(4) / Z(1)) = log(1 / 4) / 2


def calibration_interval(n_seeds, noise=0.025, level=1e-3):
    """The interval for rms(se) / std(log Z over n_seeds seeds) of a calibrated error bar: the sample standard deviation of n_seeds
    normal values lies within sqrt(chi2_(n-1) quantiles / (n - 1)) of the true one at the given two-sided level, and the rms of the
    jackknife se carries about ``noise`` of its own (the mean of n_seeds values of se^2, each with a relative spread of
    sqrt(2 / (B - 1)), halved by the root: sqrt(2 / 15 / 64) / 2 = 0.023 for B = 16)."""
    from scipy.stats import chi2
    k = n_seeds - 1
    q_lo, q_hi = chi2.ppf(level / 2, k), chi2.ppf(1 - level / 2, k)
    return (1 - noise) / math.sqrt(q_hi / k), (1 + noise) / math.sqrt(q_lo / k)


CAL_HIST = dict(lo=0.0, hi=10.0, n_bins=500)                   # e = x^2 at beta >= 1: P(e >= 10) = erfc(sqrt(10)) = 8e-6


def reweighted_mean_energy(counts, betas, beta):
    """(<e>(beta), se) by WHAM over all temperatures and the delete-one-block jackknife of the whole of it: counts[S, B, n_bins + 3]."""
    n = CAL_HIST["n_bins"]
    energies = reweighting.bin_centres(CAL_HIST["lo"], CAL_HIST["hi"], n)
    start = {}

    def fn(c):
        log_g, f, _ = reweighting.wham(c, betas, energies, f0=start.get("f"))
        start.setdefault("f", f)
        return reweighting.reweight(log_g, energies, beta)[1]

    theta, se = jackknife.jackknife_counts(np.ascontiguousarray(counts.transpose(1, 0, 2)[:, :, :n]), fn)
    return float(theta), float(se)


@pytest.fixture(scope="module")
def calibration(oracle):
    out = []
    for seed in range(1, CAL_SEEDS + 1):
        rng = np.random.default_rng(seed)
        x = rng.normal(0.0, math.sqrt(1.0 / (2.0 * CAL_BETAS[0])), CAL_M)        # equilibrium at the first beta
        tw = make_twin(CAL_M, CAL_BETAS[0], x, blocks=CAL_B, seed=seed)
        hist = [tw.histogram_by_block(**CAL_HIST)]             # the histogram of every temperature, per block of families
        for b in CAL_BETAS[1:]:
            tw.anneal(b)
            tw.sweep(CAL_SWEEPS)
            hist.append(tw.histogram_by_block(**CAL_HIST))
        value, se, _ = jackknife.anneal_log_z(tw.records_array(), tw.block_records_array(), CAL_M)
        e, e_se = reweighted_mean_energy(np.array(hist), np.array(CAL_BETAS), CAL_BETAS[-1])
        out.append((value[-1], se[-1], e, e_se))
    return np.array(out)


def test_the_error_bar_is_calibrated(calibration):
    """M = 4096, B = 16, e = x^2, beta 1 -> 4 in six geometric steps, 5 sweeps (sigma = 0.8) behind each, seeds 1 .. 64: the rms of
    the jackknife se over the seeds against the standard deviation of log Z over the same seeds, inside the chi^2_63 interval at the
    10^-3 level widened by the 2.5 % noise of the mean se^2 (calibration_interval: about [0.75, 1.43]), and no estimate further than
    5 se from the exact value log(1 / 4) / 2.  Measured: profiles/population_annealing_blocks.md."""
    lz, se = calibration[:, 0], calibration[:, 1]
    ratio = math.sqrt((se ** 2).mean()) / lz.std(ddof=1)
    worst = np.abs((lz - CAL_EXACT) / se).max()
    # tests/test_gpu_anneal_blocks.py scales this spread to its population (CAL_STD there): the two figures may not drift apart
    assert abs(lz.std(ddof=1) / 0.0060798 - 1.0) < 0.01
    lo, hi = calibration_interval(CAL_SEEDS)
    print(f"rms se {math.sqrt((se ** 2).mean())!r}, std over seeds {lz.std(ddof=1)!r}, ratio {ratio!r} in [{lo!r}, {hi!r}], "
          f"mean log Z {lz.mean()!r} (exact {CAL_EXACT!r}), largest |error / se| {worst!r}")
    assert 0.7 < lo < 0.8 and 1.35 < hi < 1.45
    assert lo <= ratio <= hi
    assert worst <= 5.0


def test_the_error_bar_of_the_reweighted_energy_is_calibrated(calibration):
    """The same 64 runs with the energy histogram of every temperature kept per block of families (500 bins of [0, 10)): <e> at the
    schedule's own last beta = 4 by WHAM over all seven temperatures, its se by the jackknife that deletes a block at EVERY temperature
    at once, against the spread of <e> over the seeds -- the same chi^2_63 gate.  (The value itself carries the bias of the bin
    centres, the same in every seed: it is printed, the gate is on the spread.)"""
    e, se = calibration[:, 2], calibration[:, 3]
    ratio = math.sqrt((se ** 2).mean()) / e.std(ddof=1)
    lo, hi = calibration_interval(CAL_SEEDS)
    print(f"<e>(4): mean {e.mean()!r} (exact {0.5 / CAL_BETAS[-1]!r}), rms se {math.sqrt((se ** 2).mean())!r}, std over seeds {e.std(ddof=1)!r}, "
          f"ratio {ratio!r} in [{lo!r}, {hi!r}]")
    assert np.all(np.isfinite(se)) and lo <= ratio <= hi


def test_the_histogram_per_block_adds_up_to_the_plain_one(oracle):
    M = 301
    x = 1.6 * np.sin(0.731 * np.arange(M) + 0.2)
    for B, chunk, dtype in ((2, 0, "f64"), (5, 7, "f32"), (64, 1, "f64")):
        xs = x.astype(np.float32).astype(np.float64) if dtype == "f32" else x
        tw = make_twin(M, 0.5, xs, blocks=B, chunk=chunk, potential="double_well", dtype=dtype)
        tw.sweep(1); tw.anneal(0.9); tw.sweep(1)
        for lo, hi, n in ((0.0, 3.0, 7), (0.2, 1.0, 40)):
            per_block = tw.histogram_by_block(lo, hi, n)
            assert per_block.shape == (B, n + 3) and per_block.dtype == np.uint64
            assert np.array_equal(per_block.sum(axis=0), E.snapshot("double_well", tw.x(), lo, hi, n, 1, dtype == "f32")[0])
            assert np.array_equal(per_block.sum(axis=1), tw.block_counts()) and per_block[:, n:].sum() > 0


# ---- the C ABI's argument checks (no device is touched) ----------------------------------------------------------------------------------
def test_new_entries_refuse_a_null_handle(amc):
    lib = amc.load()
    for name in ("amc_set_anneal_blocks", "amc_anneal_fetch_blocks", "amc_set_anneal_block_records", "amc_anneal_block_counts"):
        res, args = amc.SIGNATURES[name]
        vals = [None] + [0 if t in (C.c_int, C.c_int64, C.c_uint64) else None for t in args[1:]]
        assert getattr(lib, name)(*vals) == -1 and name.encode() in lib.amc_last_error()


# ---- the Python layer over the engine_factory seam ----------------------------------------------------------------------------------------
def build(path, steps, betas, *, every=2, M=64, callbacks=(), factory=AB.AnnealBlocksTwinEngine, **pa):
    chains = ma.ParticleChains.uniform(M, betas[0], potential="double_well")
    al = [dict(algorithm=ma.Metropolis, pool=POOL(0.5), seed=4, engine_factory=factory),
          dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, every), betas=betas[1:], **pa)]
    if callbacks:
        al.append(dict(algorithm=ma.StoreCallbacks, callbacks=tuple(callbacks), scheduler=ma.build_schedule(steps, 0, every)))
    return ma.Simulation(chains, al, steps, path=str(path))


def test_run_with_blocks_returns_value_and_error(oracle, tmp_path):
    betas = [0.5, 0.8, 1.2, 1.7, 2.5]
    sim = build(tmp_path, 8, betas, blocks=4, callbacks=(ma.callback_anneal_log_z, ma.callback_anneal_log_z_error))
    ma.run(sim)
    pa, eng = sim.algorithms[1], sim.algorithms[0].engine
    assert pa.families and pa.blocks == (4, 16)
    rec, blk = pa.records(), pa.block_records()
    assert blk.shape == (4, 2, 4) and np.all(blk[:, 0].sum(axis=1) == 64) and np.array_equal(blk[:, 1].sum(axis=1), rec[:, 4])
    assert np.array_equal(blk, eng.twin.block_records_array())
    value, se = pa.log_z(error=True)
    assert np.array_equal(value, pa.log_z()) and same(se, AB.brute_force_log_z(eng.twin.weights, 64, 4)[1]) and np.all(se > 0)
    r, rse = pa.log_z_ratios(error=True)
    assert np.array_equal(r, pa.log_z_ratios()) and rse[0] == se[0]
    assert float(open(tmp_path / "anneal_log_z_error.dat").read().splitlines()[-1].split()[-1]) == pytest.approx(se[-1])
    # the partition changes nothing else: the same schedule without it
    plain = build(tmp_path / "p", 8, betas, families=True)
    ma.run(plain)
    assert np.array_equal(plain.algorithms[1].records(), rec)
    assert np.array_equal(plain.algorithms[0].engine.download_state()[0].view(np.uint64), eng.download_state()[0].view(np.uint64))
    assert np.array_equal(plain.algorithms[0].engine.download_families(), eng.download_families())


def test_refusals_of_the_python_layer(oracle, tmp_path):
    betas = [0.5, 1.0, 2.0]
    with pytest.raises(ValueError, match="PopulationAnnealing: block_chunk = 4 without blocks"):
        build(tmp_path / "a", 4, betas, block_chunk=4)
    for bad in (1, 65, 2.5):
        with pytest.raises(ValueError, match=r"PopulationAnnealing: blocks = .* must be an integer in \[2, 64\]"):
            build(tmp_path / "b", 4, betas, blocks=bad)
    with pytest.raises(ValueError, match="PopulationAnnealing: block_chunk = 0 must be an integer >= 1"):
        build(tmp_path / "c", 4, betas, blocks=4, block_chunk=0)
    with pytest.raises(ValueError, match="make fewer chunks than blocks = 4"):
        build(tmp_path / "d", 4, betas, blocks=4, block_chunk=32)
    with pytest.raises(ValueError, match=r"this engine keeps no weight sums per block of families \(blocks needs amc_set_anneal_blocks\)"):
        build(tmp_path / "e", 4, betas, blocks=4, factory=A.AnnealTwinEngine)
    sim = build(tmp_path / "f", 4, betas, families=True)
    ma.run(sim)
    for call in (lambda: sim.algorithms[1].block_records(), lambda: sim.algorithms[1].log_z(error=True),
                 lambda: sim.algorithms[1].log_z_ratios(error=True)):
        with pytest.raises(ValueError, match="needs the partition: build the PopulationAnnealing with blocks=B"):
            call()


def test_checkpoint_carries_the_partition_and_the_block_records(oracle, tmp_path):
    betas = [0.5, 0.7, 1.0, 1.4, 2.0, 2.8, 4.0]
    whole = build(tmp_path / "w", 12, betas, blocks=8, block_chunk=3)
    ma.run(whole)
    first = build(tmp_path / "a", 6, betas, blocks=8, block_chunk=3)
    ma.run(first)
    fn = ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    d = np.load(fn)
    assert d["anneal_blocks"].tolist() == [8, 3] and d["anneal_block_records"].shape == (3, 2, 8)
    assert first.algorithms[1].block_records().shape == (3, 2, 8)          # the checkpoint left both logs where they were
    second = build(tmp_path / "b", 6, betas, blocks=8, block_chunk=3)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    assert np.array_equal(whole.algorithms[1].records(), second.algorithms[1].records())
    assert np.array_equal(whole.algorithms[1].block_records(), second.algorithms[1].block_records())
    a, b = whole.algorithms[1].log_z(error=True), second.algorithms[1].log_z(error=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    e1, e2 = whole.algorithms[0].engine, second.algorithms[0].engine
    assert np.array_equal(e1.download_state()[0].view(np.uint64), e2.download_state()[0].view(np.uint64))
    assert np.array_equal(e1.download_families(), e2.download_families())
    # another partition, or none in the checkpoint, is refused; a run without blocks writes the keys it always wrote
    other = build(tmp_path / "c", 6, betas, blocks=4)
    with pytest.raises(ValueError, match=r"checkpoint holds block records under the partition \(8, 3\)"):
        ma.restore(other.algorithms[0], str(tmp_path / "ck"))
    plain = build(tmp_path / "d", 6, betas, families=True)
    ma.run(plain)
    keys = set(np.load(ma.checkpoint(plain.algorithms[0], str(tmp_path / "ck2"))).keys())
    assert not any(k.startswith("anneal_block") for k in keys) and {"anneal_records", "families"} <= keys
    asks = build(tmp_path / "e", 6, betas, blocks=4)
    with pytest.raises(ValueError, match="checkpoint holds annealing records without block records"):
        ma.restore(asks.algorithms[0], str(tmp_path / "ck2"))


HIST = dict(lo=0.0, hi=12.0, n_bins=60)


def test_histograms_per_block_and_the_reweighted_curve_with_errors(oracle, tmp_path):
    betas = [0.5, 0.8, 1.2, 1.7, 2.5]
    sim = build(tmp_path, 8, betas, M=256, blocks=4, energy_histogram=HIST)
    ma.run(sim)
    pa, eng = sim.algorithms[1], sim.algorithms[0].engine
    b, counts = pa.histograms()
    bb, per_block = pa.histograms_blocks()
    assert np.array_equal(b, bb) and b.tolist() == betas and per_block.shape == (5, 4, 63) and per_block.dtype == np.uint64
    assert np.array_equal(per_block.sum(axis=1), counts) and np.all(counts.sum(axis=1) == 256)
    assert np.array_equal(per_block[-1], eng.twin.histogram_by_block(**HIST))
    grid = np.array([0.6, 1.0, 2.0])
    plain = pa.reweight(grid)
    value, se = pa.reweight(grid, error=True)
    assert len(value) == len(se) == 4 and all(np.allclose(v, p, rtol=1e-9, atol=1e-12) for v, p in zip(value, plain))
    assert all(s.shape == (3,) and np.all(np.isfinite(s)) and np.all(s > 0) for s in se)
    # the se against the replicates formed by hand: WHAM and the reweighting without block k at every temperature
    energies = reweighting.bin_centres(HIST["lo"], HIST["hi"], HIST["n_bins"])
    reps = np.array([reweighting.reweight(reweighting.wham((counts - per_block[:, k])[:, :60], b, energies)[0], energies, grid)[1] for k in range(4)])
    assert np.allclose(se[1], np.sqrt(3 / 4 * ((reps - reps.mean(axis=0)) ** 2).sum(axis=0)), rtol=1e-6)
    plain_run = build(tmp_path / "p", 8, betas, M=256, families=True, energy_histogram=HIST)
    ma.run(plain_run)
    assert np.array_equal(plain_run.algorithms[1].histograms()[1], counts)
    for call in (plain_run.algorithms[1].histograms_blocks, lambda: plain_run.algorithms[1].reweight(grid, error=True)):
        with pytest.raises(ValueError, match="needs the histograms per block"):
            call()


def test_checkpoint_carries_the_histograms_per_block(oracle, tmp_path):
    betas = [0.5, 0.7, 1.0, 1.4, 2.0, 2.8, 4.0]
    whole = build(tmp_path / "w", 12, betas, M=256, blocks=4, energy_histogram=HIST)
    ma.run(whole)
    first = build(tmp_path / "a", 6, betas, M=256, blocks=4, energy_histogram=HIST)
    ma.run(first)
    d = np.load(ma.checkpoint(first.algorithms[0], str(tmp_path / "ck")))
    assert d["anneal_hist_block_counts"].shape == (3, 4, 63) and np.array_equal(d["anneal_hist_block_counts"].sum(axis=1), d["anneal_hist_counts"])
    second = build(tmp_path / "b", 6, betas, M=256, blocks=4, energy_histogram=HIST)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = whole.algorithms[1].histograms_blocks(), second.algorithms[1].histograms_blocks()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].shape == (7, 4, 63)
    ra, rb = whole.algorithms[1].reweight([1.0, 3.0], error=True), second.algorithms[1].reweight([1.0, 3.0], error=True)
    assert all(np.array_equal(x, y) for x, y in zip(ra[0] + ra[1], rb[0] + rb[1]))
    # a checkpoint that holds block records is not restored into a run without blocks: they would be dropped
    plain = build(tmp_path / "c", 6, betas, M=256, families=True, energy_histogram=HIST)
    with pytest.raises(ValueError, match="asks for no blocks: they would be dropped"):
        ma.restore(plain.algorithms[0], str(tmp_path / "ck"))
