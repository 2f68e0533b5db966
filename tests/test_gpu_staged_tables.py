"""The math tables are copied into a block's LDS from a staged image (AMC_MATH_TABLES_STAGED, amc_tables.h) instead of being rotated
and scaled by every block.  The image is compared with what the generator's tables give, exactly; every kernel form that stages the
tables is run once against the oracle (or the parity its own tests use), bit for bit, at the chain counts where block and slice
edges lie."""
import os
import re
import sys

import numpy as np
import pytest

from montecarlo_amd.system import CustomPotential

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(beta=2.0, sigma=[0.35], weight=[1.0], seed=43)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the image -------------------------------------------------------------------------------------------------------------------
def test_staged_image_is_the_generators_tables_rotated_and_scaled(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_math_tables as G
    finally:
        sys.path.pop(0)
    f = lambda vals: np.array([float.fromhex(v) for v in vals])
    invc, logc = G.log_tables()
    sn, cs = G.sincos_tables()
    want = np.concatenate([f(cs), f(G.exp2_table()), f(invc), -2.0 * f(logc), f(sn)])      # rotation by the cosine table; LOGC times -2
    got = gpu.selftest_staged_tables()
    assert want.shape == got.shape == (546,)
    assert np.array_equal(bits(got), bits(want))


# ---- the headline form: block edges, one pair more than a round of the grid ------------------------------------------------------
def against_the_oracle(gpu, oracle, potential, M, steps=3):
    eng = gpu.HipEngine(n_chains=M, potential=potential, per_chain_counters=False, **KW)
    sim = oracle.OracleSim(M, potential=potential, **KW)
    eng.init_uniform(-2.0, 2.0)
    sim.init_uniform(-2.0, 2.0)
    for _ in range(steps):
        eng.sweep(1)
    sim.make_steps(steps, threads=8)
    x, e = eng.download_state()
    xo, eo = sim.state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    acc, tot = eng.counter_totals()
    ao, to = sim.counters()
    assert int(acc[0]) == int(ao.sum()) and int(tot[0]) == int(to.sum())
    eng.close()


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
@pytest.mark.parametrize("M", [1, 2, 3, 511, 512, 513])
def test_block_edges_against_the_oracle(gpu, oracle, potential, M):
    against_the_oracle(gpu, oracle, potential, M)


@pytest.fixture(scope="module")
def default_grid(gpu):
    """Blocks of the single-sweep launch's default grid, as the handle reports them for an ensemble that fills it."""
    mp = pytest.MonkeyPatch()
    mp.setenv("AMC_DEBUG_PLAN", "1")
    try:
        probe = gpu.HipEngine(n_chains=2 * 256 * 8192, potential="harmonic", per_chain_counters=False, **KW)
    finally:
        mp.undo()
    probe.init_uniform(-2.0, 2.0)
    yield probe
    probe.close()


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
def test_one_chain_more_than_a_round_of_the_grid(gpu, oracle, capfd, default_grid, potential):
    capfd.readouterr()
    default_grid.sweep(1)
    default_grid.sync()
    plans = re.findall(r"\[amc\] sweep: (\d+) pairs in a grid of (\d+) blocks", capfd.readouterr().err)
    assert plans and 0 < int(plans[0][1]) < 8192, plans
    against_the_oracle(gpu, oracle, potential, int(plans[0][1]) * 512 + 1)


# ---- the sliced route -------------------------------------------------------------------------------------------------------------
def make_sliced(gpu, slices, **kw):
    mp = pytest.MonkeyPatch()
    mp.setenv("AMC_SWEEP_SLICES", str(slices))
    mp.setenv("AMC_SWEEP_SLICE_MIN_CHAINS", "0")
    mp.setenv("AMC_DEBUG_PLAN", "1")
    try:
        return gpu.HipEngine(per_chain_counters=False, **KW, **kw)
    finally:
        mp.undo()


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
def test_two_slices_equal_whole_launches(gpu, capfd, potential):
    M = 2 * 256 * 7 + 1                                       # odd; seven whole blocks of pairs and a lone chain
    sliced, whole = make_sliced(gpu, 2, n_chains=M, potential=potential), make_sliced(gpu, 1, n_chains=M, potential=potential)
    for e in (sliced, whole):
        e.init_uniform(-2.0, 2.0)
    capfd.readouterr()
    sliced.sweep_launches(5)
    took = re.findall(r"\[amc\] sweep slice (\d+) of (\d+)", capfd.readouterr().err)
    assert len(took) == 2, took
    whole.sweep_launches(5)
    assert not re.findall(r"\[amc\] sweep slice", capfd.readouterr().err)
    (xs, es), (xw, ew) = sliced.download_state(), whole.download_state()
    assert np.array_equal(bits(xs), bits(xw)) and np.array_equal(bits(es), bits(ew))
    for a, b in zip(sliced.counter_totals(), whole.counter_totals()):
        assert np.array_equal(a, b)
    sliced.close()
    whole.close()


# ---- the other kernels that stage the tables: 4096 chains, 3 steps ---------------------------------------------------------------
M_OTHER = 4096


def test_two_moves_with_the_step_log(gpu, oracle):
    kw = dict(potential="double_well", beta=2.0, sigma=[0.2, 0.9], weight=[0.6, 0.4], seed=44)
    eng, sim = gpu.HipEngine(n_chains=M_OTHER, **kw), oracle.OracleSim(M_OTHER, **kw)
    eng.init_uniform(-2.0, 2.0)
    sim.init_uniform(-2.0, 2.0)
    for _ in range(3):
        eng.sweep(1)
    sim.make_steps(3, threads=8)
    assert np.array_equal(bits(eng.download_state()[0]), bits(sim.state()[0]))
    acc, tot = eng.download_counters()
    ao, to = sim.counters()
    assert np.array_equal(acc, ao) and np.array_equal(tot, to)
    eng.close()


def test_callback_sums_formed_in_the_sweep(gpu, oracle):
    eng = gpu.HipEngine(n_chains=M_OTHER, potential="harmonic", per_chain_counters=False, **KW)
    sim = oracle.OracleSim(M_OTHER, potential="harmonic", **KW)
    eng.init_uniform(-2.0, 2.0)
    sim.init_uniform(-2.0, 2.0)
    for _ in range(3):
        eng.sweep_reduce_begin(1)                             # the REDUCE form of the single-sweep launch
        rec, steps = eng.reduce_end_exact()
        sim.make_steps(1, threads=8)
    assert steps == 3
    assert np.array_equal(rec[:4], sim.callback_records()[:4])                 # sum e, sum x, sum x^2, count: records, word for word
    assert eng.reduce_records_value(rec, steps)[4] == int(sim.counters()[0].sum()) / 3      # pool-wide accepted total / steps
    assert np.array_equal(bits(eng.download_state()[0]), bits(sim.state()[0]))
    eng.close()


def test_one_fused_pgmc_step(gpu, oracle):
    kw = dict(n_chains=M_OTHER, potential="harmonic", beta=2.0, sigma=[0.2, 0.1], weight=[0.6, 0.4], seed=45)
    eng, ref = gpu.HipEngine(**kw), oracle.OracleEngine(**kw)
    for e in (eng, ref):
        e.init_uniform(-2.0, 2.0)
        e.sweep(2)
        e.pgmc_steps(1, [1], 2, [1], [0.05], [0.0])           # the third step: sweep + estimator + learning step in one launch
    assert eng.get_parameters(1)[0] == ref.get_parameters(1)[0]
    assert np.array_equal(bits(eng.download_state()[0]), bits(ref.download_state()[0]))
    eng.close()
    ref.close()


def test_float32_state(gpu, oracle):
    kw = dict(potential="double_well", dtype="f32", **KW)
    eng = gpu.HipEngine(n_chains=M_OTHER, per_chain_counters=False, **kw)
    sim = oracle.OracleSim(M_OTHER, **kw)
    eng.init_uniform(-2.0, 2.0)
    sim.init_uniform(-2.0, 2.0)
    for _ in range(3):
        eng.sweep(1)
    sim.make_steps(3, threads=8)
    x, e = eng.download_state()
    xo, eo = sim.state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    assert int(eng.counter_totals()[0][0]) == int(sim.counters()[0].sum())
    eng.close()


def test_custom_potential_picks_up_the_staging_through_the_embedded_sources(gpu, oracle):
    """A kernel compiled at run time from the sources the library carries: exp of the potential reads the staged tables."""
    pot = CustomPotential("(1.0 - amc_exp(-(x - 0.5))) * (1.0 - amc_exp(-(x - 0.5)))")
    eng = gpu.HipEngine(n_chains=M_OTHER, potential=pot, per_chain_counters=False, **KW)
    sim = oracle.OracleSim(M_OTHER, potential=pot, **KW)
    eng.init_uniform(-2.0, 2.0)
    sim.init_uniform(-2.0, 2.0)
    for _ in range(3):
        eng.sweep(1)
    sim.make_steps(3, threads=8)
    x, e = eng.download_state()
    xo, eo = sim.state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    assert int(eng.counter_totals()[0][0]) == int(sim.counters()[0].sum())
    eng.close()
