"""The single-sweep kernel after its instruction diet: an accept filter without clamp and sign test, a host-supplied trip count,
a running per-lane pair id.  Everything here is bit for bit -- against the reference-ordered decision (AMC_EXACT_ACCEPT=1),
against the oracle, or against a second handle.

Sizes: AMC_BLOCKS_PER_CU_SINGLE=1 makes one round of the single-sweep grid G = (number of CUs) x 256 pairs, the smallest the
handle offers, so zero to three full trips cost a few hundred thousand chains at the most."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- filter soundness where the clamp and the sign test used to act ---------------------------------------------------------------
# sigma = 50, 1e3 at beta = 2: dlogp far below -17 on most steps (and +huge on the rest); sigma = 1e-9: |dlogp| tiny, both signs
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
@pytest.mark.parametrize("sigma", [50.0, 1e3, 1e-9])
def test_filter_agrees_with_the_exact_decision_outside_the_old_range(gpu, monkeypatch, potential, dtype, sigma):
    M = 4099
    kw = dict(n_chains=M, potential=potential, beta=2.0, sigma=[sigma], weight=[1.0], seed=23, dtype=dtype)
    a = gpu.HipEngine(**kw)
    monkeypatch.setenv("AMC_EXACT_ACCEPT", "1")
    b = gpu.HipEngine(**kw)
    monkeypatch.delenv("AMC_EXACT_ACCEPT")
    for e in (a, b):
        e.init_uniform(-2.0, 2.0)
        for _ in range(8):
            e.sweep(1)                                     # single-sweep launches
        e.sweep(192)                                       # and a fused one: 200 steps
    assert np.array_equal(bits(a.download_state()[0]), bits(b.download_state()[0]))
    acc_a, tot_a = a.counter_totals()
    acc_b, tot_b = b.counter_totals()
    assert int(acc_a[0]) == int(acc_b[0]) and int(tot_a[0]) == int(tot_b[0])
    assert np.array_equal(a.download_counters()[0], b.download_counters()[0])
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_filter_with_infinite_and_nan_beta(gpu, monkeypatch, dtype):
    """A per-chain beta array with an inf and a NaN entry: dlogp = -+Inf / NaN reach the filter as they are."""
    M = 4099
    rng = np.random.default_rng(3)
    beta = rng.uniform(0.5, 3.0, M)
    beta[7], beta[8], beta[1001], beta[4098] = np.inf, np.nan, np.inf, np.nan
    x0 = rng.uniform(-2, 2, M)
    kw = dict(n_chains=M, potential="double_well", beta=1.0, sigma=[0.4], weight=[1.0], seed=29, dtype=dtype)
    engines = []
    for exact in (None, "1"):
        if exact:
            monkeypatch.setenv("AMC_EXACT_ACCEPT", exact)
        e = gpu.HipEngine(**kw)
        if exact:
            monkeypatch.delenv("AMC_EXACT_ACCEPT")
        try:
            e.upload_state(x0, beta)
        except gpu.AmcError as err:
            e.close()
            pytest.skip(f"the handle refuses a beta array with inf / NaN entries: {err}")
        engines.append(e)
    for e in engines:
        for _ in range(8):
            e.sweep(1)
        e.sweep(192)
    a, b = engines
    assert np.array_equal(bits(a.download_state()[0]), bits(b.download_state()[0]))
    assert np.array_equal(a.download_counters()[0], b.download_counters()[0])
    a.close()
    b.close()


# ---- loop shapes: zero, one, two and three full trips, ragged and odd ends -------------------------------------------------------
def _round_pairs(gpu):
    """One block per CU: the CU count as the engine's own HIP runtime reports it (grid_for, amc_api.hip).  The shape test checks
    it against what the handle says about its grid (AMC_DEBUG_PLAN)."""
    import ctypes
    hip = ctypes.CDLL(gpu.runtime_info()["hip_runtime"])
    n = ctypes.c_int(0)
    HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63         # hip_runtime_api.h, hipDeviceAttribute_t
    rc = hip.hipDeviceGetAttribute(ctypes.byref(n), HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT, 0)
    assert rc == 0 and 0 < n.value <= 4096, (rc, n.value)
    return n.value * 256


@pytest.fixture(scope="module")
def small_grid(gpu):
    mp = pytest.MonkeyPatch()
    mp.setenv("AMC_BLOCKS_PER_CU_SINGLE", "1")
    mp.setenv("AMC_DEBUG_PLAN", "1")                       # the handle reports the grid of every sweep call on stderr
    yield _round_pairs(gpu)
    mp.undo()


# chain count, and the trips of block 0 (full ones before the last): what the shape is there to exercise
SHAPES = [("1", 1), ("2", 1), ("511", 1), ("2*256", 1), ("2*G-1", 1), ("2*G+3", 2), ("4*G+2*256+1", 3), ("6*G-1", 3)]


@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("shape,trips", SHAPES, ids=[s for s, _ in SHAPES])
def test_loop_shapes_against_the_oracle(gpu, oracle, small_grid, capfd, shape, trips, counters):
    M = int(eval(shape, {"G": small_grid}))
    kw = dict(potential="harmonic", beta=2.0, sigma=[0.35], weight=[1.0], seed=31)
    eng = gpu.HipEngine(n_chains=M, per_chain_counters=counters, **kw)
    sim = oracle.OracleSim(M, **kw)
    eng.init_uniform(-2.0, 2.0)
    sim.init_uniform(-2.0, 2.0)
    capfd.readouterr()
    for _ in range(3):
        eng.sweep(1)
    # the grid the handle chose: block 0 takes ceil(pairs / pairs per round) trips -- the coverage this shape is here for
    import re
    plans = re.findall(r"\[amc\] sweep: (\d+) pairs in a grid of (\d+) blocks, (\d+) pairs per round", capfd.readouterr().err)
    assert len(plans) == 3, plans
    for pairs, grid, per_round in plans:
        assert int(pairs) == (M + 1) // 2 and int(per_round) == int(grid) * 256
        assert -(-int(pairs) // int(per_round)) == trips, (shape, pairs, grid, per_round)
    sim.make_steps(3, threads=8)
    x, e = eng.download_state()
    xo, eo = sim.state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    acc, tot = eng.counter_totals()
    ao, to = sim.counters()
    assert int(acc[0]) == int(ao.sum()) and int(tot[0]) == int(to.sum())
    if counters:                                           # the step log, folded
        a, t = eng.download_counters()
        assert np.array_equal(a, ao) and np.array_equal(t, to)
    eng.close()


# ---- the running pair id across 2^32 ----------------------------------------------------------------------------------------------
def test_pair_id_carries_across_two_to_the_32_inside_a_wave(gpu, small_grid):
    """Pair id 2^32 in lane 20 of the first wave, and again one trip later: one handle against two handles split at that id."""
    G = small_grid
    M = 2 * (G + 300)
    off = 2 * ((1 << 32) - 20)                             # even; local pair 20 is pair 2^32
    kw = dict(potential="harmonic", beta=2.0, sigma=[0.35], weight=[1.0], seed=37, per_chain_counters=False,
              n_chains_global=off + M)
    rng = np.random.default_rng(5)
    x0 = rng.uniform(-2, 2, M)
    whole = gpu.HipEngine(n_chains=M, chain_offset=off, **kw)
    lo = gpu.HipEngine(n_chains=40, chain_offset=off, **kw)
    hi = gpu.HipEngine(n_chains=M - 40, chain_offset=off + 40, **kw)
    whole.upload_state(x0)
    lo.upload_state(x0[:40])
    hi.upload_state(x0[40:])
    for e in (whole, lo, hi):
        for _ in range(3):
            e.sweep(1)
    x = whole.download_state()[0]
    assert np.array_equal(bits(x[:40]), bits(lo.download_state()[0]))
    assert np.array_equal(bits(x[40:]), bits(hi.download_state()[0]))
    for e in (whole, lo, hi):
        e.close()
