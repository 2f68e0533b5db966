"""Single-sweep launches in slices (amc_sweep_launches with AMC_SWEEP_SLICES > 1): the ensemble cut into contiguous slices whose
launches run on streams of their own.  Only the schedule changes, so everything here is bit for bit: against the same engine with
whole launches (AMC_SWEEP_SLICES=1) and against the oracle -- positions, energies, the accepted and the total count.

The slices are forced through the knobs, with AMC_SWEEP_SLICE_MIN_CHAINS=0; AMC_DEBUG_PLAN shows which route a call took."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(potential="harmonic", beta=2.0, sigma=[0.35], weight=[1.0], seed=41, per_chain_counters=False)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make(gpu, slices, blocks_per_cu=None, **kw):
    """An engine whose handle found AMC_SWEEP_SLICES = slices (the knobs are read when the handle is created)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("AMC_SWEEP_SLICES", str(slices))
    mp.setenv("AMC_SWEEP_SLICE_MIN_CHAINS", "0")
    mp.setenv("AMC_DEBUG_PLAN", "1")
    if blocks_per_cu:
        mp.setenv("AMC_SWEEP_SLICE_BLOCKS_PER_CU", str(blocks_per_cu))
    try:
        return gpu.HipEngine(**{**KW, **kw})
    finally:
        mp.undo()


def slice_lines(err):
    return re.findall(r"\[amc\] sweep slice (\d+) of (\d+): pairs from (\d+), (\d+) chains in a grid of (\d+) blocks", err)


def expected_slices(M, S):
    """Slices that hold pairs: whole blocks of 256 pairs are dealt out (amc_slices.h)."""
    return min(S, -(-((M + 1) // 2) // 256))


def same_state(a, b):
    xa, ea = a.download_state()
    xb, eb = b.download_state()
    return np.array_equal(bits(xa), bits(xb)) and np.array_equal(bits(ea), bits(eb))


def same_totals(a, b):
    (aa, ta), (ab, tb) = a.counter_totals(), b.counter_totals()
    return int(aa[0]) == int(ab[0]) and int(ta[0]) == int(tb[0])


# ---- sizes, slice counts, call lengths ---------------------------------------------------------------------------------------------
SIZES = [1, 2, 511, 512, 513, 2 * 256 * 3 + 1, 2 * 256 * 2, 100_003]

_oracle_cache = {}


def oracle_after(oracle, M, n):
    """Positions, energies and accepted total of M chains after n steps from init_uniform(-2, 2): one simulation per size, walked
    through the call lengths once and kept."""
    if M not in _oracle_cache:
        sim = oracle.OracleSim(M, **{k: v for k, v in KW.items() if k != "per_chain_counters"})
        sim.init_uniform(-2.0, 2.0)
        done, out = 0, {}
        for steps in (1, 2, 7):
            sim.make_steps(steps - done, threads=8)
            done = steps
            x, e = sim.state()
            acc, tot = sim.counters()
            out[steps] = (x.copy(), e.copy(), int(acc.sum()), int(tot.sum()))
        _oracle_cache[M] = out
    return _oracle_cache[M][n]


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("M", SIZES)
def test_sliced_call_equals_whole_launches_and_the_oracle(gpu, oracle, capfd, M, S, n):
    sliced, whole = make(gpu, S, n_chains=M), make(gpu, 1, n_chains=M)
    for e in (sliced, whole):
        e.init_uniform(-2.0, 2.0)
    capfd.readouterr()
    sliced.sweep_launches(n)
    took = slice_lines(capfd.readouterr().err)
    whole.sweep_launches(n)
    assert not slice_lines(capfd.readouterr().err)
    # the route: a call of one launch and an ensemble of one block stay whole; otherwise every slice that holds pairs is there
    want = expected_slices(M, S) if n >= 2 else 1
    assert len(took) == (want if want > 1 else 0), took
    if took:
        assert sum(int(t[3]) for t in took) == M and [int(t[2]) % 256 for t in took] == [0] * len(took)
    assert sliced.step == whole.step == n
    assert same_state(sliced, whole) and same_totals(sliced, whole)
    xo, eo, acc_o, tot_o = oracle_after(oracle, M, n)
    x, e = sliced.download_state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    acc, tot = sliced.counter_totals()
    assert int(acc[0]) == acc_o and int(tot[0]) == tot_o
    sliced.close()
    whole.close()


@pytest.mark.parametrize("S", [2, 3])
def test_slices_of_several_trips(gpu, oracle, capfd, S):
    """One block per CU and slice, and more than one round of that grid in every slice: the slice's own full_rounds / tail_pairs."""
    probe = make(gpu, S, blocks_per_cu=1, n_chains=2 * 256 * 4096 * S)       # every slice: 4096 blocks, a grid of one per CU
    probe.init_uniform(-2.0, 2.0)
    capfd.readouterr()
    probe.sweep_launches(2)
    G = int(slice_lines(capfd.readouterr().err)[0][4]) * 256                 # pairs per round of a slice's grid
    probe.close()
    assert 0 < G <= 4096 * 256
    M = 2 * S * G + 2 * 256 * 3 + 1                                          # every slice: one full round and a ragged second trip
    sliced, whole = make(gpu, S, blocks_per_cu=1, n_chains=M), make(gpu, 1, n_chains=M)
    sim = oracle.OracleSim(M, **{k: v for k, v in KW.items() if k != "per_chain_counters"})
    for e in (sliced, whole, sim):
        e.init_uniform(-2.0, 2.0)
    capfd.readouterr()
    sliced.sweep_launches(3)
    took = slice_lines(capfd.readouterr().err)
    assert len(took) == S and all(int(t[4]) * 256 == G and (int(t[3]) + 1) // 2 > G for t in took), took
    whole.sweep_launches(3)
    sim.make_steps(3, threads=8)
    assert same_state(sliced, whole) and same_totals(sliced, whole)
    xo, eo = sim.state()
    x, e = sliced.download_state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    assert int(sliced.counter_totals()[0][0]) == int(sim.counters()[0].sum())
    sliced.close()
    whole.close()


# ---- per-chain beta, and a shard whose pair ids cross 2^32 --------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3])
def test_per_chain_beta(gpu, oracle, capfd, S):
    M = 2 * 256 * 3 + 1
    rng = np.random.default_rng(11)
    x0, beta = rng.uniform(-2, 2, M), rng.uniform(0.5, 3.0, M)
    sliced, whole = make(gpu, S, n_chains=M), make(gpu, 1, n_chains=M)
    sim = oracle.OracleSim(M, **{k: v for k, v in KW.items() if k != "per_chain_counters"})
    for e in (sliced, whole):
        e.upload_state(x0, beta)
    sim.set_x(x0)
    sim.set_beta(beta)
    capfd.readouterr()
    sliced.sweep_launches(7)
    assert len(slice_lines(capfd.readouterr().err)) == S
    whole.sweep_launches(7)
    sim.make_steps(7, threads=8)
    assert same_state(sliced, whole) and same_totals(sliced, whole)
    xo, eo = sim.state()
    x, e = sliced.download_state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    assert int(sliced.counter_totals()[0][0]) == int(sim.counters()[0].sum())
    sliced.close()
    whole.close()


@pytest.mark.parametrize("S", [2, 3])
def test_pair_ids_cross_two_to_the_32_inside_a_later_slice(gpu, oracle, capfd, S):
    """Pair id 2^32 is local pair 600 of a shard of four blocks: in slice 1, which starts at pair 512 (the blocks are dealt 2 + 2 or
    2 + 1 + 1) -- the carry into the high word happens inside a slice that does not start at the shard's first pair."""
    M = 2 * 256 * 3 + 1
    off = 2 * ((1 << 32) - 600)
    kw = dict(n_chains=M, chain_offset=off, n_chains_global=off + M)
    rng = np.random.default_rng(13)
    x0 = rng.uniform(-2, 2, M)
    sliced, whole = make(gpu, S, **kw), make(gpu, 1, **kw)
    sim = oracle.OracleSim(M, chain_offset=off, **{k: v for k, v in KW.items() if k != "per_chain_counters"})
    for e in (sliced, whole):
        e.upload_state(x0)
    sim.set_x(x0)
    capfd.readouterr()
    sliced.sweep_launches(7)
    took = slice_lines(capfd.readouterr().err)
    assert len(took) == S and any(0 < int(t[2]) <= 600 < int(t[2]) + (int(t[3]) + 1) // 2 for t in took), took
    whole.sweep_launches(7)
    sim.make_steps(7, threads=8)
    assert same_state(sliced, whole) and same_totals(sliced, whole)
    xo, eo = sim.state()
    x, e = sliced.download_state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    assert int(sliced.counter_totals()[0][0]) == int(sim.counters()[0].sum())
    sliced.close()
    whole.close()


# ---- what follows a sliced call on the handle's stream sees every slice finished ---------------------------------------------------
@pytest.mark.parametrize("S", [2, 3])
def test_mixed_sequence_in_one_engine(gpu, oracle, S):
    """sweep_launches(7); a sweep that forms the callback sums (it reads the accepted slots as they are when it starts: the join
    must precede it); sweep_launches(3); download; totals."""
    M = 100_003
    sliced, whole = make(gpu, S, n_chains=M), make(gpu, 1, n_chains=M)
    sim = oracle.OracleSim(M, **{k: v for k, v in KW.items() if k != "per_chain_counters"})
    rows = []
    for e in (sliced, whole):
        e.init_uniform(-2.0, 2.0)
        e.sweep_launches(7)
        e.sweep_reduce_begin(1)
        rows.append(e.reduce_end())
        e.sweep_launches(3)
    sim.init_uniform(-2.0, 2.0)
    sim.make_steps(8, threads=8)
    acc8 = int(sim.counters()[0].sum())
    sim.make_steps(3, threads=8)
    assert np.array_equal(bits(rows[0]), bits(rows[1]))          # sum e, sum x, sum x^2, count, accepted total / steps
    assert rows[0][-1] * 8 == acc8                               # the accepted total of 8 steps, over the steps (exact: a power of two)
    assert same_state(sliced, whole) and same_totals(sliced, whole)
    xo, eo = sim.state()
    x, e = sliced.download_state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    acc, tot = sliced.counter_totals()
    assert int(acc[0]) == int(sim.counters()[0].sum()) and int(tot[0]) == 11 * M
    sliced.close()
    whole.close()


def test_two_sliced_engines_interleaved(gpu):
    M = 100_003
    pairs = []
    for seed, S in ((51, 2), (52, 3)):
        pairs.append((make(gpu, S, n_chains=M, seed=seed), make(gpu, 1, n_chains=M, seed=seed)))
    for a, b in pairs:
        a.init_uniform(-2.0, 2.0)
        b.init_uniform(-2.0, 2.0)
    for n in (2, 7, 3):                                          # the sliced engines' calls interleaved, nothing waited for in between
        for a, _ in pairs:
            a.sweep_launches(n)
    for n in (2, 7, 3):
        for _, b in pairs:
            b.sweep_launches(n)
    for a, b in pairs:
        assert same_state(a, b) and same_totals(a, b)
        a.close()
        b.close()


def test_timing_brackets_the_join(gpu, capfd):
    """timing_begin / timing_end around a sliced call: no shorter than the call's slice-0 launches on their own (an engine that
    holds slice 0's chains alone, in the same grid) -- the end event lies behind the joins."""
    M, S, n = 3_000_007, 3, 20
    sliced = make(gpu, S, blocks_per_cu=4, n_chains=M)
    sliced.init_uniform(-2.0, 2.0)
    capfd.readouterr()
    sliced.sweep_launches(n)                                     # warm-up; and the plan
    took = slice_lines(capfd.readouterr().err)
    assert len(took) == S
    m0, grid0 = int(took[0][3]), int(took[0][4])
    mp = pytest.MonkeyPatch()
    mp.setenv("AMC_BLOCKS_PER_CU_SINGLE", "4")                   # the slices' blocks per CU
    alone = make(gpu, 1, n_chains=m0)
    mp.undo()
    alone.init_uniform(-2.0, 2.0)
    alone.sweep_launches(n)
    capfd.readouterr()
    times = {}
    for name, e in (("sliced", sliced), ("alone", alone)):
        e.sync()
        e.timing_begin()
        e.sweep_launches(n)
        times[name] = e.timing_end()
    plans = re.findall(r"\[amc\] sweep: (\d+) pairs in a grid of (\d+) blocks", capfd.readouterr().err)
    assert plans and all(int(g) == grid0 for _, g in plans), (plans, grid0)
    print(f"sliced call {times['sliced']:.4f} ms, slice 0 alone {times['alone']:.4f} ms")
    assert times["sliced"] >= times["alone"] > 0.0, times
    sliced.close()
    alone.close()
