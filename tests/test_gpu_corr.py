"""Time correlation on the device (include/amc.h amc_corr_mark .. amc_corr_clear) against its host twin
(tests/corr_twin.py: oracle_lib.xsum_r over the strided slices, xsum_merge over shards), bit for bit on all 12 words of every record --
no tolerance anywhere.  The twin is applied to download_state() taken right after the mark and right after each sample;
download_state's bits are pinned by the parity and exchange tests.  Shapes are the smallest at which the kernel takes another path:
one chain, a wave and its neighbours, more than one block, a grid that is walked more than once (tail loop) and more than four times
(four loads in flight); with a ladder R = 2 with one ladder, odd R straddling a wave and a block, R = 64.  No lane-cap case, for the
reason test_gpu_rung_sums.py gives: the cap is first reached at 2^28 chains."""
import ctypes as C

import numpy as np
import pytest

from montecarlo_amd.system import CustomPotential

import corr_twin as T

pytestmark = pytest.mark.gpu
POOLS = {1: ([0.5], [1.0]), 2: ([0.5, 0.25], [0.625, 0.375])}
CUSTOM = "x*x*x*x - 2.0*x*x + 0.25*x"
LADDER = lambda R: 0.5 * 1.5 ** np.arange(R)
ERR_BAD_ARG, ERR_STATE = -1, -5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def start_state(M, R=0, offset=0):
    ids = np.arange(offset, offset + M)
    x = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)
    return x, (LADDER(R)[ids % R] if R else None)


def make(gpu, M, R=0, *, potential="harmonic", K=1, dtype="f64", offset=0, n_global=None, seed=23, env=None, **kw):
    mp = pytest.MonkeyPatch()
    for k, v in (env or {}).items():
        mp.setenv(k, v)
    try:
        sigma, weight = POOLS[K]
        eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=n_global or offset + M, potential=potential, beta=1.0,
                            sigma=sigma, weight=weight, seed=seed, dtype=dtype, **kw)
    finally:
        mp.undo()
    x, beta = start_state(M, R, offset)
    eng.upload_state(x, beta)
    if R:
        eng.set_ladder(R)
    return eng


def observe(eng, kind):
    x, e = eng.download_state()
    return x.copy() if kind == "x" else e.copy()


def same_records(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        s, g, c = (int(v) for v in np.argwhere(bits(got) != bits(want))[0][:3])
        raise AssertionError(f"{what}: records differ from the twin, first at sample {s} group {g} column {c}: "
                             f"{got[s, g, c].tolist()} != {want[s, g, c].tolist()}")


def sequence(eng, kind, R, sweep=None):
    """[mark; 3 sweeps; sample; 1 exchange; sample; sample] and the observable downloaded behind the mark and each sample."""
    sweep = sweep or eng.sweep
    eng.corr_mark(kind)
    series = [observe(eng, kind)]
    sweep(3)
    eng.corr_sample()
    series.append(observe(eng, kind))
    if R:
        eng.exchange(1)
    eng.corr_sample()
    series.append(observe(eng, kind))
    eng.corr_sample()
    series.append(observe(eng, kind))
    return series


def check_sequence(eng, kind, R, what, sweep=None):
    t0 = eng.step
    series = sequence(eng, kind, R, sweep)
    rec, steps, obs = eng.corr_fetch()
    G = max(R, 1)
    assert rec.shape == (4, G, 3, 12) and obs == T.OBSERVABLES[kind]
    assert steps.tolist() == [t0, eng.step, eng.step, eng.step] and eng.step > t0
    same_records(rec, T.records(series, G), what)
    # slot 0: O = a, so OO and AO hold the same summands
    assert np.array_equal(bits(rec[0, :, 1]), bits(rec[0, :, 2]))
    again = eng.corr_fetch()
    assert np.array_equal(bits(again[0]), bits(rec)) and np.array_equal(again[1], steps)          # fetch resets nothing
    return rec


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["energy", "x"])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 1025])
def test_shapes_without_a_ladder(gpu, M, kind):
    eng = make(gpu, M, potential="double_well")
    check_sequence(eng, kind, 0, f"M={M} {kind}")
    eng.close()


@pytest.mark.parametrize("kind", ["energy", "x"])
@pytest.mark.parametrize("R,L", [(2, 1), (3, 22), (5, 103), (64, 1), (64, 5)])
def test_shapes_with_a_ladder(gpu, R, L, kind):
    eng = make(gpu, R * L, R, potential="double_well")
    check_sequence(eng, kind, R, f"R={R} L={L} {kind}")
    eng.close()


@pytest.mark.parametrize("M,R", [(180007, 0), (300011, 0), (3 * 100003, 3)])
def test_grid_stride(gpu, M, R):
    """One block per CU (65 536 threads): 180 007 chains walk the grid three times (the tail loop), 300 011 five times (four loads in
    flight, then the tail)."""
    eng = make(gpu, M, R, env={"AMC_BLOCKS_PER_CU": "1"})
    check_sequence(eng, "energy", R, f"M={M} R={R}")
    eng.close()


# ---- 2. pools, state types, potentials, sliced launches -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["energy", "x"])
@pytest.mark.parametrize("K,dtype", [(2, "f64"), (1, "f32"), (2, "f32")])
def test_pools_and_float32_state(gpu, K, dtype, kind):
    for R, L in ((0, 1025), (5, 103)):
        eng = make(gpu, L * max(R, 1), R, K=K, dtype=dtype, potential="double_well")
        check_sequence(eng, kind, R, f"K={K} {dtype} R={R} {kind}")
        eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_custom_potential(gpu, dtype):
    for R, L in ((0, 257), (5, 103)):
        eng = make(gpu, L * max(R, 1), R, potential=CustomPotential(CUSTOM), dtype=dtype)
        check_sequence(eng, "energy", R, f"custom {dtype} R={R}")
        eng.close()


def test_sliced_sweep_launches(gpu):
    """A sample runs behind the join of the slices' streams: the records of a handle whose single-sweep launches are forced into
    slices equal those of the unsliced handle, and the twin's."""
    M, recs = 4099, []
    for slices in ("1", "3"):
        eng = make(gpu, M, per_chain_counters=False, env={"AMC_SWEEP_SLICES": slices, "AMC_SWEEP_SLICE_MIN_CHAINS": "0"})
        recs.append(check_sequence(eng, "energy", 0, f"slices={slices}", sweep=eng.sweep_launches))
        # ... and with nothing between the calls that would make the host wait
        eng.corr_mark("x"); eng.sweep_launches(2); eng.corr_sample(); eng.sweep_launches(1); eng.corr_sample()
        recs.append(eng.corr_fetch()[0])
        eng.close()
    assert np.array_equal(bits(recs[0]), bits(recs[2])) and np.array_equal(bits(recs[1]), bits(recs[3]))


# ---- 3. flags and levels --------------------------------------------------------------------------------------------------------------
def test_flags_touch_their_own_records_only(gpu):
    R, L = 4, 40
    x, beta = start_state(R * L, R)
    eng = gpu.HipEngine(n_chains=R * L, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=5)
    a = x.copy().reshape(L, R)
    a[7, 3] = np.nan                                    # an origin value that is NaN where the later value is finite
    eng.upload_state(a.reshape(-1), beta)
    eng.set_ladder(R)
    eng.corr_mark("energy")
    series = [observe(eng, "energy")]
    origin = eng.corr_origin()
    assert np.array_equal(bits(origin), bits(series[0]))
    y = x.copy().reshape(L, R)
    y[3, 0] = np.nan                                    # group 0: a NaN energy
    y[5, 1] = 1e200                                     # group 1: harmonic e = x^2 = +Inf
    y[:, 2] *= 1e20                                     # group 2: large, finite -- another level, no flag
    # (the positions change under the mark through the checkpoint route: an upload would clear it)
    rec0, steps0, _ = eng.corr_fetch()
    eng.upload_state(y.reshape(-1), beta)
    eng.set_corr("energy", origin, rec0, steps0)
    eng.corr_sample()
    series.append(observe(eng, "energy"))
    rec = eng.corr_fetch()[0]
    same_records(rec, T.records(series, R), "flags")
    val = T.values(rec)
    assert np.all(np.isnan(val[1, 0])) and np.all(np.isinf(val[1, 1]) | np.isnan(val[1, 1])) and np.all(np.isfinite(val[1, 2]))
    assert np.isnan(val[1, 3, 2]) and np.all(np.isfinite(val[1, 3, :2]))            # the NaN origin value: AO alone
    assert np.isnan(val[0, 3]).all() and np.all(np.isfinite(val[0, :3]))             # slot 0 of group 3 holds the NaN itself
    assert rec[1, 2, 0, 1] > rec[0, 2, 0, 1]             # word 1 of a record: its level, that of its own group, column and slot
    eng.close()


@pytest.mark.parametrize("kind", ["x", "energy"])
def test_levels_differ_among_the_lanes_of_one_slot(gpu, kind):
    """Every branch of the block end in ONE slot of one block.  R = 3, L = 64: 192 lanes of one block with one chain each (the 64
    lanes behind them have none), and the ladders of rung 1 hold |x| near 1, 2^-20, 2^-40, 2^-90 in turn, so neighbouring lanes of
    that rung sit 0, 1 and >= 2 levels of 50 bits below the slot's top: in O = x at the levels 0, -1, -1, -2, in O = e = x^2 at
    0, -1, -2, -4.  The mark, then a sample whose values are the neighbouring ladder's (a O mixes the magnitudes)."""
    R, L = 3, 64
    x, beta = start_state(R * L, R)
    l = np.arange(L)
    a = x.copy().reshape(L, R)
    a[:, 1] = np.where(l % 3 == 0, -1.0, 1.0) * (1.0 + 0.37 * np.sin(l)) * np.array([1.0, 2.0 ** -20, 2.0 ** -40, 2.0 ** -90])[l % 4]
    eng = gpu.HipEngine(n_chains=R * L, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=5)
    eng.upload_state(a.reshape(-1), beta)
    eng.set_ladder(R)
    eng.corr_mark(kind)
    series = [observe(eng, kind)]
    rec0, steps0, _ = eng.corr_fetch()
    same_records(rec0, T.records(series, R), f"levels in one slot, the mark, {kind}")
    origin = eng.corr_origin()
    eng.upload_state(np.roll(a, 1, axis=0).reshape(-1), beta)         # (through the checkpoint route: an upload clears the mark)
    eng.set_corr(kind, origin, rec0, steps0)
    eng.corr_sample()
    series.append(observe(eng, kind))
    same_records(eng.corr_fetch()[0], T.records(series, R), f"levels in one slot, a sample, {kind}")
    eng.close()


# ---- 4. shards ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 6])
def test_shard_invariance(gpu, R):
    G = max(R, 1)
    M = 660
    whole = make(gpu, M, R, potential="double_well", K=2)
    rec_w = check_sequence(whole, "energy", R, "whole")
    whole.close()
    for split in ([0, 402, M], [0, 258, 264, M], [0, 6, M]):           # the last: "1 | 3" -- one ladder beside the rest
        merged = None
        for a, b in zip(split, split[1:]):
            part = make(gpu, b - a, R, potential="double_well", K=2, offset=a, n_global=M)
            sequence(part, "energy", R)
            rec = part.corr_fetch()[0].reshape(-1, 12)
            merged = rec if merged is None else gpu.xsum_merge(merged, rec)
            part.close()
        assert np.array_equal(bits(merged), bits(rec_w.reshape(-1, 12))), (R, split)
    assert rec_w.shape[1] == G


# ---- 5. what the entries leave alone --------------------------------------------------------------------------------------------------
def test_corr_calls_leave_everything_else_alone(gpu):
    R, L = 5, 103

    def run(with_corr):
        eng = make(gpu, R * L, R, potential="double_well", K=2)
        eng.set_tracking(True)
        eng.sweep(2); eng.exchange(1)
        eng.bridge_accumulate(3)
        if with_corr:
            eng.corr_mark("energy")
        eng.reduce_begin()                                # a reduction in flight across the samples
        eng.sweep(2)
        if with_corr:
            eng.corr_sample()
        eng.exchange(2)
        if with_corr:
            eng.corr_sample(); eng.corr_fetch(); eng.corr_origin(); eng.corr_clear(); eng.corr_mark("x"); eng.corr_sample()
        red = eng.reduce_end()
        eng.sweep(1)
        x, e = eng.download_state()
        out = [x, e, red, *eng.download_counters(), *eng.exchange_counters(), np.array([eng.step, eng.exchange_step, eng.estimator_step]),
               *eng.labels(), np.array(eng.tracking_counters()), eng.bridge_fetch()[0], np.array([eng.bridge_fetch()[1]])]
        eng.close()
        return out

    plain, corr = run(False), run(True)
    for i, (p, c) in enumerate(zip(plain, corr)):
        p, c = np.asarray(p), np.asarray(c)
        assert p.dtype == c.dtype and p.shape == c.shape and p.tobytes() == c.tobytes(), i


# ---- 6. clearing and refusals ---------------------------------------------------------------------------------------------------------
def rc_sample(gpu, eng):
    return gpu.load().amc_corr_sample(eng._h)


def test_what_clears_the_mark_and_what_keeps_it(gpu):
    R, L = 3, 22
    x, beta = start_state(R * L, R)
    eng = make(gpu, R * L, R)
    lib = gpu.load()
    assert rc_sample(gpu, eng) == ERR_STATE and b"nothing is marked" in lib.amc_last_error()
    assert eng.corr_fetch()[2] == 0 and eng.corr_fetch()[0].shape[0] == 0
    eng.corr_mark("energy"); eng.sweep(1); eng.exchange(1); eng.reduce(); eng.reduce_rungs()
    eng.corr_sample()                                   # kept by sweeps, exchange steps and reductions
    assert eng.corr_fetch()[0].shape[0] == 2
    eng.upload_state(x, beta)
    assert rc_sample(gpu, eng) == ERR_STATE and eng.corr_fetch()[2] == 0
    eng.corr_mark("x")
    eng.set_ladder(R)
    assert rc_sample(gpu, eng) == ERR_STATE and eng.corr_fetch()[2] == 0
    eng.corr_mark("x")
    eng.init_uniform(-1.0, 1.0)
    assert rc_sample(gpu, eng) == ERR_STATE
    eng.corr_mark("x")
    eng.corr_clear()
    assert rc_sample(gpu, eng) == ERR_STATE
    eng.close()
    pa = make(gpu, 257)                                 # no ladder, one shared beta: the handle anneals
    pa.corr_mark("energy")
    pa.anneal(1.5)
    assert rc_sample(gpu, pa) == ERR_STATE and pa.corr_fetch()[2] == 0
    pa.close()


def test_refusals_leave_the_fetch_unchanged(gpu):
    eng = make(gpu, 65)
    lib = gpu.load()
    eng.corr_mark("energy")
    for _ in range(255):
        eng.corr_sample()
    before = eng.corr_fetch()
    assert before[0].shape == (256, 1, 3, 12)
    assert rc_sample(gpu, eng) == ERR_STATE and b"slots" in lib.amc_last_error()       # the 257th sample, the mark's own included
    assert lib.amc_corr_mark(eng._h, 3) == ERR_BAD_ARG and lib.amc_corr_mark(eng._h, 0) == ERR_BAD_ARG
    rec = np.zeros((255, 1, 3, 12)); steps = np.zeros(255, dtype=np.uint64); n, obs = C.c_int(0), C.c_int(0)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    assert lib.amc_corr_fetch(eng._h, rec.ctypes.data_as(dp), steps.ctypes.data_as(up), 255, C.byref(n), C.byref(obs)) == ERR_BAD_ARG
    assert lib.amc_corr_fetch(eng._h, None, steps.ctypes.data_as(up), 255, C.byref(n), C.byref(obs)) == ERR_BAD_ARG
    assert lib.amc_corr_fetch(eng._h, rec.ctypes.data_as(dp), None, 255, C.byref(n), C.byref(obs)) == ERR_BAD_ARG
    assert lib.amc_corr_fetch(eng._h, rec.ctypes.data_as(dp), steps.ctypes.data_as(up), 255, None, C.byref(obs)) == ERR_BAD_ARG
    assert lib.amc_corr_download_origin(eng._h, None) == ERR_BAD_ARG
    assert lib.amc_set_corr(eng._h, 1, None, None, None, 1) == ERR_BAD_ARG
    for fn in (lib.amc_corr_sample, lib.amc_corr_clear):
        assert fn(None) == ERR_BAD_ARG
    assert lib.amc_corr_mark(None, 1) == ERR_BAD_ARG
    after = eng.corr_fetch()
    assert np.array_equal(bits(after[0]), bits(before[0])) and np.array_equal(after[1], before[1]) and after[2] == before[2] == 1
    eng.close()


# ---- 7. the checkpoint pair -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,L", [(0, 1025), (5, 103)])
def test_set_corr_round_trip(gpu, R, L):
    M = L * max(R, 1)
    eng = make(gpu, M, R, potential="double_well")
    eng.corr_mark("energy"); eng.sweep(2); eng.corr_sample()
    rec, steps, obs = eng.corr_fetch()
    origin, x, t = eng.corr_origin(), eng.download_state()[0], eng.step
    other = make(gpu, M, R, potential="double_well")
    other.upload_state(x, start_state(M, R)[1])
    other.step = t
    other.set_corr(obs, origin, rec, steps)
    for e in (eng, other):
        e.sweep(3); e.corr_sample()
    a, b = eng.corr_fetch(), other.corr_fetch()
    assert a[0].shape[0] == 3 and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # doctored records are refused, and the mark stays as it was
    lib = gpu.load()
    for word, value in ((0, 1.0), (1, 0.5), (2, 9.0), (5, 0.5), (7, 2.0 ** 53), (4, np.nan)):
        bad = rec.copy()
        bad[1, 0, 2, word] = value
        with pytest.raises(gpu.AmcError):
            other.set_corr(obs, origin, bad, steps)
    with pytest.raises(gpu.AmcError):
        other.set_corr(obs, origin, rec, steps[::-1].copy())                  # decreasing steps
    with pytest.raises(gpu.AmcError):
        other.set_corr(3, origin, rec, steps)
    assert lib.amc_set_corr(other._h, 1, origin.ctypes.data_as(C.POINTER(C.c_double)), rec.ctypes.data_as(C.POINTER(C.c_double)),
                            steps.ctypes.data_as(C.POINTER(C.c_uint64)), 0) == ERR_BAD_ARG
    assert lib.amc_set_corr(other._h, 1, origin.ctypes.data_as(C.POINTER(C.c_double)), rec.ctypes.data_as(C.POINTER(C.c_double)),
                            steps.ctypes.data_as(C.POINTER(C.c_uint64)), 257) == ERR_BAD_ARG
    c = other.corr_fetch()
    assert np.array_equal(bits(c[0]), bits(b[0])) and np.array_equal(c[1], b[1])
    eng.close(); other.close()
