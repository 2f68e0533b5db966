"""Per-rung reproducible sums on the device (include/amc.h amc_reduce_rungs_exact) against their host twin
(tests/rung_sums_twin.py: oracle_lib.xsum_r over the strided slices), bit for bit on all 12 words of every record -- no tolerance
anywhere.  Shapes are the smallest at which the kernel takes another path: one ladder, ladders that straddle a wave (64) and a block
(256), odd R and R that divides neither 64 nor 256, R = 64, a grid that is walked more than once (tail loop) and more than four times
(the loop with four loads in flight).

No lane-cap case: a lane holds XS_LANE_CAP - 2 = 4094 summands per column and a launch has at least 65 536 lanes as soon as it makes
more than one trip (one block per CU, AMC_BLOCKS_PER_CU=1), so the cap is first reached at 2^28 chains -- 2 GiB of state, minutes of
host twin.  Beyond it the host splits the ladders over several launches of at most 4094 trips each (amc_exchange.hip); the kernel
itself never flushes mid-launch."""
import os

import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd.system import CustomPotential

import exchange_twin as X
import oracle_lib as O
import rung_sums_twin as RS

pytestmark = pytest.mark.gpu
POOLS = {1: ([0.5], [1.0]), 2: ([0.5, 0.25], [0.625, 0.375])}
CUSTOM = "x*x*x*x - 2.0*x*x + 0.25*x"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def start_state(R, M, offset=0, beta_kind="ladder", seed=11):
    """x and beta of the chains [offset, offset + M) as functions of the GLOBAL chain id (as in test_gpu_exchange.py)."""
    ids = np.arange(offset, offset + M)
    x = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)
    if beta_kind == "ladder":
        beta = (0.5 * 1.5 ** np.arange(R))[ids % R]
    else:
        beta = np.random.default_rng(seed).uniform(0.3, 6.0, size=offset + M)[offset:]
    return x, beta


def make_pair(gpu, R, L, *, potential="harmonic", K=1, counters=True, dtype="f64", param_dtype="f64", offset=0, n_global=None, seed=23):
    """(HipEngine, ExchangeTwin over the matching host simulation), both holding the same start state and a ladder of R rungs."""
    M = R * L
    sigma, weight = POOLS[K]
    x, beta = start_state(R, M, offset)
    eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=n_global or offset + M, potential=potential, beta=1.0,
                        sigma=sigma, weight=weight, seed=seed, per_chain_counters=counters, dtype=dtype, param_dtype=param_dtype)
    eng.upload_state(x, beta)
    eng.set_ladder(R)
    if param_dtype == "f32":
        import f32_param_twin as T
        sim = T.TwinSim(M, chain_offset=offset, potential=potential, beta=1.0, sigma=sigma, weight=weight, seed=seed)
        sim.beta[:] = beta.astype(np.float32)
    else:
        sim = O.OracleSim(M, chain_offset=offset, potential=potential, beta=1.0, sigma=sigma, weight=weight, seed=seed, dtype=dtype)
        sim.set_beta(beta)
    tw = X.ExchangeTwin(sim, beta, R, seed=seed, potential=potential, chain_offset=offset, f32=dtype == "f32")
    tw.state.put(x.astype(np.float32).astype(np.float64) if dtype == "f32" else x, tw.pot)
    return eng, tw


def plain_engine(gpu, R, L, *, potential="harmonic", dtype="f64", **kw):
    """A handle with a ladder of R rungs and nothing else: upload_state, set_ladder and reduce_rungs are all these tests need."""
    eng = gpu.HipEngine(n_chains=R * L, potential=potential, beta=1.0, sigma=[0.5], weight=[1.0], seed=5, dtype=dtype, **kw)
    return eng


def same_records(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        r, c = int(bad[0][0]), int(bad[0][1])
        raise AssertionError(f"{what}: records differ from the twin, first at rung {r} column {c}: {got[r, c].tolist()} != {want[r, c].tolist()}")


def check_against_downloaded_state(eng, R, what="", columns=7):
    x, e = eng.download_state()
    got = eng.reduce_rungs(columns)
    same_records(got, RS.records(x, e, R, columns), what)
    return got


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 1), (3, 1), (3, 22), (5, 103), (7, 37), (8, 33), (64, 1), (64, 5), (63, 9)]


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
@pytest.mark.parametrize("R,L", SHAPES)
def test_shapes_match_the_twin(gpu, R, L, potential):
    eng, tw = make_pair(gpu, R, L, potential=potential)
    for obj in (eng, tw):
        obj.sweep(2); obj.exchange(1); obj.sweep(1)
    xo, eo = tw.state.sim.state()                        # e and x of the oracle simulation
    got = eng.reduce_rungs()
    assert got.shape == (R, 3, 12)
    same_records(got, RS.records(xo, eo, R), f"R={R} L={L} {potential}")
    eng.close()


@pytest.mark.parametrize("dtype,param_dtype", [("f32", "f64"), ("f32", "f32")])
@pytest.mark.parametrize("R,L,potential", [(3, 22, "double_well"), (5, 103, "harmonic"), (64, 5, "double_well")])
def test_float32_state(gpu, R, L, potential, dtype, param_dtype):
    eng, tw = make_pair(gpu, R, L, potential=potential, dtype=dtype, param_dtype=param_dtype)
    for obj in (eng, tw):
        obj.sweep(2); obj.exchange(1); obj.sweep(1)
    xo, eo = tw.state.sim.state()
    xo, eo = np.asarray(xo, dtype=np.float64), np.asarray(eo, dtype=np.float64)
    same_records(eng.reduce_rungs(), RS.records(xo, eo, R), f"R={R} L={L} {potential} {dtype}/{param_dtype}")
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("R,L", [(5, 103), (63, 9)])
def test_custom_potential(gpu, R, L, dtype):
    eng, tw = make_pair(gpu, R, L, potential=CustomPotential(CUSTOM), dtype=dtype)
    eng.sweep(2); eng.exchange(1); eng.sweep(1)
    check_against_downloaded_state(eng, R, f"custom {dtype} R={R}")          # (download_state's bits are pinned by test_gpu_exchange.py)
    eng.close()


# ---- 2. levels are per rung -----------------------------------------------------------------------------------------------------------
def _level_state(R, L):
    assert R == 4
    l = np.arange(L)
    sign = np.where(l % 3 == 0, -1.0, 1.0)
    x = np.zeros((L, R))
    x[:, 0] = sign * 1e-30 * (1.0 + 0.37 * np.sin(l))
    x[:, 1] = sign * (0.5 + np.abs(np.sin(0.9 * l)))
    x[:, 2] = sign * 1e40 * (1.0 + 0.37 * np.cos(l))                     # harmonic: e ~ 1e80
    x[:, 3] = sign * 10.0 ** (-10.0 + 35.0 * l / (L - 1))                # grows with the ladder index: tops rise after deposits
    return x


def test_levels_are_per_rung(gpu):
    """What a shared wave-uniform top fails: the four rungs of a wave's lanes live 70 decades apart, and each keeps the quantum its
    own largest summand fixes.  Then values AT the level boundaries, 2^(50 k + 49) and its predecessor, in one rung."""
    R, L = 4, 80
    beta = np.tile(0.5 * 1.5 ** np.arange(R), L)
    eng = plain_engine(gpu, R, L)
    x = _level_state(R, L)
    eng.upload_state(x.reshape(-1), beta)
    eng.set_ladder(R)
    got = check_against_downloaded_state(eng, R, "levels")
    tops = got[:, 1, 1]                                                  # word 1 of a record: its top level
    assert tops[0] < tops[1] < tops[2] and len(set(got[:, 0, 1])) > 2
    # the same rungs 0 and 1 beside other neighbours: their records do not move
    y = x.copy()
    y[:, 2] *= 1e100
    y[:, 3] = x[::-1, 3]
    eng.upload_state(y.reshape(-1), beta)
    again = check_against_downloaded_state(eng, R, "levels, other neighbours")
    assert np.array_equal(bits(again[:2]), bits(got[:2]))
    # level boundaries: k from -3 to 3, both signs, rising and falling along the ladder index
    edge = []
    for k in range(-3, 4):
        b = 2.0 ** (50 * k + 49)
        edge += [b, np.nextafter(b, 0.0), -b, -np.nextafter(b, 0.0)]
    edge = np.array(edge)
    z = x.copy()
    z[:, 1] = np.resize(edge, L)
    z[:, 3] = np.resize(edge[::-1], L)
    eng.upload_state(z.reshape(-1), beta)
    check_against_downloaded_state(eng, R, "level boundaries")
    eng.close()


# ---- 3. flags stay with their rung ----------------------------------------------------------------------------------------------------
def test_flags_stay_with_their_rung(gpu):
    R, L = 5, 103
    x, beta = start_state(R, R * L)
    x = x.reshape(L, R)
    x[17, 1] = np.nan
    x[40, 2] = np.inf
    x[3, 3], x[99, 3] = -np.inf, np.inf
    eng = plain_engine(gpu, R, L, potential="double_well")
    eng.upload_state(x.reshape(-1), beta)
    eng.set_ladder(R)
    got = check_against_downloaded_state(eng, R, "flags")
    xs, es = eng.download_state()
    twin = RS.values(RS.records(xs, es, R))
    val = ma._capi.xsum_round(got.reshape(-1, 12)).reshape(R, 3)
    nan = np.isnan(twin)                                  # (the sign and payload of a NaN are no part of the definition)
    assert np.array_equal(np.isnan(val), nan) and np.array_equal(bits(val)[~nan], bits(twin)[~nan])
    assert np.isfinite(val[0]).all() and np.isfinite(val[4]).all()
    assert np.isnan(val[1]).all() and np.all(val[2] == np.inf)
    assert val[3, 0] == np.inf and np.isnan(val[3, 1]) and val[3, 2] == np.inf
    eng.close()


# ---- 4. grid stride -------------------------------------------------------------------------------------------------------------------
def _grown_state(R, L):
    """Magnitudes that rise, fall or wander with the ladder index, rung by rung: a lane that makes several trips raises its tops after
    deposits, and the lanes of one rung end the launch at different levels."""
    l = np.arange(L, dtype=np.float64)
    x = np.empty((L, R))
    for r in range(R):
        s = np.where((np.arange(L) + r) % 5 == 0, -1.0, 1.0)
        if r % 3 == 0:
            x[:, r] = s * 10.0 ** (-10.0 + 35.0 * l / (L - 1))
        elif r % 3 == 1:
            x[:, r] = s * 10.0 ** (25.0 - 35.0 * l / (L - 1))
        else:
            x[:, r] = s * 10.0 ** (20.0 * np.sin(0.001 * l + r))
    return x


@pytest.mark.parametrize("R,L", [(6, 30001), (3, 100003)])
def test_grid_stride(gpu, monkeypatch, R, L):
    """One block per CU: 6 x 30 001 chains walk the grid three times (the tail loop), 3 x 100 003 five times (four loads in flight, then
    the tail).  First the swept state, then one whose magnitudes move along the ladder index."""
    monkeypatch.setenv("AMC_BLOCKS_PER_CU", "1")
    x, beta = start_state(R, R * L)
    eng = plain_engine(gpu, R, L, potential="double_well")
    monkeypatch.delenv("AMC_BLOCKS_PER_CU")
    eng.upload_state(x, beta)
    eng.set_ladder(R)
    eng.sweep(1); eng.exchange(2)
    check_against_downloaded_state(eng, R, "grid stride")
    eng.upload_state(_grown_state(R, L).reshape(-1), beta)
    check_against_downloaded_state(eng, R, "grid stride, moving levels")
    eng.close()


# ---- 6. shard invariance --------------------------------------------------------------------------------------------------------------
def test_shard_invariance(gpu):
    R, L = 3, 342
    M = R * L
    seq = lambda o: (o.sweep(2), o.exchange(1), o.sweep(1))
    whole, _ = make_pair(gpu, R, L, potential="double_well", K=2)
    seq(whole)
    rec_w = check_against_downloaded_state(whole, R, "whole")
    for split in ([0, 402, M], [0, 258, 264, M]):
        parts = [make_pair(gpu, R, (b - a) // R, potential="double_well", K=2, offset=a, n_global=M)[0] for a, b in zip(split, split[1:])]
        merged = None
        for p in parts:
            seq(p)
            rec = p.reduce_rungs().reshape(-1, 12)
            merged = rec if merged is None else ma._capi.xsum_merge(merged, rec)
        assert np.array_equal(bits(merged), bits(rec_w.reshape(-1, 12))), split
        assert np.array_equal(bits(ma._capi.xsum_round(merged)), bits(ma._capi.xsum_round(rec_w.reshape(-1, 12))))
        for p in parts:
            p.close()
    whole.close()


# ---- 7. column mask -------------------------------------------------------------------------------------------------------------------
def test_column_mask(gpu):
    R, L = 7, 37
    eng, _ = make_pair(gpu, R, L, potential="double_well")
    eng.sweep(1)
    full = eng.reduce_rungs()
    for cols in (1, 2, 4, 5, 6):
        got = check_against_downloaded_state(eng, R, f"columns {cols}", cols)
        for c in range(3):
            if cols >> c & 1:
                assert np.array_equal(bits(got[:, c]), bits(full[:, c]))
            else:
                assert not got[:, c].any()                                  # all-zero records
    eng.close()


# ---- 8. the observed state, and what is left alone ------------------------------------------------------------------------------------
def test_observes_the_queued_steps_and_disturbs_nothing(gpu):
    R, L = 5, 103
    eng, tw = make_pair(gpu, R, L, potential="double_well", K=2)
    eng.sweep_exchange(3, 2); tw.sweep_exchange(3, 2)
    got = eng.reduce_rungs()                              # straight behind the queued rounds: no sync in between
    before = (eng.step, eng.estimator_step, eng.exchange_step, eng.exchange_counters(), eng.download_counters(), eng.counter_totals())
    xo, eo = tw.state.sim.state()
    same_records(got, RS.records(xo, eo, R), "after sweep_exchange(3, 2)")
    again = check_against_downloaded_state(eng, R, "second call")
    assert np.array_equal(bits(again), bits(got))
    after = (eng.step, eng.estimator_step, eng.exchange_step, eng.exchange_counters(), eng.download_counters(), eng.counter_totals())
    assert before[:3] == after[:3] == (6, 0, 3)
    for b, a in zip(before[3:], after[3:]):
        assert all(np.array_equal(u, v) for u, v in zip(b, a))
    red = eng.reduce()                                    # the reduction tickets are free, and the whole-ensemble sums still work
    eng.sweep(1); tw.sweep(1)
    x, e = eng.download_state()
    xo, eo = tw.state.sim.state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    ao, to = tw.state.sim.counters()
    acc, tot = eng.download_counters()
    assert np.array_equal(acc, ao) and np.array_equal(tot, to)
    eng.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was(gpu):
    R, L = 3, 22
    x, beta = start_state(R, R * L)
    eng = plain_engine(gpu, R, L)
    eng.upload_state(x, beta)
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*amc_reduce_rungs_exact.*no ladder"):
        eng.reduce_rungs()
    eng.set_ladder(R)
    for cols in (0, 8, -1, 15):
        with pytest.raises(gpu.AmcError, match=r"amc error -1.*amc_reduce_rungs_exact.*columns"):
            eng.reduce_rungs(cols)
    eng.sweep(1)
    check_against_downloaded_state(eng, R, "after the refusals")
    eng.set_ladder(0)
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*amc_reduce_rungs_exact"):
        eng.reduce_rungs()
    eng.close()


# ---- 10. through the host mirror ------------------------------------------------------------------------------------------------------
def _run(tmp, fuse, potential, dtype):
    steps, R, L = 40, 3, 343
    x = start_state(R, R * L)[0]
    if dtype == "f32":
        x = x.astype(np.float32).astype(np.float64)
    chains = ma.ParticleChains.ladder(L, [0.5, 1.0, 2.0], x=x, potential=potential, dtype=dtype)
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 0.6), ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.2], 0.4))
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=9),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 3)),
          dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_rung_energy, ma.callback_rung_moments),
               scheduler=ma.build_schedule(steps, 0, 10))]
    sim = ma.Simulation(chains, al, steps, path=str(tmp))
    ma.run(sim, fuse=fuse)
    files = {f: open(os.path.join(str(tmp), f)).read() for f in ("rung_energy.dat", "rung_moments.dat")}
    rows = sim.algorithms[2].rows
    xs, es = sim.algorithms[0].engine.download_state()
    return rows, files, RS.means(RS.records(xs, es, R), L)


@pytest.mark.parametrize("potential,dtype", [("double_well", "f64"), (CustomPotential(CUSTOM), "f32")])
def test_callbacks_through_the_host_mirror(gpu, tmp_path, potential, dtype):
    a = _run(tmp_path / "stepwise", False, potential, dtype)
    b = _run(tmp_path / "fused", True, potential, dtype)
    assert a[1] == b[1] and len(a[1]["rung_energy.dat"].splitlines()) == len(a[0][0]) >= 5
    for rows_a, rows_b in zip(a[0], b[0]):
        assert [t for t, _ in rows_a] == [t for t, _ in rows_b] and {10, 20, 30, 40} <= {t for t, _ in rows_a}
        assert all(np.array_equal(bits(u), bits(v)) for (_, u), (_, v) in zip(rows_a, rows_b))
    for rows, files, ref in (a, b):
        (t_e, energy), (t_m, moments) = rows[0][-1], rows[1][-1]
        assert t_e == t_m == 40 and energy.shape == (3,) and moments.shape == (2, 3)
        assert np.array_equal(bits(energy), bits(ref[:, 0].copy()))
        assert np.array_equal(bits(moments), bits(np.ascontiguousarray(ref[:, 1:].T)))
