"""Bridge sums on the device (DESIGN.md section 3.13 "Bridge sums"; include/amc.h amc_bridge_accumulate, amc_bridge_fetch,
amc_set_bridge) against their host twin (tests/bridge_twin.py: amo_potential, amo_exp, oracle_lib.xsum_r over the strided slices,
xsum_merge over snapshots and shards), bit for bit on all 12 words of every record -- no tolerance anywhere.  Shapes are the smallest at
which the kernel takes another path: one ladder, R = 2 (both rungs are end rungs), ladders that straddle a wave and a block, odd R and R
that divides neither 64 nor 256, R = 64, a grid that is walked more than once (tail loop) and more than four times (four loads in
flight).  No lane-cap case, for the reason test_gpu_rung_sums.py gives: the cap is first reached at 2^28 chains."""
import os

import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd.system import CustomPotential

import bridge_twin as B
import exchange_twin as X
import oracle_lib as O
from test_bridge_twin import BETAS, L as GAUSS_L, acceptance_estimate_and_error, gaussian_ensemble, numpy_summands

pytestmark = pytest.mark.gpu
POOLS = {1: ([0.5], [1.0]), 2: ([0.5, 0.25], [0.625, 0.375])}
CUSTOM = "x*x*x*x - 2.0*x*x + 0.25*x"
LADDER = lambda R: 0.5 * 1.5 ** np.arange(R)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def start_state(R, M, offset=0):
    """x and beta of the chains [offset, offset + M) as functions of the GLOBAL chain id (as in test_gpu_exchange.py)."""
    ids = np.arange(offset, offset + M)
    return 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids), LADDER(R)[ids % R]


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
    return gpu.HipEngine(n_chains=R * L, potential=potential, beta=1.0, sigma=[0.5], weight=[1.0], seed=5, dtype=dtype, **kw)


def same_records(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        r, c = int(bad[0][0]), int(bad[0][1])
        raise AssertionError(f"{what}: records differ from the twin, first at rung {r} column {c}: {got[r, c].tolist()} != {want[r, c].tolist()}")


def twin_records(tw, columns=B.ALL):
    """The twin's records of the state the ExchangeTwin's simulation holds now."""
    e = np.asarray(tw.state.sim.state()[1], dtype=np.float64)
    return B.records(e, tw.beta, tw.R, columns, tw.f32)


def device_twin_records(eng, beta, R, columns=B.ALL, f32=False):
    """The twin's records of the state the ENGINE holds now (download_state's bits are pinned by test_gpu_exchange.py)."""
    return B.records(eng.download_state()[1], beta, R, columns, f32)


def one_snapshot(eng, columns=B.ALL):
    eng.bridge_accumulate(columns)
    rec, n = eng.bridge_fetch(reset=True)
    assert n == 1
    return rec


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 1), (3, 1), (3, 22), (5, 103), (7, 37), (8, 33), (64, 1), (64, 5), (63, 9)]


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
@pytest.mark.parametrize("R,L", SHAPES)
def test_shapes_match_the_twin(gpu, R, L, potential):
    eng, tw = make_pair(gpu, R, L, potential=potential)
    for obj in (eng, tw):
        obj.sweep(2); obj.exchange(1); obj.sweep(1)
    got = one_snapshot(eng)
    assert got.shape == (R, 6, 12)
    same_records(got, twin_records(tw), f"R={R} L={L} {potential}")
    eng.close()


# ---- 2. Float32 state, script-defined potentials --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,param_dtype", [("f32", "f64"), ("f32", "f32")])
@pytest.mark.parametrize("R,L,potential", [(3, 22, "double_well"), (5, 103, "harmonic"), (64, 5, "double_well")])
def test_float32_state(gpu, R, L, potential, dtype, param_dtype):
    eng, tw = make_pair(gpu, R, L, potential=potential, dtype=dtype, param_dtype=param_dtype)
    for obj in (eng, tw):
        obj.sweep(2); obj.exchange(1); obj.sweep(1)
    same_records(one_snapshot(eng), twin_records(tw), f"R={R} L={L} {potential} {dtype}/{param_dtype}")
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("R,L", [(5, 103), (63, 9)])
def test_custom_potential(gpu, R, L, dtype):
    eng, tw = make_pair(gpu, R, L, potential=CustomPotential(CUSTOM), dtype=dtype)
    eng.sweep(2); eng.exchange(1); eng.sweep(1)
    got = one_snapshot(eng)
    same_records(got, device_twin_records(eng, tw.beta, R, f32=dtype == "f32"), f"custom {dtype} R={R}")
    eng.close()


# ---- 3. accumulation over snapshots, 4. stream order ----------------------------------------------------------------------------------
def test_accumulation_over_snapshots(gpu):
    R, L = 5, 103
    eng, tw = make_pair(gpu, R, L, potential="double_well", K=2)
    parts = []
    for i in range(3):
        for obj in (eng, tw):
            obj.sweep(2); obj.exchange(1 + i)
        eng.bridge_accumulate()
        parts.append(twin_records(tw))
    got, n = eng.bridge_fetch()
    assert n == 3
    same_records(got, B.merge(parts), "three snapshots")
    same_records(got, B.merge(parts[::-1]), "three snapshots, the other order")
    again, n2 = eng.bridge_fetch()
    assert n2 == 3 and np.array_equal(bits(again), bits(got))
    last, n3 = eng.bridge_fetch(reset=True)
    assert n3 == 3 and np.array_equal(bits(last), bits(got))
    zero, n0 = eng.bridge_fetch()
    assert n0 == 0 and not zero.any()
    eng.close()


def test_stream_order(gpu):
    R, L = 7, 37
    eng, tw = make_pair(gpu, R, L, potential="double_well")
    eng.sweep(2); tw.sweep(2)
    before = twin_records(tw)
    eng.bridge_accumulate()
    eng.sweep(3); tw.sweep(3)                           # queued behind the snapshot: it does not see them
    got, n = eng.bridge_fetch(reset=True)
    assert n == 1
    same_records(got, before, "the snapshot from before the sweep")
    same_records(one_snapshot(eng), twin_records(tw), "the snapshot after it")
    eng.close()


# ---- 5. levels ------------------------------------------------------------------------------------------------------------------------
def test_levels_per_rung_and_across_snapshots(gpu):
    R, L = 4, 80
    beta = np.tile(LADDER(R), L)
    l = np.arange(L)
    sign = np.where(l % 3 == 0, -1.0, 1.0)
    x = np.zeros((L, R))
    x[:, 0] = sign * 1e-3 * (1.0 + 0.37 * np.sin(l))
    x[:, 1] = sign * (0.5 + np.abs(np.sin(0.9 * l)))
    x[:, 2] = sign * 1e20 * (1.0 + 0.37 * np.cos(l))                      # harmonic: e ~ 1e40, EE ~ 1e80
    x[:, 3] = sign * 10.0 ** (-5.0 + 12.0 * l / (L - 1))                  # grows with the ladder index: tops rise after deposits
    eng = plain_engine(gpu, R, L)
    eng.upload_state(x.reshape(-1), beta)
    eng.set_ladder(R)
    got = one_snapshot(eng)
    first = device_twin_records(eng, beta, R)
    same_records(got, first, "levels")
    assert got[0, 0, 1] < got[1, 0, 1] < got[2, 0, 1]                     # word 1 of a record: its top level
    # per rung: a large |x| in rung 2 does not change the words of the other rungs' E and EE records, nor those of rung 0's W and M
    y = x.copy()
    y[:, 2] *= 1e30
    eng.upload_state(y.reshape(-1), beta)
    other = one_snapshot(eng)
    same_records(other, device_twin_records(eng, beta, R), "levels, another rung 2")
    assert np.array_equal(bits(other[[0, 1, 3], :2]), bits(got[[0, 1, 3], :2])) and np.array_equal(bits(other[0]), bits(got[0]))
    # across snapshots: the energies of rung 1 are 2^60 times larger in the second snapshot (harmonic: x times 2^30)
    z = x.copy()
    z[:, 1] *= 2.0 ** 30
    eng.upload_state(x.reshape(-1), beta)
    eng.bridge_accumulate()
    eng.upload_state(z.reshape(-1), beta)
    second = device_twin_records(eng, beta, R)
    eng.bridge_accumulate()
    both, n = eng.bridge_fetch(reset=True)
    assert n == 2
    same_records(both, B.merge([first, second]), "two snapshots, levels 2^60 apart")
    assert both[1, 0, 1] > first[1, 0, 1]
    eng.close()


# ---- 6. flags -------------------------------------------------------------------------------------------------------------------------
def test_flags_stay_with_their_record(gpu):
    R, L = 5, 103
    x, beta = start_state(R, R * L)
    x = x.reshape(L, R)
    x[17, 2] = 7.0            # double well: e = 2304; (-e) (beta_1 - beta_2) = 864 > 710: WB overflows, MB = 1
    eng = plain_engine(gpu, R, L, potential="double_well")
    eng.upload_state(x.reshape(-1), beta)
    eng.set_ladder(R)
    got = one_snapshot(eng)
    same_records(got, device_twin_records(eng, beta, R), "an overflowing WB")
    val = ma._capi.xsum_round(got.reshape(-1, 12)).reshape(R, 6)
    assert val[2, 3] == np.inf and got[2, 3, 2] == 2.0                     # (word 2 of a record: its flags; 2 is +Inf)
    flags = got[:, :, 2].copy()
    flags[2, 3] = 0.0
    assert not flags.any() and np.isfinite(np.delete(val.reshape(-1), 2 * 6 + 3)).all() and 1.0 <= val[2, 5] <= L
    x[17, 2] = np.nan
    eng.upload_state(x.reshape(-1), beta)
    got = one_snapshot(eng)
    same_records(got, device_twin_records(eng, beta, R), "a NaN")
    assert np.all(got[2, :, 2] == 1.0) and not np.delete(got[:, :, 2], 2, axis=0).any()       # every column of rung 2, no other rung
    eng.close()


# ---- 7. end rungs, 8. masks -----------------------------------------------------------------------------------------------------------
def test_end_rungs_and_masks(gpu):
    R, L = 7, 37
    eng, tw = make_pair(gpu, R, L, potential="double_well")
    eng.sweep(1); tw.sweep(1)
    full = one_snapshot(eng)
    same_records(full, twin_records(tw), "all columns")
    for r, c in ((R - 1, 2), (R - 1, 4), (0, 3), (0, 5)):
        assert not full[r, c].any()                                         # all-zero records
    present = np.ones((R, 6), dtype=bool)
    present[R - 1, [2, 4]] = present[0, [3, 5]] = False
    assert np.all(full[present][:, 0] == 2.0)                               # every other slot is a kind-R record
    for c in range(6):
        got = one_snapshot(eng, 1 << c)
        same_records(got, twin_records(tw, 1 << c), f"mask {1 << c}")
        assert np.array_equal(bits(got[:, c]), bits(full[:, c])) and not np.delete(got, c, axis=1).any()
    got = one_snapshot(eng, B.ACCEPTANCE_SET)
    assert np.array_equal(bits(got[:, [0, 1, 4, 5]]), bits(full[:, [0, 1, 4, 5]])) and not got[:, [2, 3]].any()
    eng.close()


def test_two_rungs_are_both_end_rungs(gpu):
    eng, tw = make_pair(gpu, 2, 67, potential="double_well")
    for obj in (eng, tw):
        obj.sweep(1); obj.exchange(1)
    got = one_snapshot(eng)
    same_records(got, twin_records(tw), "R = 2")
    assert not got[1, [2, 4]].any() and not got[0, [3, 5]].any() and got[0, [0, 1, 2, 4], 0].all() and got[1, [0, 1, 3, 5], 0].all()
    eng.close()


# ---- 9. grid stride -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,L", [(6, 30001), (3, 100003)])
def test_grid_stride(gpu, monkeypatch, R, L):
    """One block per CU: 6 x 30 001 chains walk the grid three times (the tail loop), 3 x 100 003 five times (four loads in flight, then
    the tail)."""
    monkeypatch.setenv("AMC_BLOCKS_PER_CU", "1")
    x, beta = start_state(R, R * L)
    eng = plain_engine(gpu, R, L, potential="double_well")
    monkeypatch.delenv("AMC_BLOCKS_PER_CU")
    eng.upload_state(x, beta)
    eng.set_ladder(R)
    eng.sweep(1); eng.exchange(2)
    got = one_snapshot(eng)
    same_records(got, device_twin_records(eng, beta, R), "grid stride")
    eng.close()


# ---- 10. shard invariance -------------------------------------------------------------------------------------------------------------
def test_shard_invariance(gpu):
    R, L = 3, 342
    M = R * L
    def seq(o):
        o.sweep(2); o.exchange(1); o.bridge_accumulate(); o.sweep(1); o.exchange(1); o.bridge_accumulate()
    whole, _ = make_pair(gpu, R, L, potential="double_well", K=2)
    seq(whole)
    rec_w, n_w = whole.bridge_fetch()
    assert n_w == 2
    for split in ([0, 402, M], [0, 258, 264, M]):
        parts = [make_pair(gpu, R, (b - a) // R, potential="double_well", K=2, offset=a, n_global=M)[0] for a, b in zip(split, split[1:])]
        merged = None
        for p in parts:
            seq(p)
            rec, n = p.bridge_fetch()
            assert n == 2
            rec = rec.reshape(-1, 12)
            merged = rec if merged is None else ma._capi.xsum_merge(merged, rec)
        assert np.array_equal(bits(merged), bits(rec_w.reshape(-1, 12))), split
        for p in parts:
            p.close()
    whole.close()


# ---- 11. nothing else changes ---------------------------------------------------------------------------------------------------------
def _everything(eng, track):
    out = list(eng.download_state()) + list(eng.download_counters()) + list(eng.exchange_counters())
    out += [np.array([eng.step, eng.estimator_step, eng.exchange_step])]
    if track:
        out += list(eng.labels()) + [np.array(eng.tracking_counters())]
    return out


@pytest.mark.parametrize("mode", ["tracking", "rung_sigma"])
def test_accumulating_changes_nothing_else(gpu, mode):
    R, L = 5, 103
    pair = [make_pair(gpu, R, L, potential="double_well", K=2)[0] for _ in range(2)]
    for eng in pair:
        if mode == "tracking":
            eng.set_tracking(True)
        else:
            eng.set_rung_sigma(np.outer([0.5, 0.25], 1.0 / np.sqrt(LADDER(R) / 0.5)))
    for _ in range(20):
        for i, eng in enumerate(pair):
            eng.sweep(1); eng.exchange(1)
            if i == 0:
                eng.bridge_accumulate()
    assert pair[0].bridge_fetch()[1] == 20
    a, b = (_everything(eng, mode == "tracking") for eng in pair)
    assert len(a) == len(b) and all(np.array_equal(u, v) and (u.dtype.kind != "f" or np.array_equal(bits(u), bits(v))) for u, v in zip(a, b))
    if mode == "rung_sigma":
        assert np.array_equal(bits(pair[0].rung_sigma()), bits(pair[1].rung_sigma()))
        assert all(np.array_equal(u, v) for u, v in zip(pair[0].rung_window_counts(), pair[1].rung_window_counts()))
    for eng in pair:
        eng.close()


# ---- 12. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was(gpu):
    R, L = 3, 22
    x, beta = start_state(R, R * L)
    eng = plain_engine(gpu, R, L)
    eng.upload_state(x, beta)
    for call in (eng.bridge_accumulate, eng.bridge_fetch, eng.set_bridge):
        with pytest.raises(gpu.AmcError, match=r"amc error -5.*amc_(bridge_accumulate|bridge_fetch|set_bridge).*no ladder"):
            call()
    eng.set_ladder(R)
    for cols in (0, 64, -1, 127):
        with pytest.raises(gpu.AmcError, match=r"amc error -1.*amc_bridge_accumulate.*columns"):
            eng.bridge_accumulate(cols)
    assert eng.bridge_fetch()[1] == 0
    eng.sweep(1)
    eng.bridge_accumulate(B.ACCEPTANCE_SET)
    before = eng.bridge_fetch()
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*amc_bridge_accumulate.*begun with 51"):
        eng.bridge_accumulate(B.ALL)
    bad = before[0].copy()
    bad[R - 1, 4] = bad[0, 4]                                  # MF at the last rung has no summand
    with pytest.raises(gpu.AmcError, match=r"amc error -1.*amc_set_bridge"):
        eng.set_bridge(bad, 1)
    after = eng.bridge_fetch()
    assert after[1] == before[1] == 1 and np.array_equal(bits(after[0]), bits(before[0]))
    same_records(after[0], device_twin_records(eng, beta, R, B.ACCEPTANCE_SET), "after the refusals")
    eng.bridge_fetch(reset=True)
    eng.bridge_accumulate(B.ALL)                               # the reset freed the mask
    same_records(eng.bridge_fetch()[0], device_twin_records(eng, beta, R), "another mask after the reset")
    eng.set_ladder(0)
    for call in (eng.bridge_accumulate, eng.bridge_fetch, eng.set_bridge):
        with pytest.raises(gpu.AmcError, match=r"amc error -5"):
            call()
    eng.sweep(1)
    eng.close()


# ---- 13. life cycle -------------------------------------------------------------------------------------------------------------------
def test_life_cycle(gpu):
    R, L = 4, 129
    eng, tw = make_pair(gpu, R, L, potential="double_well")
    eng.sweep(2)
    eng.respace_ladder("acceptance", 1.0, 0.01)                # refused on the device: no gap was attempted yet
    assert eng.respace_status()[0] == 2
    eng.bridge_accumulate()
    first = eng.bridge_fetch()
    assert first[1] == 1
    eng.respace_ladder("acceptance", 1.0, 0.01)                # refused again: the accumulator stays
    assert eng.respace_status()[0] == 2
    x = eng.download_state()[0]
    eng.upload_state(x, tw.beta)                               # upload_state leaves it alone
    eng.set_rung_sigma(np.full((1, R), 0.5))
    eng.sweep_exchange(8, 1)
    eng.tune_rung_sigma(min_calls=1)                           # ... and so does a tuning
    kept = eng.bridge_fetch()
    assert kept[1] == 1 and np.array_equal(bits(kept[0]), bits(first[0]))
    eng.respace_ladder("acceptance", 1.0, 0.01)                # taken: sums at other beta belong to another ladder
    assert eng.respace_status() == (0, 1)
    gone = eng.bridge_fetch()
    assert gone[1] == 0 and not gone[0].any()
    eng.bridge_accumulate()                                    # ... and the accumulator goes on at the new ladder
    beta_new = np.tile(eng.ladder(), L)
    same_records(eng.bridge_fetch()[0], device_twin_records(eng, beta_new, R), "after the respacing")
    eng.set_ladder(R)                                          # set_ladder clears it
    gone = eng.bridge_fetch()
    assert gone[1] == 0 and not gone[0].any()
    eng.close()


def test_set_bridge_restores_the_accumulator(gpu):
    R, L = 5, 103
    a, _ = make_pair(gpu, R, L, potential="double_well")
    b, _ = make_pair(gpu, R, L, potential="double_well")
    for eng in (a, b):
        eng.sweep(1); eng.exchange(1); eng.bridge_accumulate(B.ACCEPTANCE_SET); eng.sweep(1); eng.bridge_accumulate(B.ACCEPTANCE_SET)
    rec, n = b.bridge_fetch()
    b.set_bridge(None)
    assert b.bridge_fetch()[1] == 0
    b.set_bridge(rec, n)
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*begun with 51"):
        b.bridge_accumulate(B.ALL)                             # the mask came back with the records
    for eng in (a, b):
        eng.sweep(2); eng.exchange(1); eng.bridge_accumulate(B.ACCEPTANCE_SET)
    ra, rb = a.bridge_fetch(), b.bridge_fetch()
    assert ra[1] == rb[1] == 3 and np.array_equal(bits(ra[0]), bits(rb[0]))
    # a level word or a flag word that is no integer is refused, as amc_set_corr refuses it, and the accumulator stays as it was
    for word, value in ((1, 0.5), (2, 0.5)):
        bad = rb[0].copy()
        bad[1, 0, word] = value
        with pytest.raises(gpu.AmcError, match=r"amc error -1.*amc_set_bridge.*rung 1, column 0 is no kind-R record"):
            b.set_bridge(bad, 3)
    after = b.bridge_fetch()
    assert after[1] == 3 and np.array_equal(bits(after[0]), bits(rb[0]))
    a.close(); b.close()


def _build(path, steps, fuse_marker=None):
    chains = ma.ParticleChains.ladder(171, [0.5, 1.0, 2.0], x=start_state(3, 513)[0], potential="double_well")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=4, per_chain_counters=True),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), bridge=True, bridge_every=2)]
    return ma.Simulation(chains, al, steps, path=str(path))


def test_checkpoint_and_resume_accumulate_on_to_the_same_bits(gpu, tmp_path):
    whole = _build(tmp_path / "w", 20)
    ma.run(whole)
    first = _build(tmp_path / "a", 10)
    ma.run(first)
    assert first.algorithms[0].engine.exchange_step == 5 and first.algorithms[0].engine.bridge_fetch()[1] == 2
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    second = _build(tmp_path / "b", 10)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    r1, r2 = whole.algorithms[0].engine.bridge_fetch(), second.algorithms[0].engine.bridge_fetch()
    assert r1[1] == r2[1] == 5 and np.array_equal(bits(r1[0]), bits(r2[0]))
    assert np.array_equal(bits(whole.algorithms[1].log_z()), bits(second.algorithms[1].log_z()))
    # no bridge, no new field
    plain = ma.Simulation(ma.ParticleChains.ladder(9, [0.5, 1.0, 2.0], potential="double_well"),
                          [dict(algorithm=ma.Metropolis, pool=(ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),), seed=4),
                           dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(4, 0, 2))], 4,
                          path=str(tmp_path / "p"))
    ma.run(plain)
    fn = ma.checkpoint(plain.algorithms[0], str(tmp_path / "ckp"))
    assert not [k for k in np.load(fn).files if k.startswith("bridge")]
    assert {"bridge_records", "bridge_columns", "bridge_snapshots"} <= set(np.load(os.path.join(str(tmp_path / "ck"), "checkpoint_rank0.npz")).files)


# ---- 14. through the host mirror ------------------------------------------------------------------------------------------------------
MIRROR = dict(steps=24, R=3, L=41, betas=[0.5, 1.0, 2.0], every=3, bridge_every=2, seed=9)


def _run(tmp, fuse):
    m = MIRROR
    x = start_state(m["R"], m["R"] * m["L"])[0]
    chains = ma.ParticleChains.ladder(m["L"], m["betas"], x=x, potential="double_well")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=m["seed"]),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(m["steps"], 0, m["every"]), bridge=True,
               bridge_every=m["bridge_every"]),
          dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_log_z, ma.callback_heat_capacity), scheduler=ma.build_schedule(m["steps"], 0, 8))]
    sim = ma.Simulation(chains, al, m["steps"], path=str(tmp))
    ma.run(sim, fuse=fuse)
    files = {f: open(os.path.join(str(tmp), f)).read() for f in ("log_z.dat", "heat_capacity.dat")}
    return sim.algorithms[2].rows, files, sim.chains.x.copy()


def test_callbacks_through_the_host_mirror(gpu, tmp_path):
    a = _run(tmp_path / "stepwise", False)
    b = _run(tmp_path / "fused", True)
    assert a[1] == b[1] and np.array_equal(bits(a[2]), bits(b[2]))
    for rows_a, rows_b in zip(a[0], b[0]):
        assert [t for t, _ in rows_a] == [t for t, _ in rows_b] and {8, 16, 24} <= {t for t, _ in rows_a}
        assert all(np.array_equal(bits(u), bits(v)) for (_, u), (_, v) in zip(rows_a, rows_b))
    # the twin of the whole run: a sweep per time step, an exchange step every third, a snapshot behind every second exchange step
    m = MIRROR
    R, M = m["R"], m["R"] * m["L"]
    x = start_state(R, M)[0]
    beta = np.tile(m["betas"], m["L"])
    sim = O.OracleSim(M, potential="double_well", beta=1.0, sigma=[0.5], weight=[1.0], seed=m["seed"])
    sim.set_beta(beta)
    tw = X.ExchangeTwin(sim, beta, R, seed=m["seed"], potential="double_well")
    tw.state.put(x, tw.pot)
    parts, at = [], {}
    for t in range(1, m["steps"] + 1):
        tw.sweep(1)
        if t % m["every"] == 0:
            tw.exchange(1)
            if tw.t_x % m["bridge_every"] == 0:
                parts.append(twin_records(tw))
        if t % 8 == 0:
            at[t] = B.merge(parts) if parts else None
    assert np.array_equal(bits(a[2]), bits(tw.state.get())), "the run's final state differs from the twin's"
    n_ladders = float(m["L"])
    for rows in (a[0], b[0]):
        log_z, heat = dict(rows[0]), dict(rows[1])
        for t, rec in at.items():
            n = float(sum(1 for s in range(1, t + 1) if s % (m["every"] * m["bridge_every"]) == 0)) * n_ladders
            want_z = np.concatenate([[0.0], np.cumsum(B.log_z_acceptance(rec))])
            assert np.array_equal(bits(log_z[t]), bits(want_z)), (t, log_z[t], want_z)
            want_c = B.heat_capacity(rec, n, m["betas"])
            assert np.array_equal(bits(heat[t]), bits(want_c)), (t, heat[t], want_c)


# ---- 15. statistics on the device -----------------------------------------------------------------------------------------------------
def test_statistics_of_an_exact_gaussian_ensemble(gpu, tmp_path):
    R = BETAS.size
    x, beta = gaussian_ensemble()
    chains = ma.ParticleChains.ladder(GAUSS_L, list(BETAS), x=x, potential="harmonic")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=1),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(1, 0, 1), bridge=True)]
    sim = ma.Simulation(chains, al, 1, path=str(tmp_path))
    for alg in sim.algorithms:
        alg.initialise(sim)
    met, rx = sim.algorithms
    met.engine.bridge_accumulate(rx.bridge)                    # one snapshot of the uploaded ensemble, nothing stepped
    cols = numpy_summands(x, beta, R)
    est, se = acceptance_estimate_and_error(cols)
    got = rx.log_z_ratios("acceptance")
    print("device", got, "numpy", est, "standard errors", se)
    assert got.shape == (R - 1,) and np.allclose(got, est, rtol=1e-12, atol=0.0)
    assert np.all(np.abs(got - 0.5 * np.log(BETAS[:-1] / BETAS[1:])) < 5.0 * se)
    e = cols[0]
    var = e.var(axis=0)                                         # heat capacity beta^2 var(e) = 1 / 2 for the harmonic well
    d = (e - e.mean(axis=0)) ** 2
    se_c = BETAS ** 2 * d.std(axis=0, ddof=1) / np.sqrt(GAUSS_L)
    heat = rx.heat_capacity()
    print("heat capacity", heat, "numpy", BETAS ** 2 * var, "standard errors", se_c)
    assert heat.shape == (R,) and np.all(np.abs(heat - 0.5) < 5.0 * se_c)
    assert np.allclose(rx.log_z(), np.concatenate([[0.0], np.cumsum(got)]), rtol=0, atol=0)
    with pytest.raises(ValueError, match="leaves out"):
        rx.log_z_ratios("exponential")                         # (the default mask holds no W column)
    for alg in sim.algorithms:
        alg.finalise(sim)
