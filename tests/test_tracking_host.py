"""Walker tracking (DESIGN.md section 3.13 "Walker tracking") without a GPU: the rules as the host twin states them (tests/track_twin.py)
against values worked out by hand, their invariants, argument validation through the C ABI (a NULL handle: the refusals of a live handle
without a ladder need a device and are in test_gpu_tracking.py), and checkpoints, callbacks and run()'s scheduling through the
engine_factory seam."""
import ctypes as C

import numpy as np
import pytest

import montecarlo_amd as ma

import exchange_twin as X
import track_twin as T
from test_exchange_host import _flat, _recording


def _twin(oracle, n_ladders, betas, *, seed=3, offset=0, potential="harmonic"):
    R = len(betas)
    n = n_ladders * R
    ids = np.arange(offset, offset + n)
    x = np.sin(0.37 * ids + 0.1) * 1.7
    beta = np.tile(np.asarray(betas, dtype=np.float64), n_ladders)
    sim = oracle.OracleSim(n, chain_offset=offset, potential=potential, beta=1.0, sigma=[0.4], weight=[1.0], seed=seed)
    sim.set_x(x)
    sim.set_beta(beta)
    tw = T.TrackTwin(sim, beta, R, seed=seed, potential=potential, chain_offset=offset)
    tw.set_tracking(True)
    return sim, tw


@pytest.mark.parametrize("R", [2, 3, 4, 5])
def test_equal_beta_trips_worked_out_by_hand(oracle, R):
    """Equal beta: every attempted swap is accepted, so the steps are the rounds of an odd-even transposition network and every walker
    moves ballistically.  A walker at an even rung first moves up, one at an odd rung first moves down (step 0 attempts the even
    gaps); at an end it waits one step when its gap is not due, then turns.  That path closes after 2R steps (R - 1 moves up, R - 1
    moves down, two waits) and arrives exactly once at either end on the way, so after 4R steps the walker ids are the identity again
    and every walker has arrived twice at rung 0 and twice at rung R - 1, alternately.  An arrival counts unless it is the walker's
    first visit of any end: that is the case for the first arrival of the walkers that start in the middle (d = 0), and for nobody
    else (walker 0 starts with d = 1 and first arrives at rung R - 1, walker R - 1 starts with d = 2 and first arrives at rung 0).
    A middle walker at an odd rung loses its first arrival at rung 0, one at an even rung its first arrival at rung R - 1:
        round_trips per ladder = 2R - #{odd r in [1, R - 2]},   up_trips per ladder = 2R - #{even r in [1, R - 2]}
    and the last end a walker saw is rung 0 when it moved up first (even start, d = 1) and rung R - 1 otherwise (d = 2)."""
    by_hand = {2: (4, 4, [0 | 64, 1 | 128]),
               3: (5, 6, [0 | 64, 1 | 128, 2 | 128]),
               4: (7, 7, [0 | 64, 1 | 128, 2 | 64, 3 | 128]),
               5: (8, 9, [0 | 64, 1 | 128, 2 | 64, 3 | 128, 4 | 128])}
    rt, up, lab = by_hand[R]
    L = 7
    sim, tw = _twin(oracle, L, [1.25] * R)
    x0 = sim.state()[0].copy()
    half = None
    for step in range(4 * R):
        tw.exchange(1)
        if step + 1 == R:
            half = tw.lab.copy()
    acc, att = tw.counters()
    assert np.array_equal(acc, att) and att.sum() > 0
    assert np.array_equal((half & 63).reshape(L, R), np.tile(np.arange(R)[::-1], (L, 1)))      # R rounds reverse every ladder
    assert np.array_equal(tw.lab, np.tile(np.array(lab, dtype=np.uint8), L))
    assert (tw.round_trips, tw.up_trips) == (rt * L, up * L) and rt > 0 and up > 0
    assert np.array_equal(sim.state()[0].view(np.uint64), x0.view(np.uint64))                  # the positions travelled with them


@pytest.mark.parametrize("R", [2, 3, 6])
def test_invariants_hold_after_every_step(oracle, R):
    """Walker ids stay a permutation per ladder, rung 0 holds d = 1 and rung R - 1 d = 2, the flow counts add up to the ladder count,
    the labels travel with the positions, and the trip counters never decrease."""
    L = 23
    betas = list(0.4 * 1.35 ** np.arange(R))
    sim, tw = _twin(oracle, L, betas, potential="double_well")
    x_of_walker = sim.state()[0].reshape(L, R).copy()              # tracking starts now: walker w of ladder l carries x[l, w]
    trips = (0, 0)
    for step in range(3 * R + 4):
        tw.exchange(1)
        T.check_labels(tw.lab, R)
        n = tw.flow_rungs()
        assert np.all(n.sum(axis=1) == L) and n[0, 1] == L and n[R - 1, 2] == L
        x = sim.state()[0].reshape(L, R)
        w = (tw.lab & 63).reshape(L, R).astype(np.int64)
        assert np.array_equal(x.view(np.uint64), np.take_along_axis(x_of_walker, w, axis=1).view(np.uint64))
        assert tw.round_trips >= trips[0] and tw.up_trips >= trips[1]
        trips = (tw.round_trips, tw.up_trips)
    acc, att = tw.counters()
    assert 0 < acc.sum() < att.sum()                               # (some swaps were rejected: a rejected swap writes nothing)


def test_tracking_changes_nothing_else_and_does_not_depend_on_the_split(oracle):
    betas, L = [0.5, 1.5, 4.0], 24
    seq = lambda o: (o.sweep(2), o.exchange(1), o.sweep(1), o.exchange(4))
    sim, tw = _twin(oracle, L, betas)
    seq(tw)
    plain_sim = oracle.OracleSim(3 * L, potential="harmonic", beta=1.0, sigma=[0.4], weight=[1.0], seed=3)
    plain_sim.set_x(np.sin(0.37 * np.arange(3 * L) + 0.1) * 1.7)
    plain_sim.set_beta(np.tile(betas, L))
    plain = X.ExchangeTwin(plain_sim, np.tile(betas, L), 3, seed=3)
    seq(plain)
    assert np.array_equal(sim.state()[0].view(np.uint64), plain_sim.state()[0].view(np.uint64))
    assert np.array_equal(tw.accepted, plain.accepted) and np.array_equal(tw.attempted, plain.attempted) and tw.t_x == plain.t_x
    parts = []
    for a, b in [(0, 33), (33, 72)]:
        psim, p = _twin(oracle, (b - a) // 3, betas, offset=a)
        seq(p)
        parts.append(p)
    assert np.array_equal(np.concatenate([p.lab for p in parts]), tw.lab)
    assert sum(p.round_trips for p in parts) == tw.round_trips and sum(p.up_trips for p in parts) == tw.up_trips
    assert np.array_equal(sum(p.flow_rungs() for p in parts), tw.flow_rungs())


def test_new_entries_refuse_a_null_handle(amc):
    lib = amc.load()
    new = ["amc_set_tracking", "amc_download_labels", "amc_upload_labels", "amc_flow_rungs", "amc_tracking_counters",
           "amc_set_tracking_counters"]
    for name in new:
        assert name in amc.SIGNATURES
        res, args = amc.SIGNATURES[name]
        zeros = [None if (a is C.c_void_p or hasattr(a, "contents")) else a(0) for a in args]
        assert getattr(lib, name)(*zeros) == -1, name
        assert name.encode() in lib.amc_last_error()


# ---- run(), callbacks and checkpoints over the engine double ----------------------------------------------------------------------
def _rx_sim(path, factory, steps, every, extra, track):
    chains = ma.ParticleChains.ladder(6, [0.5, 1.0, 2.0], x=np.linspace(-1.5, 1.5, 18))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 0.7), ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.2], 0.3))
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=7, engine_factory=factory),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, every), track=track)]
    return ma.Simulation(chains, al + extra, steps, path=str(path))


def test_fused_and_stepwise_runs_issue_the_same_steps_with_tracking(oracle, tmp_path):
    steps = 31
    out = []
    for i, fuse in enumerate((False, True)):
        calls = []

        class Recording(_recording(calls), T.TrackEngine):
            pass
        extra = [dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_energy, ma.callback_flow_fraction, ma.callback_round_trips),
                      scheduler=ma.build_schedule(steps, 0, 10))]
        sim = _rx_sim(tmp_path / str(i), Recording, steps, 3, extra, True)
        ma.run(sim, fuse=fuse)
        eng = sim.algorithms[0].engine
        files = {f: open(tmp_path / str(i) / f).read() for f in ("energy.dat", "flow_fraction.dat", "round_trips.dat")}
        out.append((_flat(calls), [c for c in calls if isinstance(c, tuple)], eng.labels(), eng.tracking_counters(), eng.flow_rungs(), files))
    (seq0, grouped0, lab0, trips0, flow0, files0), (seq1, grouped1, lab1, trips1, flow1, files1) = out
    assert seq0 == seq1 == (["S"] * 3 + ["X"]) * 10 + ["S", "X"]
    assert grouped0 == [] and len(grouped1) > 0
    assert np.array_equal(lab0[0], lab1[0]) and np.array_equal(lab0[1], lab1[1]) and trips0 == trips1 and np.array_equal(flow0, flow1)
    assert files0 == files1
    first = files0["flow_fraction.dat"].splitlines()[0]
    assert "NaN" in first                                          # t = 0: the middle rung has seen no end yet, 0/0
    assert len(files0["round_trips.dat"].splitlines()[-1].split()) == 3          # t and the two counts


def test_callbacks_refuse_an_untracked_algorithm(oracle, tmp_path):
    sim = _rx_sim(tmp_path, T.TrackEngine, 4, 1, [], False)
    ma.run(sim)
    for cb in (ma.callback_flow_fraction, ma.callback_round_trips):
        with pytest.raises(ValueError, match="track=True"):
            cb(sim)
    tracked = _rx_sim(tmp_path / "t", T.TrackEngine, 4, 1, [], True)
    ma.run(tracked)
    f = ma.callback_flow_fraction(tracked)
    assert f.shape == (3,) and f[0] == 1.0 and f[2] == 0.0
    assert ma.callback_round_trips(tracked).shape == (2,)


def test_checkpoint_carries_the_tracking_state(oracle, tmp_path):
    """Checkpoint after an odd number of exchange steps, restore, continue: the labels and trip counters of the uninterrupted run.  A
    checkpoint of an untracked run has none of the new keys, and one written through an engine without the new surface
    (exchange_twin.TwinEngine) is written and restored as before."""
    new_keys = {"walker", "direction", "trips"}

    def build(path, steps, factory=T.TrackEngine, track=True):
        return _rx_sim(path, factory, steps, 2, [], track)
    whole = build(tmp_path / "w", 12)
    ma.run(whole)
    first = build(tmp_path / "a", 6)
    ma.run(first)
    eng = first.algorithms[0].engine
    assert eng.exchange_step == 3
    at_6 = eng.tracking_counters()
    eng.set_tracking_counters(at_6[0] + 5, at_6[1] + 9)            # (the counters are restored as saved and counted on from there)
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    saved = np.load(tmp_path / "ck" / "checkpoint_rank0.npz")
    assert new_keys <= set(saved.files) and saved["trips"].tolist() == [at_6[0] + 5, at_6[1] + 9]
    assert np.array_equal(saved["walker"], eng.labels()[0]) and np.array_equal(saved["direction"], eng.labels()[1])
    second = build(tmp_path / "b", 6)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)                                                 # (initialise must not reset the restored labels)
    e1, e2 = whole.algorithms[0].engine, second.algorithms[0].engine
    assert np.array_equal(whole.chains.x.view(np.uint64), second.chains.x.view(np.uint64))
    assert all(np.array_equal(a, b) for a, b in zip(e1.labels(), e2.labels()))
    assert not np.array_equal(e1.labels()[0], np.tile(np.arange(3, dtype=np.uint8), 6))        # (walkers did move)
    assert e2.tracking_counters() == (e1.tracking_counters()[0] + 5, e1.tracking_counters()[1] + 9)
    for factory in (T.TrackEngine, X.TwinEngine):
        plain = build(tmp_path / f"p{factory.__name__}", 6, factory, False)
        ma.run(plain)
        ma.checkpoint(plain.algorithms[0], str(tmp_path / f"ck{factory.__name__}"))
        assert not new_keys & set(np.load(tmp_path / f"ck{factory.__name__}" / "checkpoint_rank0.npz").files)
        again = build(tmp_path / f"q{factory.__name__}", 6, factory, False)
        ma.restore(again.algorithms[0], str(tmp_path / f"ck{factory.__name__}"))
        ma.run(again)
        assert np.array_equal(whole.chains.x.view(np.uint64), again.chains.x.view(np.uint64))

