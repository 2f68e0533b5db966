"""RespaceLadder in an algorithm list (montecarlo_amd/exchange.py): the stepwise and the fused run agree bit for bit, ``until`` is
respected, callback_ladder writes the ladder's history through StoreCallbacks, chains.beta_array follows the device, and a run
interrupted by checkpoint / restore continues bit for bit."""
import os

import numpy as np
import pytest

import montecarlo_amd as ma

from test_gpu_exchange import bits, start_state

pytestmark = pytest.mark.gpu
R, L = 4, 129
START = [0.6, 0.7, 0.85, 2.4]


def build(path, steps, *, rule="flow", respace_at=(12, 24), until=None, gamma=0.9, store=True):
    chains = ma.ParticleChains.ladder(L, START, x=start_state(R, R * L)[0], potential="double_well")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=4, per_chain_counters=True),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), track=True),
          dict(algorithm=ma.RespaceLadder, dependencies=(ma.ReplicaExchange,), scheduler=[t for t in respace_at if t <= steps], rule=rule,
               gamma=gamma, eps=0.01, until=until)]
    if store:
        al.append(dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_ladder,), scheduler=ma.build_schedule(steps, 0, 6)))
    return ma.Simulation(chains, al, steps, path=str(path))


def state(sim):
    eng = sim.algorithms[0].engine
    w, d = eng.labels()
    return [bits(sim.chains.x), bits(eng.ladder()), *eng.exchange_counters(), w, d, np.array(eng.tracking_counters()),
            np.array([eng.exchange_step, eng.step, *eng.respace_status()])]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("rule", ["flow", "acceptance"])
def test_fused_run_equals_stepwise_run(gpu, tmp_path, rule):
    a, b = build(tmp_path / "stepwise", 36, rule=rule), build(tmp_path / "fused", 36, rule=rule)
    ma.run(a)
    ma.run(b, fuse=True)
    assert same(state(a), state(b))
    rl = a.algorithms[2]
    assert [t for t, _ in rl.statuses] == [12, 24] and a.algorithms[0].engine.respace_status()[1] == sum(s == 0 for _, s in rl.statuses) > 0
    assert rl.statuses == b.algorithms[2].statuses
    files = [open(os.path.join(str(tmp_path / d), "ladder.dat")).read() for d in ("stepwise", "fused")]
    assert files[0] == files[1]
    # chains.beta_array holds the new ladder, and so does ReplicaExchange.betas()
    lad = a.algorithms[1].betas()
    assert np.array_equal(a.chains.beta_array, np.tile(lad, L)) and not np.array_equal(lad, START)
    assert lad[0] == START[0] and lad[-1] == START[-1] and np.all(np.diff(lad) > 0)


def test_callback_ladder_writes_the_history(gpu, tmp_path):
    sim = build(tmp_path / "run", 36)
    ma.run(sim)
    lines = [ln for ln in open(os.path.join(str(tmp_path / "run"), "ladder.dat")).read().splitlines() if ln.strip()]
    rows = dict(sim.algorithms[3].rows[0])                     # t -> the ladder at t (the file's rows, in memory)
    assert len(lines) == len(sim.algorithms[3].rows[0]) >= 6 and lines[0].startswith("0 ")
    assert np.array_equal(rows[0], START) and np.array_equal(rows[6], START)                    # before the first respacing (t = 12)
    assert not np.array_equal(rows[12], START) and np.array_equal(rows[12], rows[18])           # behind it, at the same t already
    assert not np.array_equal(rows[24], rows[18]) and np.array_equal(rows[36], sim.algorithms[1].betas())
    assert all(len(v) == R and np.all(np.diff(v) > 0) for v in rows.values())


def test_until_is_respected(gpu, tmp_path):
    a = build(tmp_path / "a", 36, respace_at=(12, 24), until=20, store=False)
    b = build(tmp_path / "b", 36, respace_at=(12,), store=False)
    ma.run(a); ma.run(b)
    assert [t for t, _ in a.algorithms[2].statuses] == [12]
    assert same(state(a), state(b))


def test_checkpoint_restore_continue(gpu, tmp_path):
    whole = build(tmp_path / "w", 36, store=False)
    ma.run(whole)
    first = build(tmp_path / "a", 20, store=False)
    ma.run(first)
    assert first.algorithms[0].engine.respace_status()[1] == 1
    fn = ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    saved = np.load(fn)
    assert int(saved["n_respaced"]) == 1 and np.array_equal(saved["beta"], np.tile(first.algorithms[1].betas(), L))
    # the rest of the run: 16 steps, the second respacing at its step 4 (global 24)
    second = build(tmp_path / "b", 16, respace_at=(4,), store=False)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    assert same(state(whole), state(second))
    assert np.array_equal(second.chains.beta_array, whole.chains.beta_array)
    # no respacing, no new field
    plain = build(tmp_path / "p", 8, respace_at=(), store=False)
    ma.run(plain)
    assert "n_respaced" not in np.load(ma.checkpoint(plain.algorithms[0], str(tmp_path / "ck2")))
