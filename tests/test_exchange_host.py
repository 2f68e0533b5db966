"""Replica exchange without a GPU: properties of the step as the host twin states it (tests/exchange_twin.py),
argument validation through the C ABI, and run()'s scheduling of [Metropolis, ReplicaExchange] through the engine_factory seam."""
import ctypes as C

import numpy as np
import pytest

import montecarlo_amd as ma

import exchange_twin as X


def _ladder_sim(oracle, n_ladders, betas, *, potential="harmonic", seed=3, offset=0, n_local=None, dtype="f64"):
    """(OracleSim over chains [offset, offset + n_local), its ExchangeTwin) of an ensemble of n_ladders ladders whose positions are
    a fixed function of the GLOBAL chain id."""
    R = len(betas)
    M = n_ladders * R
    n_local = M - offset if n_local is None else n_local
    ids = np.arange(offset, offset + n_local)
    x = np.sin(0.37 * ids + 0.1) * 1.7
    beta = np.tile(np.asarray(betas, dtype=np.float64), n_ladders)[offset:offset + n_local]
    sim = oracle.OracleSim(n_local, chain_offset=offset, potential=potential, beta=1.0, sigma=[0.4], weight=[1.0], seed=seed, dtype=dtype)
    sim.set_x(x)
    sim.set_beta(beta)
    return sim, X.ExchangeTwin(sim, beta, R, seed=seed, potential=potential, chain_offset=offset, f32=dtype == "f32")


@pytest.mark.parametrize("f32", [False, True])
def test_equal_beta_always_swaps(oracle, f32):
    """At equal beta the two sums of delta hold the same two products: delta == 0 exactly, alpha == 1 > u for every u in [0, 1)."""
    rng = np.random.default_rng(5)
    for pot in (0, 1):
        for xa, xb, b in zip(rng.normal(size=200) * 3, rng.normal(size=200) * 3, rng.uniform(0.1, 40.0, size=200)):
            for u in (0.0, 0.5, 1.0 - 2.0 ** -52):
                assert X.swap_decision(pot, xa, xb, b, b, u, f32)
    assert not X.swap_decision(0, np.nan, 1.0, 1.0, 2.0, 0.0)                # a NaN delta rejects
    assert not X.swap_decision(0, np.inf, np.inf, 1.0, 2.0, 0.0)             # (inf - inf)


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
def test_a_step_permutes_positions_inside_each_ladder(oracle, potential):
    betas = [0.5, 1.0, 2.0, 4.0, 8.0]
    sim, tw = _ladder_sim(oracle, 41, betas, potential=potential)
    x0 = sim.state()[0].reshape(41, 5)
    for step in range(4):
        tw.exchange(1)
        x, e = sim.state()
        assert np.array_equal(np.sort(x.reshape(41, 5), axis=1).view(np.uint64), np.sort(x0, axis=1).view(np.uint64))
        assert np.array_equal(e, ma.potential(potential, x))                                 # e == potential(x)
    acc, att = tw.counters()
    assert 0 < acc.sum() < att.sum()


@pytest.mark.parametrize("R", [2, 3, 4, 5])
def test_gap_selection(oracle, R):
    assert X.gaps_of_step(R, 0) == list(range(0, R - 1, 2)) and X.gaps_of_step(R, 1) == list(range(1, R - 1, 2))
    if R == 2:
        assert X.gaps_of_step(2, 1) == []
    betas = list(0.5 * 2.0 ** np.arange(R))
    n_ladders = 7
    sim, tw = _ladder_sim(oracle, n_ladders, betas)
    for step in range(4):
        before = sim.state()[0].reshape(n_ladders, R).copy()
        att0 = tw.attempted.copy()
        tw.exchange(1)
        after = sim.state()[0].reshape(n_ladders, R)
        gaps = X.gaps_of_step(R, step)
        expect = np.zeros(R - 1, dtype=np.int64)
        expect[gaps] = n_ladders
        assert np.array_equal(tw.attempted - att0, expect)
        touched = sorted({c for r in gaps for c in (r, r + 1)})
        untouched = [c for c in range(R) if c not in touched]
        assert np.array_equal(before[:, untouched], after[:, untouched])
        for r in gaps:          # a gap either swapped or stayed; rungs 0 and R - 1 never meet across ladders
            same = (before[:, r] == after[:, r]) & (before[:, r + 1] == after[:, r + 1])
            swapped = (before[:, r] == after[:, r + 1]) & (before[:, r + 1] == after[:, r])
            assert np.all(same | swapped)
    assert tw.t_x == 4


def test_draws_do_not_depend_on_the_shard_split(oracle):
    """The draw of gap (l, r) is keyed by the GLOBAL id of its lower chain: one shard, two and three shards give the same bits and
    gap counters that add up."""
    betas, n_ladders = [0.5, 1.5, 4.0], 24
    for split in ([0, 33, 72], [0, 12, 45, 72]):
        parts = [_ladder_sim(oracle, n_ladders, betas, offset=a, n_local=b - a) for a, b in zip(split, split[1:])]
        ref_sim, ref = _ladder_sim(oracle, n_ladders, betas)
        for obj in [ref] + [p[1] for p in parts]:
            obj.sweep(2); obj.exchange(1); obj.sweep(1); obj.exchange(2)
        x = np.concatenate([p[0].state()[0] for p in parts])
        assert np.array_equal(x.view(np.uint64), ref_sim.state()[0].view(np.uint64))
        assert np.array_equal(sum(p[1].accepted for p in parts), ref.accepted)
        assert np.array_equal(sum(p[1].attempted for p in parts), ref.attempted)
    assert X.draw_uniform(3, 17, 5) != X.draw_uniform(3, 18, 5) and X.draw_uniform(3, 17, 5) != X.draw_uniform(3, 17, 6)


def test_new_entries_refuse_a_null_handle(amc):
    lib = amc.load()
    new = ["amc_set_ladder", "amc_exchange", "amc_sweep_exchange", "amc_exchange_counters", "amc_set_exchange_counters",
           "amc_get_exchange_step", "amc_set_exchange_step", "amc_histogram_rungs"]
    for name in new:
        assert name in amc.SIGNATURES
        res, args = amc.SIGNATURES[name]
        zeros = [None if (a is C.c_void_p or hasattr(a, "contents")) else a(0) for a in args]
        assert getattr(lib, name)(*zeros) == -1, name
        assert name.encode() in lib.amc_last_error()


# ---- run(): fuse=True and fuse=False issue the same sequence of sweeps and exchange steps -----------------------------------------
def _recording(calls):
    class Recording(X.TwinEngine):
        def sweep(self, n=1):                      # (sweep_reduce_begin and pgmc_steps come through here too)
            calls.extend("S" * int(n))
            super().sweep(n)

        def exchange(self, n=1):
            calls.extend("X" * int(n))
            super().exchange(n)

        def sweep_exchange(self, n, s=1):
            calls.append(("grouped", int(n), int(s)))
            super().sweep_exchange(n, s)           # (the twin calls self.sweep, recorded above, and its own exchange)

        def pg_estimate(self, *a, **k):
            calls.append("E")
            return super().pg_estimate(*a, **k)
    return Recording


def _flat(calls):
    """The sequence of sweeps (S), exchange steps (X) and estimator calls (E); a grouped call stands for n x (s sweeps, X), its sweeps
    were recorded by the twin's own calls to sweep()."""
    out, i = [], 0
    calls = list(calls)
    while i < len(calls):
        c = calls[i]
        if isinstance(c, tuple):
            _, n, s = c
            body = calls[i + 1:i + 1 + n * s]
            assert body == ["S"] * (n * s), body
            for _ in range(n):
                out.extend(["S"] * s + ["X"])
            i += 1 + n * s
        else:
            out.append(c)
            i += 1
    return out


def _rx_sim(path, factory, steps, every, extra):
    chains = ma.ParticleChains.ladder(6, [0.5, 1.0, 2.0], x=np.linspace(-1.5, 1.5, 18))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 0.7), ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.2], 0.3))
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=7, engine_factory=factory),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, every))]
    return ma.Simulation(chains, al + extra, steps, path=str(path))


@pytest.mark.parametrize("case", ["bare", "callbacks", "estimator"])
def test_fused_and_stepwise_runs_issue_the_same_steps(oracle, tmp_path, case):
    steps = 31
    extra = {"bare": [],
             "callbacks": [dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_energy, ma.callback_acceptance, ma.callback_exchange_acceptance),
                                scheduler=ma.build_schedule(steps, 0, 10))],
             "estimator": [dict(algorithm=ma.PolicyGradientEstimator, dependencies=(ma.Metropolis,), optimisers=(ma.Static(), ma.VPG(0.01)),
                                q_batch_size=2, scheduler=ma.build_schedule(steps, 0, 4)),
                           dict(algorithm=ma.PolicyGradientUpdate, dependencies=(ma.PolicyGradientEstimator,), scheduler=ma.build_schedule(steps, 0, 8))]}[case]
    out = []
    for i, fuse in enumerate((False, True)):
        calls = []
        sim = _rx_sim(tmp_path / str(i), _recording(calls), steps, 3, [dict(e) for e in extra])
        ma.run(sim, fuse=fuse)
        met = sim.algorithms[0]
        files = {f: open(tmp_path / str(i) / f).read() for f in ("energy.dat", "acceptance.dat", "exchange_acceptance.dat")} if case == "callbacks" else {}
        out.append((_flat(calls), [c for c in calls if isinstance(c, tuple)], sim.chains.x.copy(), met.engine.exchange_counters(),
                    met.engine.exchange_step, files, [m.sigma for m in met.pool]))
    (seq0, grouped0, x0, cnt0, tx0, files0, sig0), (seq1, grouped1, x1, cnt1, tx1, files1, sig1) = out
    assert seq0 == seq1
    assert [c for c in seq0 if c != "E"] == (["S"] * 3 + ["X"]) * 10 + ["S", "X"]       # build_schedule appends the last step
    assert grouped0 == [] and len(grouped1) > 0
    assert np.array_equal(x0.view(np.uint64), x1.view(np.uint64))
    assert np.array_equal(cnt0[0], cnt1[0]) and np.array_equal(cnt0[1], cnt1[1]) and tx0 == tx1 == 11
    assert files0 == files1 and sig0 == sig1
    if case == "bare":
        assert grouped1 == [("grouped", 10, 3)]          # then the lone last step: one sweep, one exchange


def test_exchange_every_step_is_one_call(oracle, tmp_path):
    calls = []
    sim = _rx_sim(tmp_path, _recording(calls), 12, 1, [])
    ma.run(sim)
    assert [c for c in calls if isinstance(c, tuple)] == [("grouped", 12, 1)]
    assert "ReplicaExchange\n\t\tCalls: 12\n\t\tRungs: 3\n\t\tLadders: 6\n" in open(tmp_path / "summary.log").read()
    assert ma.callback_exchange_acceptance(sim).shape == (2,)
    e = ma.rung_energy(sim)
    x = sim.chains.x.reshape(6, 3)
    assert np.allclose(e, (x * x).mean(axis=0), rtol=1e-15)


def test_checkpoint_carries_the_ladder(oracle, tmp_path):
    """Checkpoint after an odd number of exchange steps, restore, continue: the uninterrupted run, gap counters included; a
    checkpoint without a ladder restores as before."""
    def build(path, steps):
        return _rx_sim(path, X.TwinEngine, steps, 2, [])
    whole = build(tmp_path / "w", 12)
    ma.run(whole)
    first = build(tmp_path / "a", 6)
    ma.run(first)
    assert first.algorithms[0].engine.exchange_step == 3
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    second = build(tmp_path / "b", 6)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    e1, e2 = whole.algorithms[0].engine, second.algorithms[0].engine
    assert np.array_equal(whole.chains.x.view(np.uint64), second.chains.x.view(np.uint64))
    assert e1.exchange_step == e2.exchange_step == 6
    assert all(np.array_equal(a, b) for a, b in zip(e1.exchange_counters(), e2.exchange_counters()))
    assert int(np.load(tmp_path / "ck" / "checkpoint_rank0.npz")["n_rungs"]) == 3
    # a Metropolis without a ladder writes none of the new fields, and its checkpoint restores as before
    def plain(path, steps=5):
        chains = ma.ParticleChains(18, np.tile([0.5, 1.0, 2.0], 6), x=np.linspace(-1.5, 1.5, 18))
        pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
        return ma.Simulation(chains, [dict(algorithm=ma.Metropolis, pool=pool, seed=7, engine_factory=X.TwinEngine)], steps, path=str(path))
    a, b, c = plain(tmp_path / "p0", 10), plain(tmp_path / "p1"), plain(tmp_path / "p2")
    ma.run(a)
    ma.run(b)
    ma.checkpoint(b.algorithms[0], str(tmp_path / "ckp"))
    assert not {"n_rungs", "exchange_step", "exchange_accepted", "exchange_attempted"} & set(np.load(tmp_path / "ckp" / "checkpoint_rank0.npz").files)
    ma.restore(c.algorithms[0], str(tmp_path / "ckp"))
    ma.run(c)
    assert getattr(c.algorithms[0], "n_rungs", 0) == 0
    assert np.array_equal(a.chains.x.view(np.uint64), c.chains.x.view(np.uint64))


def test_a_shard_that_cuts_a_ladder_is_refused(oracle, tmp_path):
    chains = ma.ParticleChains(16, np.tile([1.0, 2.0], 8), x=np.zeros(16))
    al = [dict(algorithm=ma.Metropolis, pool=(ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),), engine_factory=X.TwinEngine),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), n_rungs=3)]
    sim = ma.Simulation(chains, al, 2, path=str(tmp_path))
    with pytest.raises(ValueError, match=r"R = 3 .*\[0, 16\) of 16"):
        ma.run(sim)
