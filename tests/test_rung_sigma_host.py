"""Proposal widths per rung, the parts that need no GPU: the validations of Metropolis(..., rung_sigma=...) (each a ValueError raised
before an engine is made), the host twin (tests/rung_sigma_twin.py) against hand-strided OracleSim runs, the checkpoint field and the
acceptance reads through an engine double, and the statistical run of the twin."""
import re

import numpy as np
import pytest

import montecarlo_amd as ma

import exchange_twin as X
import oracle_lib as O
import rung_sigma_twin as RT


def no_engine(**kw):
    raise AssertionError("the validation comes before the engine is made")


def gauss_pool(K=1):
    return tuple(ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5 / (k + 1)], 1.0 / K) for k in range(K))


def make(rung_sigma, pool=None, **kw):
    ch = ma.ParticleChains.uniform(32, 2.0)
    return ma.Metropolis(ch, pool=pool or gauss_pool(), engine_factory=no_engine, rung_sigma=rung_sigma, **kw)


@pytest.mark.parametrize("bad,words", [
    ([[0.5, 0.4], [0.3, 0.2]], "shape"),                    # K = 1 pool, two rows
    ([0.5], "shape"),                                       # one rung
    ([0.5, 0.0, 0.2], "rung_sigma[0][1]"),
    ([0.5, float("nan")], "rung_sigma[0][1]"),
    ([0.5, 1e101], "rung_sigma[0][1]"),
    ([0.5, -0.1], "rung_sigma[0][1]"),
    ([0.1] * 65, "65"),
])
def test_rung_sigma_is_validated_before_an_engine_is_made(bad, words):
    with pytest.raises(ValueError, match=re.escape(words)):
        make(bad)


def test_rung_sigma_limits_name_the_numbers():
    with pytest.raises(ValueError, match="5 x 13 = 65"):
        make(np.full((5, 13), 0.3), pool=gauss_pool(5))
    with pytest.raises(ValueError, match="streams = 2"):
        make([0.5, 0.4], streams=2)
    f32 = (ma.Move(ma.Displacement(), ma.StandardGaussian(), np.array([0.5], dtype=np.float32), 1.0),)
    with pytest.raises(ValueError, match="Float64 parameters"):
        make([0.5, 0.4], pool=f32)
    scaled = (ma.Move(ma.Displacement(), ma.ScaledGaussian("1.0 + x*x"), [0.5], 1.0),)
    with pytest.raises(ValueError, match="built-in Gaussian"):
        make([0.5, 0.4], pool=scaled)


def test_twin_is_the_hand_strided_pair_of_oracle_runs():
    R, L, seed = 2, 5, 19
    M = R * L
    sig = np.array([[0.5, 0.3], [0.25, 0.1]])
    w = [0.625, 0.375]
    x0 = 1.3 * np.sin(0.7 * np.arange(M))
    beta = np.array([0.5, 2.0])[np.arange(M) % R]
    tw = RT.RungSigmaTwin(M, sig, weight=w, seed=seed, beta=1.0)
    tw.set_beta(beta); tw.set_x(x0)
    tw.make_steps(3)
    tw.make_steps(2)
    runs = []
    for r in range(R):
        s = O.OracleSim(M, sigma=list(sig[:, r]), weight=w, seed=seed, beta=1.0)
        s.set_beta(beta); s.set_x(x0)
        s.make_steps(5)
        runs.append((s.state(), s.counters()))
    x, e = tw.state()
    acc, tot = tw.counters()
    for c in range(M):
        (xr, er), (ar, tr) = runs[c % R]
        assert x[c].tobytes() == xr[c].tobytes() and e[c].tobytes() == er[c].tobytes()
        assert np.array_equal(acc[:, c], ar[:, c]) and np.array_equal(tot[:, c], tr[:, c])
    assert tw.step == 5 and tot.sum(axis=0).tolist() == [5] * M


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
def test_the_exchange_step_over_arrays_is_the_twins(potential):
    """ArrayExchangeTwin (the statistical run's exchange step) against exchange_twin.ExchangeTwin: positions, gap counters and step
    index, over both parities, odd R and a chain offset."""
    R, L, seed, offset = 5, 40, (7 << 32) | 11, 35
    M = R * L
    tab = [0.6, 0.5, 0.4, 0.3, 0.2]
    x0 = 1.4 * np.sin(0.9 * np.arange(M) + 0.1)
    beta = (0.5 * 1.7 ** np.arange(R))[np.arange(M) % R]
    twins = []
    for cls in (X.ExchangeTwin, RT.ArrayExchangeTwin):
        sim = RT.RungSigmaTwin(M, tab, chain_offset=offset, potential=potential, beta=1.0, seed=seed)
        sim.set_beta(beta); sim.set_x(x0)
        tw = cls(sim, beta, R, seed=seed, potential=potential, chain_offset=offset)
        tw.sweep(2); tw.exchange(3); tw.sweep_exchange(4, 1)
        twins.append(tw)
    a, b = twins
    assert np.array_equal(a.sim.state()[0].view(np.uint64), b.sim.state()[0].view(np.uint64))
    assert np.array_equal(a.accepted, b.accepted) and np.array_equal(a.attempted, b.attempted) and a.t_x == b.t_x == 7
    assert 0 < a.accepted.sum() < a.attempted.sum()


def test_harmonic_ladder_with_widths_per_rung_samples_every_rung_on_the_twin():
    """The configuration of the GPU test (tests/test_gpu_rung_sigma.py) on the host twin: R = 4, beta_r = 0.5 2^r,
    sigma_r = 0.8 / sqrt(beta_r), 4096 ladders, 300 rounds of [1 sweep; 1 exchange] after 300 of burn-in.  The mean over the rounds of
    <x^2>_r lies within six standard errors of ONE snapshot of independent ladders, 6 sqrt(2 / 4096) / (2 beta_r), of 1 / (2 beta_r),
    and every acceptance of the move lies in (0.2, 0.8): the band and the burn-in hold without any kernel."""
    R, L, seed = 4, 4096, 5
    M = R * L
    betas = 0.5 * 2.0 ** np.arange(R)
    beta = np.tile(betas, L)
    sim = RT.RungSigmaTwin(M, 0.8 / np.sqrt(betas), potential="harmonic", beta=1.0, seed=seed, threads=min(4, O.load().amo_max_threads()))
    sim.set_beta(beta)
    sim.set_x(np.zeros(M))
    for s in sim.sims:
        s.init_uniform(-1.0, 1.0)
    sim.set_x(sim.sims[0].state()[0])
    tw = RT.ArrayExchangeTwin(sim, beta, R, seed=seed, potential="harmonic")
    tw.sweep_exchange(300, 1)
    xx = np.zeros(R)
    for _ in range(300):
        tw.sweep_exchange(1, 1)
        x = sim.state()[0].reshape(L, R)
        xx += (x * x).mean(axis=0)
    xx /= 300
    acc, tot = sim.counters()
    ratio = acc[0].reshape(L, R).sum(axis=0) / tot[0].reshape(L, R).sum(axis=0)
    print("x^2 per rung", xx, "expected", 1 / (2 * betas), "acceptance", ratio, "swaps", tw.accepted / tw.attempted)
    assert np.all(np.abs(xx - 1 / (2 * betas)) <= 6 * np.sqrt(2 / L) / (2 * betas))
    assert np.all((ratio > 0.2) & (ratio < 0.8))
    assert tot.sum() == 600 * M and tw.t_x == 600


class TableEngine(X.TwinEngine):
    """TwinEngine with the table's entries of HipEngine.  A double of the HOST logic only: it keeps the table it is handed and
    forgets it with the ladder, as amc_set_ladder does; its sweeps go on with the pool's sigma."""

    table = None

    def set_ladder(self, n_rungs):
        super().set_ladder(n_rungs)
        self.table = None

    def set_rung_sigma(self, sigma):
        self.table = None if sigma is None else np.array(sigma, dtype=np.float64).reshape(self.n_moves, self.n_rungs)

    def rung_sigma(self):
        assert self.table is not None
        return self.table.copy()

    def rung_counter_totals(self):
        acc, tot = self.download_counters()
        return (acc.reshape(self.n_moves, -1, self.n_rungs).sum(axis=1), tot.reshape(self.n_moves, -1, self.n_rungs).sum(axis=1))


TAB = np.array([[0.5, 0.4, 0.3], [0.2, 0.15, 0.1]])


def _rx_sim(path, steps, tab):
    chains = ma.ParticleChains.ladder(6, [0.5, 1.0, 2.0], x=np.linspace(-1.5, 1.5, 18))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 0.625), ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.2], 0.375))
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=7, engine_factory=TableEngine, rung_sigma=tab),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2))]
    return ma.Simulation(chains, al, steps, path=str(path))


def _fields(path):
    return np.load(path / "checkpoint_rank0.npz")


def test_checkpoint_has_the_field_only_when_a_table_is_set(oracle, tmp_path):
    with_tab, plain = _rx_sim(tmp_path / "a", 6, TAB), _rx_sim(tmp_path / "b", 6, None)
    for sim, name in ((with_tab, "ck"), (plain, "ckp")):
        ma.run(sim)
        ma.checkpoint(sim.algorithms[0], str(tmp_path / name))
    assert with_tab.algorithms[0].engine.per_chain_counters and np.array_equal(with_tab.algorithms[0].engine.table, TAB)
    assert np.array_equal(_fields(tmp_path / "ck")["rung_sigma"], TAB)
    assert "rung_sigma" not in _fields(tmp_path / "ckp").files
    assert set(_fields(tmp_path / "ck").files) - set(_fields(tmp_path / "ckp").files) == {"rung_sigma"}


def test_restore_hands_the_checkpoints_table_to_the_engine(oracle, tmp_path):
    """Whatever table the restored Metropolis was built with, and whether or not its ladder is set already, the engine ends with
    the checkpoint's table -- or none -- and so does the next checkpoint."""
    for name, tab in (("ck", TAB), ("ckp", None)):
        sim = _rx_sim(tmp_path / name, 4, tab)
        ma.run(sim)
        ma.checkpoint(sim.algorithms[0], str(tmp_path / name))
    other = TAB * 0.5
    for built_with in (TAB, other, None):
        for ladder_first in (False, True):
            for name, saved in (("ck", TAB), ("ckp", None)):
                sim = _rx_sim(tmp_path / "r", 4, built_with)
                met = sim.algorithms[0]
                if ladder_first:
                    met.initialise(sim)                # (the per-chain beta array goes up with the state)
                    met.set_ladder(3)                  # the engine now holds the constructor's table
                    assert (met.engine.table is None) == (built_with is None)
                ma.restore(met, str(tmp_path / name))
                for got in (met.engine.table, met.rung_sigma):
                    assert (got is None) if saved is None else np.array_equal(got, saved)
                ma.checkpoint(met, str(tmp_path / "again"))
                again = _fields(tmp_path / "again")
                assert ("rung_sigma" not in again.files) if saved is None else np.array_equal(again["rung_sigma"], saved)


@pytest.mark.parametrize("bad,words", [(np.ones((2, 4)) * 0.3, "4 rungs per move for a ladder of R = 3"), (np.ones((3, 3)) * 0.3, "shape (3, 3)"),
                                       (np.array([[0.5, 0.4, 0.3], [0.2, 0.0, 0.1]]), "rung_sigma[1][1]")])
def test_restore_checks_the_tables_shape_and_values(oracle, tmp_path, bad, words):
    sim = _rx_sim(tmp_path / "a", 4, TAB)
    ma.run(sim)
    ma.checkpoint(sim.algorithms[0], str(tmp_path / "ck"))
    d = dict(_fields(tmp_path / "ck"))
    d["rung_sigma"] = bad
    np.savez(tmp_path / "ck" / "checkpoint_rank0.npz", **d)
    with pytest.raises(ValueError, match=re.escape(words)):
        ma.restore(_rx_sim(tmp_path / "b", 4, TAB).algorithms[0], str(tmp_path / "ck"))


def test_rung_acceptance_and_its_callback_divide_the_integer_totals(oracle, tmp_path):
    sim = _rx_sim(tmp_path, 12, TAB)
    met = sim.algorithms[0]
    with pytest.raises(ValueError, match="no ladder"):
        met.rung_acceptance()
    ma.run(sim)
    acc, tot = met.engine.download_counters()
    want = acc.reshape(2, 6, 3).sum(axis=1) / tot.reshape(2, 6, 3).sum(axis=1)
    got = met.rung_acceptance()
    assert got.shape == (2, 3) and np.array_equal(got, want) and tot.sum() == 12 * 18
    assert np.array_equal(ma.callback_rung_acceptance(sim), want)
    # 0 / 0 is NaN: a move that was never picked at a rung
    met.engine.upload_counters(np.zeros_like(acc), np.where(np.arange(18) % 3 == 1, 0, tot))
    got = met.rung_acceptance()
    assert np.all(np.isnan(got[:, 1])) and np.all(got[:, [0, 2]] == 0.0)
