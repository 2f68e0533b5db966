"""Convergence per group, the parts that need no GPU: the host formulas against a direct two-pass computation
on the full series, synthetic converged and dispersed ensembles, and ``Convergence`` over the engine doubles of
tests/chain_stats_twin.py -- the order of the samples, the refusals, the checkpoint section."""
import glob
import os

import numpy as np
import pytest

import montecarlo_amd as ma

import chain_stats_twin as T

M = 64


def records_of(series, G=1):
    """records[G][7][12] and (n, n) of series[2n][M]: the first n samples into part 0, the rest into part 1."""
    twin = T.ChainStatsTwin(series.shape[1], G)
    n = series.shape[0] // 2
    for s, o in enumerate(series):
        twin.accumulate("x", o, 0 if s < n else 1)
    return twin.records(), (n, n)


def two_pass(seqs):
    """(W, Bn, var_plus) of the sequences seqs[m][L], directly."""
    L = seqs.shape[1]
    w = np.mean(np.var(seqs, axis=1, ddof=1))
    bn = np.var(np.mean(seqs, axis=1), ddof=1)
    return w, bn, (L - 1) / L * w + bn


@pytest.mark.parametrize("n,N,G,mean", [(2, 3, 1, 0.0), (7, 5, 2, 3.0), (32, 64, 3, -5.0), (64, 16, 1, 1.0)])
def test_formulas_against_two_passes(oracle, n, N, G, mean):
    """Values O(1), <O>^2 / Var <= 100 (sd 0.5 at the least), n <= 64: the plain sums lose at most about 64 * 100 * 2^-52 = 1.4e-12,
    three decades below rtol 1e-9, which a wrong factor misses by far."""
    rng = np.random.default_rng(100 * n + N)
    series = mean + 0.5 * rng.standard_normal((2 * n, N * G)) + 0.3 * rng.standard_normal(N * G) + 0.05 * np.arange(2 * n)[:, None]
    rec, cnt = records_of(series, G)
    for split in (True, False):
        got = ma.variances_from_records(rec, cnt, N, split)
        rhat = ma.rhat_from_records(rec, cnt, N, split)
        for g in range(G):
            chains = series[:, g::G].T                          # [N][2n]
            seqs = np.concatenate([chains[:, :n], chains[:, n:]]) if split else chains
            w, bn, vp = two_pass(seqs)
            assert got[0][g] == pytest.approx(w, rel=1e-9) and got[1][g] == pytest.approx(bn, rel=1e-9) and got[2][g] == pytest.approx(vp, rel=1e-9)
            assert rhat[g] == pytest.approx(np.sqrt(vp / w), rel=1e-9)
            if split:
                assert ma.tau_batch_from_records(rec, cnt, N)[g] == pytest.approx(n * bn / (2 * vp), rel=1e-9)


def test_iid_series_are_converged(oracle):
    rng = np.random.default_rng(5)
    rec, cnt = records_of(rng.standard_normal((64, 4096)))
    for split in (True, False):
        assert abs(ma.rhat_from_records(rec, cnt, 4096, split)[0] - 1.0) < 0.01
    assert ma.tau_batch_from_records(rec, cnt, 4096)[0] == pytest.approx(0.5, abs=0.05)


def test_dispersed_ar1_chains_are_not(oracle):
    """Means +-1, innovation sd 0.1, phi = 0.9: the stationary sd within a chain is 0.23, the chains' means are 2 apart."""
    rng = np.random.default_rng(6)
    N, phi = 256, 0.9
    mu = np.where(np.arange(N) % 2, 1.0, -1.0)
    y = 0.1 / np.sqrt(1 - phi * phi) * rng.standard_normal(N)
    series = []
    for _ in range(64):
        y = phi * y + 0.1 * rng.standard_normal(N)
        series.append(mu + y)
    rec, cnt = records_of(np.array(series))
    for split in (True, False):
        assert ma.rhat_from_records(rec, cnt, N, split)[0] > 2.0


def test_unequal_counts_raise(oracle):
    rec, _ = records_of(np.random.default_rng(1).standard_normal((8, 16)))
    for fn in (ma.rhat_from_records, ma.variances_from_records, ma.tau_batch_from_records):
        with pytest.raises(ValueError, match="part 0 holds 4, part 1 holds 3"):
            fn(rec, (4, 3), 16)
        with pytest.raises(ValueError, match="part 0 holds 1, part 1 holds 1"):
            fn(rec, (1, 1), 16)


# ---- the algorithm over the engine doubles ---------------------------------------------------------------------------------------------
def build(path, steps, scheduler, n_samples=4, observable="x", extra=(), potential="double_well", factory=T.ChainStatsTwinEngine):
    chains = ma.ParticleChains.uniform(M, 1.0, potential=potential)
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.4], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=3, engine_factory=factory),
          dict(algorithm=ma.Convergence, dependencies=(ma.Metropolis,), scheduler=scheduler, observable=observable, n_samples=n_samples)]
    return ma.Simulation(chains, al + list(extra), steps, path=str(path))


def conv_of(sim):
    return next(a for a in sim.algorithms if isinstance(a, ma.Convergence))


@pytest.mark.parametrize("fuse", [True, False])
def test_the_halves_fill_in_order_and_later_calls_launch_nothing(oracle, amc, tmp_path, fuse):
    sim = build(tmp_path, 12, [2, 4, 6, 8, 10, 12])
    ma.run(sim, fuse=fuse)
    eng, cv = sim.algorithms[0].engine, conv_of(sim)
    assert eng.cs_calls == [("accumulate", 0, 2), ("accumulate", 0, 4), ("accumulate", 1, 6), ("accumulate", 1, 8)]
    assert cv.counts() == (2, 2) and cv.rhat().shape == cv.rhat(split=False).shape == cv.tau_int_batch().shape == (1,)
    assert all(v.shape == (1,) for v in cv.variances())
    assert np.array_equal(ma.callback_rhat(sim), cv.rhat())
    # a result is ONE fetch of the engine (the sums passes, the copy, the wait); the counts and a checkpoint's fields are none
    for call, fetches in ((cv.rhat, 1), (cv.variances, 1), (cv.tau_int_batch, 1), (lambda: ma.callback_rhat(sim), 1), (cv.counts, 0), (cv.state, 0)):
        before = eng.cs_fetches
        call()
        assert eng.cs_fetches - before == fetches, call
    cv.restart()
    assert cv.phase == 0 and eng.chain_stats_fetch()[2] == 0
    with pytest.raises(ValueError, match="nothing has been accumulated"):
        cv.rhat()


def test_rhat_while_the_halves_are_unequal_raises(oracle, amc, tmp_path):
    sim = build(tmp_path, 6, [2, 4, 6])
    ma.run(sim)
    with pytest.raises(ValueError, match="part 0 holds 2, part 1 holds 1"):
        conv_of(sim).rhat()
    assert np.isnan(ma.callback_rhat(sim)).all()


def test_the_reference_of_the_device_run_is_converged(oracle, amc, tmp_path):
    """tests/test_gpu_chain_stats_run.py asks |R-hat - 1| < 0.01 of 65 536 harmonic chains at beta = 2, sigma = 1, 200 sweeps of burn-in
    and 64 samples twenty sweeps apart: the same run on the twin engine at 4096 chains -- sixteen times fewer, so four times the noise
    -- stays within 0.005, so the bound on the device is a condition on the code and not a measurement."""
    chains = ma.ParticleChains(4096, 2.0, "harmonic", x=np.random.default_rng(11).uniform(-1.0, 1.0, 4096))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [1.0], 1.0),)
    sched = [200 + 20 * (k + 1) for k in range(64)]
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=9, engine_factory=T.ChainStatsTwinEngine),
          dict(algorithm=ma.Convergence, dependencies=(ma.Metropolis,), scheduler=sched, observable="x", n_samples=64)]
    sim = ma.Simulation(chains, al, sched[-1], path=str(tmp_path))
    ma.run(sim)
    r = conv_of(sim).rhat()[0]
    print("split R-hat of the twin run", r, "tau_int_batch", conv_of(sim).tau_int_batch()[0])
    assert abs(r - 1.0) < 0.005


def test_bad_arguments(oracle, amc, tmp_path):
    for kw, match in ((dict(observable="e"), "observable"), (dict(n_samples=5), "n_samples"), (dict(n_samples=2), "n_samples"),
                      (dict(n_samples=None), "n_samples")):
        with pytest.raises(ValueError, match=match):
            build(tmp_path, 4, [1, 2], **kw)


def test_an_anneal_inside_the_window_is_refused_at_initialise(oracle, amc, tmp_path):
    pa = lambda at: dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=at, betas=[1.5, 2.0, 2.5])
    sim = build(tmp_path / "a", 12, [2, 4, 6, 8], extra=[pa([5])])
    with pytest.raises(ValueError, match=r"annealing step at t = 5 .* first sample at t = 2 .* last sample at t = 8"):
        ma.run(sim)
    assert not hasattr(sim.algorithms[0].engine, "cs_calls")
    sim = build(tmp_path / "b", 12, [2, 4, 6, 8], extra=[pa([1, 8, 9])])      # outside, and behind the last sample at its own t
    ma.run(sim)
    assert len(sim.algorithms[0].engine.cs_calls) == 4


def ladder_sim(path, extra, tab=None):
    from test_tune_host import TuneEngine

    class Engine(T.ChainStatsSurface, TuneEngine):
        pass
    chains = ma.ParticleChains.ladder(4, [0.5, 1.0, 2.0], x=np.linspace(-1.5, 1.5, 12))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.4], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=7, engine_factory=Engine, rung_sigma=tab),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=[1, 3, 5, 7]),
          dict(algorithm=ma.Convergence, dependencies=(ma.Metropolis,), scheduler=[2, 4, 6, 8], observable="x", n_samples=4)]
    return ma.Simulation(chains, al + list(extra), 8, path=str(path))


def test_a_respacing_or_a_tuning_inside_the_window_is_refused_at_initialise(oracle, amc, tmp_path):
    rs = lambda at: dict(algorithm=ma.RespaceLadder, dependencies=(ma.ReplicaExchange,), scheduler=at, rule="acceptance")
    tn = lambda at: dict(algorithm=ma.TuneRungSigma, dependencies=(ma.Metropolis,), scheduler=at, target=0.5, min_calls=1)
    with pytest.raises(ValueError, match=r"respacing at t = 3 .* first sample at t = 2 .* last sample at t = 8"):
        ma.run(ladder_sim(tmp_path / "a", [rs([3])]))
    with pytest.raises(ValueError, match=r"tuning of the widths at t = 6 .* first sample at t = 2 .* last sample at t = 8"):
        ma.run(ladder_sim(tmp_path / "b", [tn([1, 6])], tab=[0.5, 0.4, 0.3]))
    sim = ladder_sim(tmp_path / "c", [tn([1])], tab=[0.5, 0.4, 0.3])          # in front of the window: allowed, one value per rung
    ma.run(sim)
    assert conv_of(sim).rhat().shape == (3,)


@pytest.mark.parametrize("cut", [1, 3, 5, 7])
def test_checkpoint_section_round_trip(oracle, amc, tmp_path, cut):
    """Stopped before the window, in its first half and in its second: the resumed run ends on the bits of the whole one."""
    sched = [2, 3, 4, 6, 7, 8]
    whole = build(tmp_path / "w", 9, sched, n_samples=6)
    ma.run(whole)
    first = build(tmp_path / "a", cut, [t for t in sched if t <= cut], n_samples=6)
    ma.run(first)
    ck = ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    d = np.load(ck)
    assert {"conv_observable", "conv_phase", "conv_n"} <= set(d.files) and ("conv_sums" in d.files) == (int(d["conv_phase"]) > 0)
    second = build(tmp_path / "b", 9 - cut, [t - cut for t in sched if t > cut], n_samples=6)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = conv_of(second), conv_of(whole)
    assert a.counts() == b.counts() == (3, 3)
    assert np.array_equal(a.records().view(np.uint64), b.records().view(np.uint64))
    assert np.array_equal(a.metropolis.engine.chain_stats_sums().view(np.uint64), b.metropolis.engine.chain_stats_sums().view(np.uint64))
    assert np.array_equal(a.rhat().view(np.uint64), b.rhat().view(np.uint64))


def test_checkpoints_without_the_section_load_as_before(oracle, amc, tmp_path):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "checkpoints")
    files = sorted(glob.glob(os.path.join(golden, "*.npz")))
    assert files
    for fn in files:
        assert not any(k.startswith("conv_") for k in np.load(fn).files), fn
    chains = ma.ParticleChains.uniform(M, 1.0, potential="double_well")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.4], 1.0),)
    plain = ma.Simulation(chains, [dict(algorithm=ma.Metropolis, pool=pool, seed=3, engine_factory=T.ChainStatsTwinEngine)], 4, path=str(tmp_path / "p"))
    ma.run(plain)
    ck = ma.checkpoint(plain.algorithms[0], str(tmp_path / "ck"))
    assert not any(k.startswith("conv_") for k in np.load(ck).files)
    sim = build(tmp_path / "s", 8, [1, 2, 3, 4])
    ma.restore(sim.algorithms[0], str(tmp_path / "ck"))
    ma.run(sim)
    assert [c[:2] for c in sim.algorithms[0].engine.cs_calls] == [("accumulate", 0), ("accumulate", 0), ("accumulate", 1), ("accumulate", 1)]


def test_the_handle_state_is_released_and_forgotten_where_the_slots_change():
    """ChainStatsState under the rules tests/test_handle_state_static.py holds the other grouped state to (sources only); the annealing
    step leaves the sums alone on purpose."""
    import re
    from test_handle_state_static import _braces, _code, _device_pointers, _read, _release_body
    pointers = _device_pointers("ChainStatsState")
    assert sorted(pointers) == ["d_stat_rows", "d_sums"]
    arg, text = _release_body("ChainStatsState", "chain_stats_release")
    assert sorted(re.findall(r"hipFree\(%s\.(\w+)\)" % arg, text)) == sorted(pointers)
    api = _code(_read("amc_api.hip"))
    assert "chain_stats_release(h->cstat);" in _braces(api, api.index("int amc_destroy(amc_handle* h)"))
    for unit, entry, forgets in (("amc_state.hip", "int amc_upload_state(", True), ("amc_state.hip", "int amc_init_uniform(", True),
                                 ("amc_exchange.hip", "static int ladder_reset(", True), ("amc_anneal.hip", "int amc_anneal(", False)):
        text = _code(_read(unit))
        assert ("chain_stats_forget(h);" in _braces(text, text.index(entry))) == forgets, entry


def test_null_handles_are_refused(amc):
    lib = amc.load()
    assert lib.amc_chain_stats_accumulate(None, 1, 0) == -1 and b"amc_chain_stats_accumulate" in lib.amc_last_error()
    assert lib.amc_chain_stats_fetch(None, None, 0, None, None, None) == -1 and lib.amc_chain_stats_download(None, None) == -1
    assert lib.amc_set_chain_stats(None, 0, None, None) == -1 and lib.amc_chain_stats_clear(None) == -1
