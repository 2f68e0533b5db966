"""``Autocorrelation`` over an engine double that records its calls (corr_twin.CorrTwinEngine): the order of marks and samples,
repeat origins, the refusals, and the checkpoint section.  No GPU."""
import glob
import os

import numpy as np
import pytest

import montecarlo_amd as ma

import corr_twin as T

M = 64


def build(path, steps, scheduler, n_lags, origins=1, observable="energy", anneal_at=None, anneal_first=False, potential="harmonic"):
    chains = ma.ParticleChains.uniform(M, 1.0, potential=potential)
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.4], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=3, engine_factory=T.CorrTwinEngine)]
    ac = dict(algorithm=ma.Autocorrelation, dependencies=(ma.Metropolis,), scheduler=scheduler, observable=observable, n_lags=n_lags,
              origins=origins)
    pa = None if anneal_at is None else dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=anneal_at,
                                             betas=[1.5, 2.0, 2.5])
    al += [x for x in ((pa, ac) if anneal_first else (ac, pa)) if x is not None]
    return ma.Simulation(chains, al, steps, path=str(path))


def corr_of(sim):
    return next(a for a in sim.algorithms if isinstance(a, ma.Autocorrelation))


@pytest.mark.parametrize("fuse", [True, False])
def test_mark_then_samples_at_the_scheduled_steps(oracle, amc, tmp_path, fuse):
    sim = build(tmp_path, 12, [2, 4, 6, 8, 10], n_lags=3)
    ma.run(sim, fuse=fuse)
    eng, ac = sim.algorithms[0].engine, corr_of(sim)
    assert eng.calls == [("mark", 2), ("sample", 4), ("sample", 6), ("sample", 8)]       # the fifth call: every origin is taken
    assert np.array_equal(ac.lags(), [0, 2, 4, 6])
    rec = ac.records()
    assert rec.shape == (4, 1, 3, T.WORDS)
    rho = ac.rho()
    assert rho.shape == (1, 4) and rho[0, 0] == pytest.approx(1.0, abs=1e-12)
    tau, window, converged = ac.tau_int()
    assert tau.shape == window.shape == converged.shape == (1,)
    assert np.array_equal(ma.callback_rho(sim), rho[:, -1]) and np.array_equal(ma.callback_tau_int(sim), tau)


def test_fused_and_stepwise_runs_hold_the_same_records(oracle, amc, tmp_path):
    recs = []
    for fuse in (True, False):
        sim = build(tmp_path / str(fuse), 12, [2, 4, 6, 8], n_lags=3, observable="x", potential="double_well")
        ma.run(sim, fuse=fuse)
        recs.append(corr_of(sim).records())
    assert np.array_equal(recs[0].view(np.uint64), recs[1].view(np.uint64))


def test_repeat_origins_merge_slot_by_slot(oracle, amc, tmp_path):
    sim = build(tmp_path, 12, [1, 2, 3, 5, 6, 7], n_lags=2, origins=2)
    ma.run(sim)
    eng, ac = sim.algorithms[0].engine, corr_of(sim)
    assert [c for c in eng.calls if c[0] != "fetch"] == [("mark", 1), ("sample", 2), ("sample", 3), ("mark", 5), ("sample", 6), ("sample", 7)]
    assert ("fetch", 5) in eng.calls
    second = eng.corr_fetch()[0]
    rec = ac.records()
    assert ac.origins_done == 2 and ac.n_per_group() == 2 * M and np.array_equal(ac.lags(), [0, 1, 2])
    # the accumulator is the first origin's records merged with the second's: taking the second away leaves a record that rounds to
    # the first origin's sums, and slot 0's O column is sum a over both origins
    first = T.values(rec) - T.values(second)
    assert np.all(np.isfinite(first)) and T.values(rec)[0, 0, 1] > T.values(second)[0, 0, 1] > 0.0
    assert np.array_equal(rec.view(np.uint64), T.merge([ac._acc]).view(np.uint64))


def test_a_repeat_origin_with_other_lag_steps_is_refused(oracle, amc, tmp_path):
    sim = build(tmp_path, 12, [1, 2, 3, 5, 6, 8], n_lags=2, origins=2)
    ma.run(sim)
    with pytest.raises(ValueError, match="same pattern"):
        corr_of(sim).records()


def test_unequal_lag_steps_refuse_tau_int(oracle, amc, tmp_path):
    sim = build(tmp_path, 12, [1, 2, 4, 5], n_lags=3)
    ma.run(sim)
    ac = corr_of(sim)
    assert np.array_equal(ac.lags(), [0, 1, 3, 4]) and ac.rho().shape == (1, 4)
    with pytest.raises(ValueError, match="not equally spaced"):
        ac.tau_int()


def test_an_anneal_between_mark_and_sample_is_refused_at_initialise(oracle, amc, tmp_path):
    sim = build(tmp_path / "a", 12, [2, 4, 6], n_lags=2, anneal_at=[5])
    with pytest.raises(ValueError, match=r"annealing step at t = 5 .* mark at t = 2 .* sample at t = 6"):
        ma.run(sim)
    assert sim.algorithms[0].engine.calls == []
    # same t as the sample: listed in front of the Autocorrelation the anneal comes first and falls between ...
    sim = build(tmp_path / "b", 12, [2, 4, 6], n_lags=2, anneal_at=[6], anneal_first=True)
    with pytest.raises(ValueError, match="t = 6"):
        ma.run(sim)
    # ... listed behind it, and everywhere outside the origin, it is allowed
    sim = build(tmp_path / "c", 12, [2, 4, 6], n_lags=2, anneal_at=[1, 6, 9])
    ma.run(sim)
    assert [c[0] for c in sim.algorithms[0].engine.calls] == ["mark", "sample", "sample"]


def test_bad_arguments(oracle, amc, tmp_path):
    for kw, match in ((dict(observable="e"), "observable"), (dict(n_lags=0), "n_lags"), (dict(n_lags=256), "n_lags"), (dict(origins=0), "origins")):
        args = dict(scheduler=[1, 2], n_lags=1)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            build(tmp_path, 4, **args)


@pytest.mark.parametrize("cut", [3, 5, 8])
def test_checkpoint_section_round_trip(oracle, amc, tmp_path, cut):
    """Stopped in the middle of the first origin, between the origins and in the middle of the second: the resumed run ends on the
    bits of the whole one."""
    sched = [1, 2, 3, 4, 6, 7, 8, 9]
    whole = build(tmp_path / "w", 10, sched, n_lags=3, origins=2)
    ma.run(whole)
    first = build(tmp_path / "a", cut, [t for t in sched if t <= cut], n_lags=3, origins=2)
    ma.run(first)
    ck = ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    d = np.load(ck)
    assert {"corr_observable", "corr_phase", "corr_origins_done"} <= set(d.files)
    assert ("corr_origin" in d.files) == (int(d["corr_phase"]) >= 0) and ("corr_acc" in d.files) == (int(d["corr_origins_done"]) > 0)
    second = build(tmp_path / "b", 10 - cut, [t - cut for t in sched if t > cut], n_lags=3, origins=2)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = corr_of(second), corr_of(whole)
    assert np.array_equal(a.records().view(np.uint64), b.records().view(np.uint64)) and np.array_equal(a.lags(), b.lags())
    assert a.origins_done == b.origins_done == 2


def test_checkpoints_without_the_section_load_as_before(oracle, amc, tmp_path):
    """Every committed checkpoint lacks the section; a run without an Autocorrelation writes none."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "checkpoints")
    files = sorted(glob.glob(os.path.join(golden, "*.npz")))
    assert files
    for fn in files:
        assert not any(k.startswith("corr_") for k in np.load(fn).files), fn
    chains = ma.ParticleChains.uniform(M, 1.0)
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.4], 1.0),)
    plain = ma.Simulation(chains, [dict(algorithm=ma.Metropolis, pool=pool, seed=3, engine_factory=T.CorrTwinEngine)], 4, path=str(tmp_path / "p"))
    ma.run(plain)
    ck = ma.checkpoint(plain.algorithms[0], str(tmp_path / "ck"))
    assert not any(k.startswith("corr_") for k in np.load(ck).files)
    # ... and a run WITH an Autocorrelation restores from it: nothing is marked
    sim = build(tmp_path / "s", 4, [1, 2, 3], n_lags=2)
    ma.restore(sim.algorithms[0], str(tmp_path / "ck"))
    ma.run(sim)
    assert [c[0] for c in sim.algorithms[0].engine.calls] == ["mark", "sample", "sample"]
