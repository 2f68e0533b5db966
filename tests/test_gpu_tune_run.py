"""TuneRungSigma in an algorithm list (montecarlo_amd/exchange.py): the stepwise and the fused run agree bit for bit, ``until`` is
respected, the summary block and the callback files are written, Metropolis.rung_sigma follows the device, a run interrupted by
checkpoint / restore in the middle of the burn-in continues bit for bit -- and the tuning does its job: on the harmonic well the
acceptance of every rung lands on the target."""
import os

import numpy as np
import pytest

import montecarlo_amd as ma

import tune_twin as TT
from test_gpu_exchange import bits, start_state

pytestmark = pytest.mark.gpu
R, L = 4, 129
BETAS = [0.6, 0.9, 1.5, 2.4]
TAB0 = [[0.05, 0.1, 0.9, 2.0]]


def build(path, steps, *, tune_at=(12, 24), until=None, store=True, tab=TAB0, tune=True):
    chains = ma.ParticleChains.ladder(L, BETAS, x=start_state(R, R * L)[0], potential="double_well")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=4, rung_sigma=tab),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,))]
    if tune:
        al.append(dict(algorithm=ma.TuneRungSigma, dependencies=(ma.Metropolis,), scheduler=[t for t in tune_at if t <= steps], target=0.44,
                       gamma=0.9, min_calls=100, sigma_min=1e-3, sigma_max=10.0, until=until))
    if store:
        al.append(dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_rung_sigma, ma.callback_rung_window_acceptance),
                       scheduler=ma.build_schedule(steps, 0, 6)))
    return ma.Simulation(chains, al, steps, path=str(path))


def state(sim):
    met = sim.algorithms[0]
    eng = met.engine
    st, n = eng.tune_status()
    return [bits(sim.chains.x), bits(eng.rung_sigma()), bits(met.rung_sigma), *eng.exchange_counters(), *eng.download_counters(),
            *eng.rung_window_base(), st, np.array([eng.exchange_step, eng.step, n])]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def test_fused_run_equals_stepwise_run(gpu, tmp_path):
    a, b = build(tmp_path / "stepwise", 36), build(tmp_path / "fused", 36)
    ma.run(a, fuse=False)
    ma.run(b, fuse=True)
    assert same(state(a), state(b))
    ta, tb = a.algorithms[2], b.algorithms[2]
    assert [t for t, _ in ta.statuses] == [12, 24] and all(np.all(s == 0) for _, s in ta.statuses)
    assert all(np.array_equal(u, v) for (_, u), (_, v) in zip(ta.statuses, tb.statuses))
    assert a.algorithms[0].engine.tune_status()[1] == 2 and not np.array_equal(a.algorithms[0].rung_sigma, TAB0)
    for name in ("rung_sigma.dat", "rung_window_acceptance.dat"):
        files = [open(os.path.join(str(tmp_path / d), name)).read() for d in ("stepwise", "fused")]
        assert files[0] == files[1] and len(files[0].splitlines()) >= 6
    text = open(tmp_path / "fused" / "summary.log").read()
    assert "TuneRungSigma\n\t\tCalls: 2\n\t\tTarget: 0.44\n\t\tGamma: 0.9\n\t\tMin calls: 100\n\t\tSigma min: 0.001\n\t\tSigma max: 10.0\n\t\tUntil: None" in text
    # the history the callback wrote: the table before the first tuning, behind it at the same t already, and at the end
    rows = dict(b.algorithms[3].rows[0])
    assert np.array_equal(rows[6], TAB0) and not np.array_equal(rows[12], TAB0) and np.array_equal(rows[12], rows[18])
    assert np.array_equal(bits(rows[36]), bits(b.algorithms[0].engine.rung_sigma()))
    wa = dict(b.algorithms[3].rows[1])
    assert np.all(np.isnan(wa[12])) and np.all((wa[18] > 0.0) & (wa[18] < 1.0))          # an empty window right behind a tuning


def test_until_is_respected(gpu, tmp_path):
    a = build(tmp_path / "a", 36, tune_at=(12, 24), until=20, store=False)
    b = build(tmp_path / "b", 36, tune_at=(12,), store=False)
    ma.run(a); ma.run(b)
    assert [t for t, _ in a.algorithms[2].statuses] == [12]
    assert same(state(a), state(b))


def test_checkpoint_restore_continue(gpu, tmp_path):
    whole = build(tmp_path / "w", 36, store=False)
    ma.run(whole)
    first = build(tmp_path / "a", 20, store=False)
    ma.run(first)
    met = first.algorithms[0]
    assert met.engine.tune_status()[1] == 1
    saved = np.load(ma.checkpoint(met, str(tmp_path / "ck")))
    assert int(saved["n_tuned"]) == 1 and np.array_equal(bits(saved["rung_sigma"]), bits(met.engine.rung_sigma()))
    assert np.array_equal(saved["rung_window_total"], met.engine.rung_window_base()[1]) and np.all(saved["rung_window_total"] == 12 * L)
    # the rest of the run: 16 steps, the second tuning at its step 4 (global 24), from whatever table the constructor was given
    second = build(tmp_path / "b", 16, tune_at=(4,), store=False, tab=[[0.3] * R])
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    assert same(state(whole), state(second))
    # no tuning, no restart: no new field
    plain = build(tmp_path / "p", 8, store=False, tune=False)
    ma.run(plain)
    fields = np.load(ma.checkpoint(plain.algorithms[0], str(tmp_path / "ck2"))).files
    assert "rung_sigma" in fields and not {"n_tuned", "rung_window_accepted", "rung_window_total"} & set(fields)


# ---- the tuning does its job ------------------------------------------------------------------------------------------------------------
ST_R, ST_L, ST_TARGET, ST_TUNINGS, ST_WINDOW = 4, 4096, 0.5, 12, 50
ST_BETAS = 0.5 * 2.0 ** np.arange(ST_R)
ST_SIGMA0 = 0.05


def noise_free_map():
    """The map iterated on the host from the same start with the closed-form acceptance: sigma after the tunings, per rung."""
    s = np.full(ST_R, ST_SIGMA0)
    n = 10 ** 15
    for _ in range(ST_TUNINGS):
        a = TT.harmonic_acceptance(s, ST_BETAS)
        s = np.array([TT.tune_rule(s[r], round(float(a[r]) * n), n, ST_TARGET, 1.0, 1)[1] for r in range(ST_R)])
    return s


def test_the_tuned_acceptance_lands_on_the_target(gpu):
    """Harmonic well, R = 4 geometric beta, 4096 ladders in equilibrium, sigma_0 = 0.05 everywhere, target 0.5: 12 tunings with windows
    of 50 sweeps, then one untouched window of 50 sweeps.  se = sqrt(0.25 / n), n = 50 x 4096 calls per rung, = 0.0011.
    Required per rung: |a_window - target| <= |a(sigma_map) - target| + 10 se, sigma_map the noise-free map's width after 12 steps --
    5 se for the last window's binomial error, 5 se for the noise of the earlier windows, which the contraction (g' = 0.363 at
    a = 0.5) damps by 1 / (1 - 0.37).  The map alone must be inside 1 se (checked first, on the host).  And sigma_r sqrt(beta_r) must be
    equal across rungs within the relative spread 10 se of acceptance implies through da / dsigma of the closed form."""
    n = ST_WINDOW * ST_L
    se = np.sqrt(0.25 / n)
    s_map = noise_free_map()
    a_map = TT.harmonic_acceptance(s_map, ST_BETAS)
    print("map: sigma", s_map, "acceptance", a_map, "se", se)
    assert np.all(np.abs(a_map - ST_TARGET) <= se)                       # (if not: more tunings, not a wider margin)
    M = ST_R * ST_L
    rng = np.random.default_rng(12)
    beta = np.tile(ST_BETAS, ST_L)
    x = rng.standard_normal(M) / np.sqrt(2.0 * beta)                      # equilibrium of exp(-beta x^2)
    eng = gpu.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=77, per_chain_counters=True)
    eng.upload_state(x, beta)
    eng.set_ladder(ST_R)
    eng.set_rung_sigma(np.full((1, ST_R), ST_SIGMA0))
    for _ in range(ST_TUNINGS):
        eng.sweep(ST_WINDOW)
        eng.tune_rung_sigma(ST_TARGET, 1.0, 1000, 1e-100, 1e100)
    st, n_tuned = eng.tune_status()
    assert np.all(st == 0) and n_tuned == ST_TUNINGS
    eng.sweep(ST_WINDOW)
    acc, tot = eng.rung_window_counts()
    sigma = eng.rung_sigma()[0]
    eng.close()
    assert np.all(tot == n)
    a = acc[0] / tot[0]
    print("device: sigma", sigma, "window acceptance", a, "bound", np.abs(a_map - ST_TARGET) + 10 * se)
    assert np.all(np.abs(a - ST_TARGET) <= np.abs(a_map - ST_TARGET) + 10 * se)
    c = np.sqrt(2.0 / ST_BETAS)
    slope = (2.0 / np.pi) * c / (s_map ** 2 + c ** 2)                     # |da / dsigma| of the closed form at sigma_map
    rel = 10 * se / (s_map * slope)
    scaled = sigma * np.sqrt(ST_BETAS)
    print("sigma sqrt(beta)", scaled, "relative spread allowed", rel)
    assert np.all(np.abs(scaled / scaled.mean() - 1.0) <= rel.max())
