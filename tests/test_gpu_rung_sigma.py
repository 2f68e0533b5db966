"""Proposal widths per rung on the device (DESIGN.md section 3.13 "Widths per rung"; include/amc.h amc_set_rung_sigma,
amc_rung_counter_totals) against the host twin (tests/rung_sigma_twin.py inside tests/exchange_twin.py), bit for bit: positions,
energies, per-chain Move counters, gap counters, step indices."""
import numpy as np
import pytest

from montecarlo_amd.system import CustomPotential

import exchange_twin as X
import oracle_lib as O
import rung_sigma_twin as RT

pytestmark = pytest.mark.gpu
CUSTOM = "x*x*x*x - 2.0*x*x + 0.25*x"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pool(K):
    sigma = [0.5 / (1.0 + 0.37 * k) for k in range(K)]
    w = np.arange(K, 0, -1, dtype=np.float64)
    w = w / 2.0 ** np.ceil(np.log2(w.sum()))               # dyadic weights ...
    w[0] += 1.0 - w.sum()                                  # ... that sum to 1 exactly
    return sigma, [float(v) for v in w]


def table(K, R):
    """sigma[k][r] = sigma_k 1.3^-r: no two entries equal."""
    sigma, _ = pool(K)
    return np.array([[s * 1.3 ** (-r) for r in range(R)] for s in sigma])


def start_state(R, M, offset=0):
    ids = np.arange(offset, offset + M)
    x = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)
    return x, (0.5 * 1.5 ** np.arange(R))[ids % R]


def make_engine(gpu, R, L, K, *, potential="harmonic", dtype="f64", offset=0, n_global=None, seed=23, sweepstep=1, tab=None, ladder=True):
    M = R * L
    sigma, weight = pool(K)
    x, beta = start_state(R, M, offset)
    eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=n_global or offset + M, potential=potential, beta=1.0,
                        sigma=sigma, weight=weight, seed=seed, per_chain_counters=True, dtype=dtype, sweepstep=sweepstep)
    eng.upload_state(x, beta)
    if ladder:
        eng.set_ladder(R)
    if tab is not None:
        eng.set_rung_sigma(tab)
    return eng


def make_twin(R, L, K, tab, *, potential="harmonic", dtype="f64", offset=0, seed=23, sweepstep=1):
    M = R * L
    _, weight = pool(K)
    x, beta = start_state(R, M, offset)
    sim = RT.RungSigmaTwin(M, tab, chain_offset=offset, potential=potential, beta=1.0, weight=weight, seed=seed, dtype=dtype, sweepstep=sweepstep)
    sim.set_beta(beta)
    tw = X.ExchangeTwin(sim, beta, R, seed=seed, potential=potential, chain_offset=offset, f32=dtype == "f32")
    tw.state.put(x.astype(np.float32).astype(np.float64) if dtype == "f32" else x, tw.pot)
    return tw


def compare(eng, tw):
    x, e = eng.download_state()
    xo, eo = tw.sim.state()
    assert np.array_equal(bits(x), bits(xo)), "positions differ from the twin"
    assert np.array_equal(bits(e), bits(eo)), "energies differ from the twin"
    acc, tot = eng.download_counters()
    ao, to = tw.sim.counters()
    assert np.array_equal(acc, ao) and np.array_equal(tot, to), "Move counters differ from the twin"
    ga, gt = eng.exchange_counters()
    assert np.array_equal(ga, tw.accepted) and np.array_equal(gt, tw.attempted), "gap counters differ from the twin"
    assert eng.exchange_step == tw.t_x and eng.step == tw.sim.step


def interleave(eng, tw):
    for obj in (eng, tw):
        obj.sweep(1); obj.exchange(1); obj.sweep(3); obj.exchange(2)
    compare(eng, tw)
    for obj in (eng, tw):
        obj.sweep_exchange(4, 2)
    compare(eng, tw)


def check_rung_totals(eng, R):
    acc, tot = eng.download_counters()
    ra, rt = eng.rung_counter_totals()
    for r in range(R):
        assert np.array_equal(ra[:, r], acc[:, r::R].sum(axis=1)) and np.array_equal(rt[:, r], tot[:, r::R].sum(axis=1)), r
    ta, tt = eng.counter_totals()
    assert np.array_equal(ra.sum(axis=1), ta) and np.array_equal(rt.sum(axis=1), tt)


@pytest.mark.parametrize("R,L,K", [(2, 1, 2), (3, 171, 2), (4, 129, 2), (6, 171, 2), (64, 9, 1), (7, 37, 9)])
def test_rung_widths_match_the_twin(gpu, R, L, K):
    tab = table(K, R)
    eng, tw = make_engine(gpu, R, L, K, tab=tab), make_twin(R, L, K, tab)
    assert np.array_equal(eng.rung_sigma(), tab)
    interleave(eng, tw)
    check_rung_totals(eng, R)
    eng.close()


@pytest.mark.parametrize("kw", [dict(potential="double_well"), dict(potential=CustomPotential(CUSTOM)), dict(dtype="f32"), dict(sweepstep=3)],
                         ids=["double_well", "custom", "f32", "sweepstep3"])
def test_rung_widths_in_the_other_forms(gpu, kw):
    R, L, K = 3, 171, 2
    tab = table(K, R)
    eng, tw = make_engine(gpu, R, L, K, tab=tab, **kw), make_twin(R, L, K, tab, **kw)
    interleave(eng, tw)
    eng.close()


def test_a_grid_walked_more_than_once(gpu, monkeypatch):
    """One block per CU: several trips per block, a ragged last one, and with odd R the rung of a lane changes between trips."""
    monkeypatch.setenv("AMC_BLOCKS_PER_CU", "1")
    R, L, K = 3, 60002, 2
    tab = table(K, R)
    eng, tw = make_engine(gpu, R, L, K, tab=tab), make_twin(R, L, K, tab)
    for obj in (eng, tw):
        obj.sweep(3)
    compare(eng, tw)
    check_rung_totals(eng, R)
    eng.close()


def test_shards_equal_the_whole(gpu):
    R, L, K = 3, 171, 2
    tab = table(K, R)
    whole = make_engine(gpu, R, L, K, tab=tab)
    parts = [make_engine(gpu, R, 86, K, tab=tab, offset=0, n_global=R * L), make_engine(gpu, R, L - 86, K, tab=tab, offset=R * 86, n_global=R * L)]
    for e in [whole] + parts:
        e.sweep(1); e.exchange(1); e.sweep(3); e.exchange(2); e.sweep_exchange(4, 2)
    x = np.concatenate([p.download_state()[0] for p in parts])
    assert np.array_equal(bits(x), bits(whole.download_state()[0]))
    for i in range(2):
        assert np.array_equal(np.concatenate([p.download_counters()[i] for p in parts], axis=1), whole.download_counters()[i])
        assert np.array_equal(sum(p.rung_counter_totals()[i] for p in parts), whole.rung_counter_totals()[i])
    for e in [whole] + parts:
        e.close()


def test_equal_table_and_clearing_give_the_plain_bits(gpu):
    R, L, K = 3, 171, 2
    sigma, _ = pool(K)
    flat = np.repeat(np.array(sigma)[:, None], R, axis=1)
    a, b, c = make_engine(gpu, R, L, K), make_engine(gpu, R, L, K, tab=flat), make_engine(gpu, R, L, K, tab=table(K, R))
    for e in (a, b, c):
        e.sweep(2); e.exchange(1); e.sweep(1)
    assert np.array_equal(bits(a.download_state()[0]), bits(b.download_state()[0]))
    assert all(np.array_equal(p, q) for p, q in zip(a.download_counters(), b.download_counters()))
    assert not np.array_equal(bits(a.download_state()[0]), bits(c.download_state()[0]))
    # clearing: from the same state and step on, the plain bits
    x, _ = c.download_state()
    a.upload_state(x, start_state(R, R * L)[1])
    c.set_rung_sigma(None)
    with pytest.raises(gpu.AmcError):
        c.rung_sigma()
    for e in (a, c):
        e.sweep(3)
    assert np.array_equal(bits(a.download_state()[0]), bits(c.download_state()[0]))
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("K", [1, 2, 9])
@pytest.mark.parametrize("wide", [False, True])
def test_rung_counter_totals(gpu, monkeypatch, K, wide):
    if wide:
        monkeypatch.setenv("AMC_WIDE_COUNTERS", "1")
    R, L = 4, 129
    for tab in (None, table(K, R) if K * R <= 64 else None):
        eng = make_engine(gpu, R, L, K, tab=tab)
        eng.sweep(5); eng.exchange(1); eng.sweep(2)
        check_rung_totals(eng, R)
        acc, tot = eng.download_counters()
        # counts beyond 2^32 go into the 64-bit bases; the total_calls of a chain add up to the same step count on every chain
        ar, add = np.arange(R * L), np.zeros_like(tot)
        if K == 1:
            add[0] = 1 << 34
        else:
            add[0], add[K - 1] = (1 << 33) + ar, (1 << 33) + R * L - ar
        eng.upload_counters(acc + add // 2, tot + add)
        eng.sweep(3)
        check_rung_totals(eng, R)
        eng.close()


def test_refusals_leave_the_handle_as_it_was(gpu):
    R, L, K = 5, 40, 2
    ref = make_engine(gpu, R, L, K)
    eng = make_engine(gpu, R, L, K, ladder=False)
    with pytest.raises(gpu.AmcError, match="no ladder"):
        eng.set_rung_sigma(table(K, R))
    eng.set_ladder(R)
    for bad in (0.0, float("nan"), 1e101):
        t = table(K, R); t[1, 2] = bad
        with pytest.raises(gpu.AmcError, match=r"sigma\[7\]"):
            eng.set_rung_sigma(t)
    with pytest.raises(gpu.AmcError, match="entries"):
        eng.set_rung_sigma(np.full(K * R + 1, 0.3))
    for e in (ref, eng):
        e.sweep(2); e.exchange(1); e.sweep(1)
    assert np.array_equal(bits(ref.download_state()[0]), bits(eng.download_state()[0]))
    # an estimator call while a table is set; the sweeps go on
    eng.set_rung_sigma(table(K, R))
    with pytest.raises(gpu.AmcError, match="widths per rung"):
        eng.pg_estimate([0], 2)
    with pytest.raises(gpu.AmcError, match="widths per rung"):
        eng.pgmc_steps(1, [0], 2, [1], [0.05], [0.0])
    eng.set_rung_sigma(None)
    for e in (ref, eng):
        e.sweep(2)
    assert np.array_equal(bits(ref.download_state()[0]), bits(eng.download_state()[0]))
    ref.close(); eng.close()


def test_a_table_of_65_entries_is_refused(gpu):
    R, L, K = 13, 4, 5
    ref, big = make_engine(gpu, R, L, K), make_engine(gpu, R, L, K)
    with pytest.raises(gpu.AmcError, match="65"):
        big.set_rung_sigma(np.full((K, R), 0.3))
    with pytest.raises(gpu.AmcError):
        big.rung_sigma()                                   # no table was set
    for e in (ref, big):
        e.sweep(2); e.exchange(1); e.sweep(1)
    assert np.array_equal(bits(ref.download_state()[0]), bits(big.download_state()[0]))
    assert all(np.array_equal(p, q) for p, q in zip(ref.download_counters(), big.download_counters()))
    ref.close(); big.close()


@pytest.mark.parametrize("extra,words", [
    (dict(per_chain_counters=False), "per_chain_counters"),
    (dict(per_chain_counters=True, dtype="f32", param_dtype="f32"), "AMC_DTYPE_F32"),
    (dict(per_chain_counters=True, proposal=("sigma*z", "-(delta*delta)/(2.0*(sigma*sigma)) - amc_log(sigma)", None)), "script-defined"),
], ids=["no_per_chain_counters", "f32_parameters", "script_policy"])
def test_handles_that_take_no_table_refuse_it_and_sweep_on(gpu, extra, words):
    """The refused handle against a handle of the same configuration that was never asked: the same bits after the same steps."""
    x, beta = start_state(4, 64)
    kw = dict(n_chains=64, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=3)
    ref, e = gpu.HipEngine(**kw, **extra), gpu.HipEngine(**kw, **extra)
    for h in (ref, e):
        h.upload_state(x, beta)
        h.set_ladder(4)
    with pytest.raises(gpu.AmcError, match=words):
        e.set_rung_sigma([0.5, 0.4, 0.3, 0.2])
    for h in (ref, e):
        h.sweep(2); h.exchange(1); h.sweep(1)
    (xr, er), (xe, ee) = ref.download_state(), e.download_state()
    assert np.array_equal(bits(xr), bits(xe)) and np.array_equal(bits(er), bits(ee))
    assert all(np.array_equal(p, q) for p, q in zip(ref.counter_totals(), e.counter_totals()))
    assert all(np.array_equal(p, q) for p, q in zip(ref.exchange_counters(), e.exchange_counters()))
    ref.close(); e.close()


def test_callback_sums_of_a_handle_with_a_table(gpu):
    R, L, K = 3, 171, 2
    a, b = make_engine(gpu, R, L, K, tab=table(K, R)), make_engine(gpu, R, L, K, tab=table(K, R))
    a.sweep_reduce_begin(3)
    ra = a.reduce_end_exact()
    b.sweep(3)
    rb = b.reduce_exact()
    assert np.array_equal(np.asarray(ra[0]), np.asarray(rb[0]), equal_nan=True) and ra[1] == rb[1]
    a.close(); b.close()


def test_harmonic_ladder_with_widths_per_rung_samples_every_rung(gpu, tmp_path):
    """R = 4, beta_r = 0.5 2^r, sigma_r = 0.8 / sqrt(beta_r), 4096 ladders, 300 rounds of [1 sweep; 1 exchange] after 300 of burn-in: the
    mean over the rounds of <x^2>_r (ReplicaExchange.rung_sums) lies within six standard errors of ONE snapshot of independent ladders,
    6 sqrt(2 / 4096) / (2 beta_r), of 1 / (2 beta_r), and every Metropolis.rung_acceptance() value lies in (0.2, 0.8).  The host twin
    stays inside both (tests/test_rung_sigma_host.py)."""
    import montecarlo_amd as ma
    from montecarlo_amd._capi import AMC_REDUCE_XX
    R, L = 4, 4096
    betas = 0.5 * 2.0 ** np.arange(R)
    chains = ma.ParticleChains.ladder(L, betas, init_uniform=(-1.0, 1.0))
    al = [dict(algorithm=ma.Metropolis, pool=(ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),), seed=5, rung_sigma=0.8 / np.sqrt(betas)),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,))]
    sim = ma.Simulation(chains, al, 300, path=str(tmp_path))
    ma.run(sim)                                            # the burn-in: 300 x [sweep; exchange]
    met, rx = sim.algorithms
    assert met.engine.step == 300 and met.engine.exchange_step == 300
    xx = np.zeros(R)
    for _ in range(300):
        met.sweep_exchange(1, 1)
        xx += rx.rung_sums(AMC_REDUCE_XX)[:, 2]
    xx /= 300
    ratio = met.rung_acceptance()
    print("x^2 per rung", xx, "expected", 1 / (2 * betas), "acceptance", ratio)
    assert np.all(np.abs(xx - 1 / (2 * betas)) <= 6 * np.sqrt(2 / L) / (2 * betas))
    assert ratio.shape == (1, R) and np.all((ratio > 0.2) & (ratio < 0.8))
    ra, rt = met.engine.rung_counter_totals()
    assert rt.sum() == 600 * R * L and np.array_equal(ma.callback_rung_acceptance(sim), ra / rt) and np.array_equal(ratio, ra / rt)
    met.engine.close()


def _rx_sim(path, steps, tab):
    import montecarlo_amd as ma
    chains = ma.ParticleChains.ladder(171, [0.5, 1.0, 2.0], x=1.5 * np.sin(0.37 * np.arange(3 * 171)))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 0.625), ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.2], 0.375))
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=7, rung_sigma=tab),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2))]
    return ma.Simulation(chains, al, steps, path=str(path))


def test_metropolis_takes_the_table_and_checkpoints_carry_it(gpu, tmp_path):
    """Metropolis(rung_sigma=...) hands the table to the engine with the ladder; a run checkpointed and restored in the middle ends
    where the uninterrupted run ends; the field is there only when a table is set."""
    import montecarlo_amd as ma
    tab = table(2, 3)
    whole = _rx_sim(tmp_path / "w", 12, tab)
    ma.run(whole)
    met = whole.algorithms[0]
    assert np.array_equal(met.engine.rung_sigma(), tab) and met.engine.per_chain_counters
    ra, rt = met.engine.rung_counter_totals()
    assert np.array_equal(met.rung_acceptance(), ra / rt) and rt.sum() == 12 * 3 * 171
    first = _rx_sim(tmp_path / "a", 6, tab)
    ma.run(first)
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    assert np.array_equal(np.load(tmp_path / "ck" / "checkpoint_rank0.npz")["rung_sigma"], tab)
    second = _rx_sim(tmp_path / "b", 6, tab * 0.5)         # the checkpoint's table replaces the constructor's
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    assert np.array_equal(second.algorithms[0].engine.rung_sigma(), tab)
    ma.run(second)
    assert np.array_equal(bits(whole.chains.x), bits(second.chains.x))
    assert all(np.array_equal(p, q) for p, q in zip(met.engine.download_counters(), second.algorithms[0].engine.download_counters()))
    plain = _rx_sim(tmp_path / "p", 4, None)
    ma.run(plain)
    ma.checkpoint(plain.algorithms[0], str(tmp_path / "ckp"))
    assert "rung_sigma" not in np.load(tmp_path / "ckp" / "checkpoint_rank0.npz").files
