"""Replica exchange on the device (include/amc.h amc_set_ladder .. amc_histogram_rungs) against its host twin
(tests/exchange_twin.py), bit for bit: positions, energies, the Move counters and the gap counters, over sequences that interleave
sweeps and exchange steps.  Shapes are the smallest at which the kernel takes another path: ladders that straddle wave (64) and
block (256) boundaries, odd R (ladders off the 16-byte pairs), R = 2 (an empty odd phase), one ladder (one partial block), a grid
that is walked more than once."""
import json
import os

import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd.system import CustomPotential

import exchange_twin as X
import oracle_lib as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POOLS = {1: ([0.5], [1.0]), 2: ([0.5, 0.25], [0.625, 0.375])}
CUSTOM = "x*x*x*x - 2.0*x*x + 0.25*x"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def start_state(R, M, offset=0, beta_kind="ladder", seed=11):
    """x and beta of the chains [offset, offset + M) as functions of the GLOBAL chain id."""
    ids = np.arange(offset, offset + M)
    x = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)
    if beta_kind == "ladder":
        beta = (0.5 * 1.5 ** np.arange(R))[ids % R]
    else:                                                  # not periodic in R: the kernel only ever reads beta_c
        beta = np.random.default_rng(seed).uniform(0.3, 6.0, size=offset + M)[offset:]
    return x, beta


def make_pair(gpu, R, L, *, potential="harmonic", K=1, counters=True, dtype="f64", param_dtype="f64", beta_kind="ladder", offset=0,
              n_global=None, seed=23):
    """(HipEngine, ExchangeTwin over the matching host simulation), both holding the same start state and a ladder of R rungs."""
    M = R * L
    sigma, weight = POOLS[K]
    x, beta = start_state(R, M, offset, beta_kind)
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


def twin_state(tw):
    s = tw.state.sim
    return s.state()


def compare(eng, tw, counters=True):
    x, e = eng.download_state()
    xo, eo = twin_state(tw)
    assert np.array_equal(bits(x), bits(xo)), "positions differ from the twin"
    assert np.array_equal(bits(e), bits(eo)), "energies differ from the twin"
    ao, to = tw.state.sim.counters()
    if counters:
        acc, tot = eng.download_counters()
        assert np.array_equal(acc, ao) and np.array_equal(tot, to), "Move counters differ from the twin"
    acc_t, tot_t = eng.counter_totals()
    assert np.array_equal(acc_t, ao.sum(axis=1)) and np.array_equal(tot_t, to.sum(axis=1))
    ga, gt = eng.exchange_counters()
    assert np.array_equal(ga, tw.accepted) and np.array_equal(gt, tw.attempted), ("gap counters differ from the twin", ga, gt, tw.counters())
    assert eng.exchange_step == tw.t_x


def interleave(eng, tw):
    """sweep(1), exchange(1), sweep(3), exchange(2), sweep_exchange(4, 2) on both; compared after the separate calls and at the end."""
    for obj in (eng, tw):
        obj.sweep(1); obj.exchange(1); obj.sweep(3); obj.exchange(2)
    t_before = eng.step
    compare(eng, tw, counters=eng.per_chain_counters)
    for obj in (eng, tw):
        obj.sweep_exchange(4, 2)
    assert eng.step == t_before + 8 and eng.estimator_step == 0          # exchange steps leave t and t_est alone
    compare(eng, tw, counters=eng.per_chain_counters)


SHAPES = [(2, 1), (2, 513), (3, 1), (3, 171), (4, 129), (6, 171), (64, 9)]


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
@pytest.mark.parametrize("R,L", SHAPES)
def test_exchange_matches_the_twin(gpu, R, L, potential):
    eng, tw = make_pair(gpu, R, L, potential=potential)
    interleave(eng, tw)
    acc, att = eng.exchange_counters()
    if R == 2:
        assert att.tolist() == [4 * L]                   # 7 exchange steps, the 3 odd ones attempt nothing
    eng.close()


@pytest.mark.parametrize("K,counters", [(1, False), (2, True)])
@pytest.mark.parametrize("R,L", [(3, 171), (4, 129)])
def test_exchange_with_other_pools(gpu, R, L, K, counters):
    eng, tw = make_pair(gpu, R, L, potential="double_well", K=K, counters=counters)
    interleave(eng, tw)
    eng.close()


@pytest.mark.parametrize("dtype,param_dtype", [("f32", "f64"), ("f32", "f32")])
@pytest.mark.parametrize("R,L,potential", [(3, 171, "double_well"), (4, 129, "harmonic")])
def test_exchange_with_float32_state(gpu, R, L, potential, dtype, param_dtype):
    eng, tw = make_pair(gpu, R, L, potential=potential, dtype=dtype, param_dtype=param_dtype)
    interleave(eng, tw)
    x = eng.download_state()[0]
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exchange_with_a_custom_potential(gpu, dtype):
    eng, tw = make_pair(gpu, 3, 171, potential=CustomPotential(CUSTOM), dtype=dtype)
    interleave(eng, tw)
    eng.close()


@pytest.mark.parametrize("R,L", [(3, 171), (6, 171)])
def test_exchange_reads_beta_per_chain(gpu, R, L):
    """A beta array that is not periodic in R (random per chain): the kernel only ever reads beta_c."""
    eng, tw = make_pair(gpu, R, L, potential="double_well", beta_kind="random")
    interleave(eng, tw)
    eng.close()


def test_grid_stride(gpu, monkeypatch):
    """One block per CU and 3 x 30 001 gaps per even step: the grid-stride loop runs more than once."""
    monkeypatch.setenv("AMC_BLOCKS_PER_CU", "1")
    eng, tw = make_pair(gpu, 6, 30001)
    monkeypatch.delenv("AMC_BLOCKS_PER_CU")
    for obj in (eng, tw):
        obj.sweep(1); obj.exchange(2)
    compare(eng, tw)
    assert eng.exchange_counters()[1].tolist() == [30001] * 5
    eng.close()


def test_shard_invariance(gpu):
    """The global range as one handle and as two and three handles whose offsets are multiples of R: equal bits per chain, gap
    counters that add up to the whole's."""
    R, L = 3, 342
    M = R * L
    whole, tw = make_pair(gpu, R, L, potential="double_well", K=2)
    seq = lambda o: (o.sweep(2), o.exchange(1), o.sweep(1), o.exchange(2), o.sweep_exchange(2, 1))
    seq(whole); seq(tw)
    compare(whole, tw)
    xw, cw = whole.download_state()[0], whole.exchange_counters()
    for split in ([0, 402, M], [0, 258, 264, M]):
        parts = [make_pair(gpu, R, (b - a) // R, potential="double_well", K=2, offset=a, n_global=M)[0] for a, b in zip(split, split[1:])]
        for p in parts:
            seq(p)
        x = np.concatenate([p.download_state()[0] for p in parts])
        assert np.array_equal(bits(x), bits(xw))
        cnt = [p.exchange_counters() for p in parts]
        assert np.array_equal(sum(c[0] for c in cnt), cw[0]) and np.array_equal(sum(c[1] for c in cnt), cw[1])
        for p in parts:
            p.close()
    whole.close()


def test_refusals_leave_the_handle_as_it_was(gpu):
    kw = dict(potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=23)
    x, beta = start_state(3, 60)
    eng = gpu.HipEngine(n_chains=60, **kw)
    eng.upload_state(x)
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*per-chain beta"):
        eng.set_ladder(3)                                     # no beta array
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*no ladder"):
        eng.exchange(1)
    eng.upload_state(x, beta)
    for R, what in [(1, "n_rungs = 1"), (65, "n_rungs = 65"), (-2, "n_rungs = -2"), (7, "n_chains_global = 60")]:
        with pytest.raises(gpu.AmcError, match=r"amc error -1.*" + what):
            eng.set_ladder(R)
    with pytest.raises(gpu.AmcError, match=r"amc error -5"):
        eng.sweep_exchange(1, 1)
    with pytest.raises(gpu.AmcError, match=r"amc error -5"):
        eng.exchange_counters()
    part = gpu.HipEngine(n_chains=20, chain_offset=4, n_chains_global=60, **kw)      # offset 4 and count 20: no multiples of 3
    part.upload_state(x[4:24], beta[4:24])
    with pytest.raises(gpu.AmcError, match=r"amc error -1.*chain_offset = 4"):
        part.set_ladder(3)
    part.close()
    part = gpu.HipEngine(n_chains=20, chain_offset=6, n_chains_global=60, **kw)
    part.upload_state(x[6:26], beta[6:26])
    with pytest.raises(gpu.AmcError, match=r"amc error -1.*n_chains = 20"):
        part.set_ladder(3)
    part.close()
    # the refused handle still sweeps, takes a valid ladder, and matches the twin
    sim = O.OracleSim(60, beta=1.0, sigma=[0.5], weight=[1.0], seed=23)
    sim.set_x(x); sim.set_beta(beta)
    tw = X.ExchangeTwin(sim, beta, 3, seed=23)
    eng.sweep(2); tw.sweep(2)
    eng.set_ladder(3)
    eng.exchange(2); tw.exchange(2)
    compare(eng, tw)
    eng.set_ladder(0)                                         # cleared: exchange is refused again, sweeps go on
    with pytest.raises(gpu.AmcError, match=r"amc error -5"):
        eng.exchange(1)
    eng.sweep(1); tw.sweep(1)
    assert np.array_equal(bits(eng.download_state()[0]), bits(sim.state()[0]))
    eng.close()


def _run_list(tmp, fuse, pgmc):
    steps = 40
    chains = ma.ParticleChains.ladder(343, [0.5, 1.0, 2.0], x=start_state(3, 1029)[0], potential="double_well")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 0.6), ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.2], 0.4))
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=9)]
    if pgmc:
        al += [dict(algorithm=ma.PolicyGradientEstimator, dependencies=(ma.Metropolis,), optimisers=(ma.Static(), ma.VPG(0.01)), q_batch_size=2),
               dict(algorithm=ma.PolicyGradientUpdate, dependencies=(ma.PolicyGradientEstimator,))]
    al += [dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 3)),
           dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_energy, ma.callback_acceptance, ma.callback_exchange_acceptance),
                scheduler=ma.build_schedule(steps, 0, 10))]
    sim = ma.Simulation(chains, al, steps, path=str(tmp))
    ma.run(sim, fuse=fuse)
    files = {f: open(os.path.join(str(tmp), f)).read() for f in ("energy.dat", "acceptance.dat", "exchange_acceptance.dat")}
    return sim.chains.x.copy(), files, [m.sigma for m in sim.algorithms[0].pool]


@pytest.mark.parametrize("pgmc", [False, True])
def test_fused_run_equals_stepwise_run(gpu, tmp_path, pgmc):
    a = _run_list(tmp_path / "stepwise", False, pgmc)
    b = _run_list(tmp_path / "fused", True, pgmc)
    assert np.array_equal(bits(a[0]), bits(b[0]))
    assert a[1] == b[1] and a[2] == b[2]
    assert "NaN" in a[1]["exchange_acceptance.dat"].splitlines()[0] and "NaN" not in a[1]["exchange_acceptance.dat"].splitlines()[-1]


def test_checkpoint_after_an_odd_number_of_exchange_steps(gpu, tmp_path):
    def build(path, steps):
        chains = ma.ParticleChains.ladder(171, [0.5, 1.0, 2.0], x=start_state(3, 513)[0], potential="double_well")
        pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
        al = [dict(algorithm=ma.Metropolis, pool=pool, seed=4, per_chain_counters=True),
              dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2))]
        return ma.Simulation(chains, al, steps, path=str(path))
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
    assert np.array_equal(bits(whole.chains.x), bits(second.chains.x))
    assert e1.exchange_step == e2.exchange_step == 6
    assert all(np.array_equal(a, b) for a, b in zip(e1.exchange_counters(), e2.exchange_counters()))
    assert all(np.array_equal(a, b) for a, b in zip(e1.download_counters(), e2.download_counters()))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_histogram_by_rung(gpu, dtype):
    R, L, lo, hi, nb = 5, 205, -1.25, 1.5, 37
    eng, tw = make_pair(gpu, R, L, dtype=dtype)
    eng.sweep(2); eng.exchange(1)
    x = eng.download_state()[0]
    x[7], x[13] = np.nan, np.inf
    eng.upload_state(x)

    def expected(n):
        want = np.zeros((R, n + 3), dtype=np.uint64)
        inv_w = n / (hi - lo)
        for r in range(R):
            v = x[r::R]
            nan = np.isnan(v)
            below, above = (v < lo) & ~nan, (v >= hi) & ~nan
            inside = ~(nan | below | above)
            want[r, :n] = np.bincount(np.minimum(((v[inside] - lo) * inv_w).astype(np.int64), n - 1), minlength=n)
            want[r, n], want[r, n + 1], want[r, n + 2] = below.sum(), above.sum(), nan.sum()
        return want

    got = eng.histogram_rungs(lo, hi, nb)
    assert got.shape == (R, nb + 3)
    assert np.array_equal(got, expected(nb)), np.argwhere(got != expected(nb))
    assert np.array_equal(got.sum(axis=0), eng.histogram(lo, hi, nb))
    wide = eng.histogram_rungs(lo, hi, 4000)                   # rows too large for LDS: the global-atomic form, the same bin rule
    assert np.array_equal(wide, expected(4000)), np.argwhere(wide != expected(4000))
    assert np.array_equal(wide.sum(axis=0), eng.histogram(lo, hi, 4000)) and wide.sum() == R * L
    eng.close()


@pytest.mark.parametrize("idx", [0, 3])
def test_handles_without_a_ladder_are_left_alone(gpu, idx):
    """A handle with no ladder, created after and beside one that has exchanged, reproduces the golden trajectories."""
    other, _ = make_pair(gpu, 3, 171)
    other.sweep(1); other.exchange(2)
    case = json.load(open(os.path.join(GOLDEN, "oracle_trajectories.json")))["cases"][idx]
    sp = case["spec"]
    fh = lambda v: np.array([float.fromhex(s) for s in v])
    e = gpu.HipEngine(n_chains=sp["M"], chain_offset=sp["offset"], n_chains_global=sp["offset"] + sp["M"], potential=sp["potential"],
                      beta=sp["beta"], sigma=sp["sigma"], weight=sp["weight"], seed=sp["seed"], sweepstep=sp["sweepstep"],
                      dtype=sp.get("dtype", "f64"), scale_expr=sp.get("scale"))
    e.init_uniform(-2.0, 2.0)
    done = 0
    for snap in case["snapshots"]:
        e.sweep(snap["sweep"] - done)
        other.exchange(1)
        done = snap["sweep"]
        x, en = e.download_state()
        assert np.array_equal(bits(x), bits(fh(snap["x"]))) and np.array_equal(bits(en), bits(fh(snap["e"])))
        acc, tot = e.download_counters()
        assert acc.tolist() == snap["accepted"] and tot.tolist() == snap["total"]
    e.close()
    other.close()
