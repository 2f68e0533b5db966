"""Float32 policy parameters (param_dtype = "f32": the all-Float32 model) on the device, against the host
twin of the new arithmetic (tests/f32_param_twin.py) BIT FOR BIT: positions, energies, pooled and per-chain counters, callback
records word for word -- in every sweep form that exists for Float32 state.  Also: what such a handle refuses, the sigma range,
and that handles with param_dtype = 0 compute what they computed before."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import f32_param_twin as T
import montecarlo_amd as ma

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def f32s(*v):
    return [float(F(x)) for x in v]


def make_pair(gpu, M, *, counters=True, offset=0, n_global=None, **kw):
    kw.setdefault("seed", 11)
    eng = gpu.HipEngine(n_chains=M, dtype="f32", param_dtype="f32", per_chain_counters=counters, chain_offset=offset,
                        n_chains_global=n_global if n_global is not None else offset + M, **kw)
    sim = T.TwinSim(M, chain_offset=offset, **kw)
    return eng, sim


def assert_same_state(eng, sim, per_chain=True):
    x, e = eng.download_state()
    xo, eo = sim.state()
    assert np.array_equal(bits(x), bits(xo)) and np.array_equal(bits(e), bits(eo))
    acc, tot = eng.counter_totals()
    ao, to = sim.counters()
    assert acc.tolist() == ao.sum(axis=1).tolist() and tot.tolist() == to.sum(axis=1).tolist()
    if per_chain:
        a, t = eng.download_counters()
        assert np.array_equal(a, ao) and np.array_equal(t, to)


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
@pytest.mark.parametrize("counters", [False, True])
def test_single_move_bit_exact(gpu, potential, counters):
    M = 20011                                              # odd: a lone last chain
    eng, sim = make_pair(gpu, M, potential=potential, beta=2.0, sigma=f32s(0.35), weight=[1.0], counters=counters)
    eng.init_uniform(-2.0, 2.0)
    sim.init_uniform(-2.0, 2.0)
    assert_same_state(eng, sim, counters)
    for n in (1, 1, 7, 1, 64):                             # single-step launches and fused ones
        eng.sweep(n)
        sim.make_steps(n)
        assert_same_state(eng, sim, counters)
    eng.close()


def test_three_moves_with_weights_and_callback_records(gpu):
    M = 20011
    eng, sim = make_pair(gpu, M, potential="double_well", beta=2.0, sigma=f32s(0.2, 0.7, 1.5), weight=[0.3, 0.45, 0.25], seed=3)
    eng.init_uniform(-2.0, 2.0)
    sim.init_uniform(-2.0, 2.0)
    for n in (1, 1, 7, 1, 64):
        eng.sweep(n)
        sim.make_steps(n)
    assert_same_state(eng, sim)
    # the callback sums: a pass of their own, then formed inside the sweep launch (single-step and fused) -- records word for word
    rec, steps = eng.reduce_exact()
    assert steps == 74 and np.array_equal(rec, sim.callback_records(), equal_nan=True)
    for n in (1, 10):
        eng.sweep_reduce_begin(n)
        rec, _ = eng.reduce_end_exact()
        sim.make_steps(n)
        assert np.array_equal(rec, sim.callback_records(), equal_nan=True)
    assert_same_state(eng, sim)
    eng.close()


def test_custom_potential_and_the_pool_wide_counter_in_the_callback(gpu):
    M = 10001
    pot = ma.CustomPotential("0.5*x*x + 0.1f*x*x*x*x")          # a Float64 literal promotes, a Float32 one does not
    eng, sim = make_pair(gpu, M, potential=pot, beta=1.5, sigma=f32s(0.6), weight=[1.0], counters=False, seed=8)
    eng.init_uniform(-2.0, 2.0)
    sim.init_uniform(-2.0, 2.0)
    for n in (1, 5):
        eng.sweep_reduce_begin(n)
        rec, steps = eng.reduce_end_exact()
        sim.make_steps(n)
        want = sim.callback_records()
        assert np.array_equal(rec[:4], want[:4])
        red = eng.reduce_records_value(rec, steps)
        assert red[4] == sim.acc.sum() / sim.t                    # pool-wide accepted total / steps
    assert_same_state(eng, sim, per_chain=False)
    eng.close()


@pytest.mark.parametrize("fuse", [True, False])
def test_callbacks_every_ten_steps_through_simulation(gpu, tmp_path, fuse):
    M, steps = 4099, 60
    chains = ma.ParticleChains.uniform(M, 2.0, -2.0, 2.0, dtype="f32")
    pool = (ma.Move(ma.Displacement(0.0), ma.StandardGaussian(), F([0.2]), 0.6), ma.Move(ma.Displacement(0.0), ma.StandardGaussian(), F([0.9]), 0.4))
    sched = ma.build_schedule(steps, 0, [0, 10])
    sim = ma.Simulation(chains, (dict(algorithm=ma.Metropolis, pool=pool, seed=42),
                                 dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_energy, ma.callback_acceptance), scheduler=sched),
                                 dict(algorithm=ma.StoreParameters, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 30))), steps, path=str(tmp_path))
    ma.run(sim, fuse=fuse)
    tw = T.TwinSim(M, potential="harmonic", beta=2.0, sigma=f32s(0.2, 0.9), weight=[0.6, 0.4], seed=42)
    tw.init_uniform(-2.0, 2.0)
    rows_e = open(tmp_path / "energy.dat").read().splitlines()
    rows_a = open(tmp_path / "acceptance.dat").read().splitlines()
    import oracle_lib as O
    from montecarlo_amd.simulation import julia_repr
    for row_e, row_a in zip(rows_e[1:], rows_a[1:]):
        t = int(row_e.split()[0])
        tw.make_steps(t - tw.t)
        val = O.xsum_round(tw.callback_records())
        assert row_e == f"{t} {julia_repr(val[0] / M)}"
        assert row_a == f"{t} {julia_repr(list(val[4:] / M))}"
    assert tw.t == steps
    assert np.array_equal(bits(sim.chains.x), bits(tw.state()[0]))
    assert open(tmp_path / "parameters" / "1" / "parameters.dat").read().splitlines()[0] == "0 Float32[0.2]"


def test_exact_accept_path_agrees_with_the_filter(gpu, monkeypatch):
    """Every wave through accept_exact (the Float32 quotient, the Float64 exp) gives the filter path's bits -- and the twin's."""
    M = 20011
    kw = dict(potential="double_well", beta=2.5, sigma=f32s(0.4, 0.9), weight=[0.5, 0.5], seed=5)
    a, sim = make_pair(gpu, M, **kw)
    monkeypatch.setenv("AMC_EXACT_ACCEPT", "1")
    b, _ = make_pair(gpu, M, **kw)
    monkeypatch.delenv("AMC_EXACT_ACCEPT")
    sim.init_uniform(-2, 2)
    for e in (a, b):
        e.init_uniform(-2, 2)
        e.sweep(1)
        e.sweep(30)
    sim.make_steps(31)
    assert_same_state(a, sim)
    assert_same_state(b, sim)
    a.close()
    b.close()


@pytest.mark.parametrize("n_shards", [1, 2, 3])
def test_shards_by_chain_offset_equal_the_unsharded_run(gpu, n_shards):
    M = 6007
    kw = dict(potential="harmonic", beta=2.0, sigma=f32s(0.3, 1.1), weight=[0.5, 0.5], seed=77)
    whole = T.TwinSim(M, **kw)
    whole.init_uniform(-2, 2)
    whole.make_steps(12)
    n_pairs = (M + 1) // 2
    bounds = [min(2 * ((i * n_pairs) // n_shards), M) for i in range(n_shards)] + [M]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        eng = gpu.HipEngine(n_chains=hi - lo, chain_offset=lo, n_chains_global=M, dtype="f32", param_dtype="f32", **kw)
        eng.init_uniform(-2, 2)
        eng.sweep(1)
        eng.sweep(11)
        x, _ = eng.download_state()
        assert np.array_equal(bits(x), bits(whole.state()[0][lo:hi]))
        assert np.array_equal(eng.download_counters()[0], whole.acc[:, lo:hi])
        eng.close()


def test_checkpoint_resume_equals_the_uninterrupted_run_and_the_other_type_is_refused(gpu, tmp_path):
    from montecarlo_amd import storage
    M = 3001

    def build(params):
        chains = ma.ParticleChains.uniform(M, 2.0, -2.0, 2.0, dtype="f32")
        pool = (ma.Move(ma.Displacement(0.0), ma.StandardGaussian(), params, 1.0),)
        met = ma.Metropolis(chains, pool=pool, seed=19, per_chain_counters=True)
        met.engine.init_uniform(-2.0, 2.0)
        return met
    a = build(F([0.3]))
    a.engine.sweep(9)
    storage.checkpoint(a, str(tmp_path))
    a.engine.sweep(16)
    b = build(F([0.3]))
    storage.restore(b, str(tmp_path))
    b.engine.sweep(16)
    assert np.array_equal(bits(a.engine.download_state()[0]), bits(b.engine.download_state()[0]))
    assert np.array_equal(a.engine.download_counters()[0], b.engine.download_counters()[0])
    tw = T.TwinSim(M, potential="harmonic", beta=2.0, sigma=f32s(0.3), seed=19)
    tw.init_uniform(-2, 2)
    tw.make_steps(25)
    assert np.array_equal(bits(b.engine.download_state()[0]), bits(tw.state()[0]))
    c = build([float(F(0.3))])                               # the same value as a Float64 parameter: other arithmetic
    with pytest.raises(ValueError, match="param_dtype"):
        storage.restore(c, str(tmp_path))


def test_sigma_range_edges_and_checked_values(gpu):
    lo, hi = 2.0 ** -63, 2.0 ** 60
    for s in (lo, hi):
        eng, sim = make_pair(gpu, 1025, potential="harmonic", beta=2.0, sigma=[s], weight=[1.0])
        eng.init_uniform(-2, 2)
        sim.init_uniform(-2, 2)
        eng.sweep(1)
        eng.sweep(5)
        sim.make_steps(6)
        assert_same_state(eng, sim)
        eng.close()
    kw = dict(n_chains=64, dtype="f32", param_dtype="f32", weight=[1.0])
    for bad, what in ((0.1, "not a Float32"), (lo / 2, r"\[2\^-63, 2\^60\]"), (hi * 2, r"\[2\^-63, 2\^60\]"), (float("nan"), "Float32")):
        with pytest.raises(gpu.AmcError, match=what):
            gpu.HipEngine(sigma=[bad], **kw)
    with pytest.raises(gpu.AmcError, match="param_dtype.*requires state_dtype"):
        gpu.HipEngine(n_chains=64, dtype="f64", param_dtype="f32", sigma=f32s(0.1), weight=[1.0])
    eng, sim = make_pair(gpu, 1025, potential="harmonic", beta=2.0, sigma=f32s(0.5), weight=[1.0])
    for bad in (0.1, lo / 2):
        with pytest.raises(gpu.AmcError):
            eng.set_parameters(0, [bad])
    assert eng.get_parameters(0)[0] == float(F(0.5))
    eng.set_parameters(0, f32s(0.25))                        # ... and a Float32 value is taken: the table follows
    sim.set_sigma(0, F(0.25))
    eng.init_uniform(-2, 2)
    sim.init_uniform(-2, 2)
    eng.sweep(8)
    sim.make_steps(8)
    assert_same_state(eng, sim)
    eng.close()


def test_what_is_not_built_is_refused_and_the_handle_still_sweeps(gpu):
    eng, sim = make_pair(gpu, 2049, potential="harmonic", beta=2.0, sigma=f32s(0.2, 0.1), weight=[0.6, 0.4])
    eng.init_uniform(-2, 2)
    sim.init_uniform(-2, 2)
    calls = (lambda: eng.pg_estimate([1], 2), lambda: eng.pg_estimate_exact([1], 2), lambda: eng.pg_accumulate([1], 2),
             lambda: eng.pg_update([1], [1], [0.05], [0.0]), lambda: eng.pgmc_steps(1, [1], 2, [1], [0.05], [0.0]),
             lambda: eng.pgmc_steps(1, [1], 2, [1], [0.05], [0.0], reduce_begin=True), lambda: eng.pg_get_accumulated([1]))
    for call in calls:
        with pytest.raises(gpu.AmcError, match="param_dtype"):
            call()
    eng.sweep(3)
    sim.make_steps(3)
    assert_same_state(eng, sim)
    eng.close()
    kw = dict(n_chains=64, dtype="f32", param_dtype="f32", sigma=f32s(0.5), weight=[1.0])
    mala = ("-2.0*sigma*sigma*x + sigma*z", "-((delta + 2.0*sigma*sigma*x)*(delta + 2.0*sigma*sigma*x))/(2.0*(sigma*sigma)) - amc_log(sigma)", None)
    gauss = ("sigma*z", "-(delta*delta)/(2.0*(sigma*sigma)) - amc_log(6.283185307179586*(sigma*sigma))/2.0", None)
    for extra in (dict(proposal=mala), dict(scale_expr="0.5 + x*x"), dict(classes=[gauss], class_of_move=[0]),
                  dict(proposal=("theta0 + theta1*z", "-((delta-theta0)*(delta-theta0))/(2.0*theta1*theta1) - amc_log(theta1)", None), n_params=2,
                       sigma=[f32s(0.1, 0.5)])):
        with pytest.raises(gpu.AmcError, match="param_dtype"):
            gpu.HipEngine(**{**kw, **extra})


@pytest.mark.parametrize("idx", [0, 4])
def test_handles_with_param_dtype_zero_compute_what_they_did(gpu, idx):
    """A Float64 and a Float32-state run with Float64 parameters equal the golden trajectories, created after (and beside) a
    Float32-parameter handle of the same process: the new define leaves the old forms' code objects alone."""
    other, _ = make_pair(gpu, 257, potential="harmonic", beta=2.0, sigma=f32s(0.1), weight=[1.0])
    other.init_uniform(-2, 2)
    other.sweep(2)
    case = json.load(open(os.path.join(GOLDEN, "oracle_trajectories.json")))["cases"][idx]
    sp = case["spec"]
    fh = lambda v: np.array([float.fromhex(s) for s in v])
    e = gpu.HipEngine(n_chains=sp["M"], chain_offset=sp["offset"], n_chains_global=sp["offset"] + sp["M"], potential=sp["potential"],
                      beta=sp["beta"], sigma=sp["sigma"], weight=sp["weight"], seed=sp["seed"], sweepstep=sp["sweepstep"],
                      dtype=sp.get("dtype", "f64"), param_dtype="f64")
    e.init_uniform(-2.0, 2.0)
    done = 0
    for snap in case["snapshots"]:
        e.sweep(snap["sweep"] - done)
        done = snap["sweep"]
        x, en = e.download_state()
        assert np.array_equal(bits(x), bits(fh(snap["x"]))) and np.array_equal(bits(en), bits(fh(snap["e"])))
        acc, tot = e.download_counters()
        assert acc.tolist() == snap["accepted"] and tot.tolist() == snap["total"]
    e.close()
    other.close()


def test_stationary_density_goodness_of_fit_at_full_size_float32_parameters(gpu):
    """test_stationary_density_goodness_of_fit_at_full_size for the all-Float32 model: 1e7 independent chains after its burn-in,
    a 200-bin histogram against exp(-beta x^2), chi^2 within 5 sigma of its degrees of freedom (harmonic, beta = 2, sigma = 0.1f0)."""
    from scipy import stats
    M, beta, n_bins, lo, hi, burn = 10_000_000, 2.0, 200, -2.0, 2.0, 6000
    e = gpu.HipEngine(n_chains=M, beta=beta, seed=20260304, potential="harmonic", sigma=f32s(0.1), weight=[1.0], per_chain_counters=False,
                      dtype="f32", param_dtype="f32")
    e.init_uniform(-2, 2)
    e.sweep(burn)
    counts = e.histogram(lo, hi, n_bins).astype(np.float64)
    assert counts[n_bins + 2] == 0 and counts.sum() == M
    edges = np.linspace(lo, hi, n_bins + 1)
    cdf = stats.norm(0.0, 1.0 / np.sqrt(2 * beta)).cdf
    p = np.concatenate([np.diff(cdf(edges)), [cdf(lo), cdf(lo)]])
    expect = p * M
    obs = counts[:n_bins + 2]
    keep = expect >= 20
    chi2 = float(np.sum((obs[keep] - expect[keep]) ** 2 / expect[keep]))
    dof = int(keep.sum()) - 1
    print(f"all-Float32 stationary density: chi2 = {chi2:.1f}, dof = {dof}")
    assert dof >= 150
    assert abs(chi2 - dof) < 5.0 * np.sqrt(2.0 * dof), (chi2, dof)
    # the same numbers as a mean / variance statement, by the same 5-sigma rule: x ~ N(0, 1 / (2 beta)) over 1e7 independent chains,
    # standard error of the mean 0.5 / sqrt(M) = 1.58e-4, of the second moment sqrt(2) 0.25 / sqrt(M) = 1.12e-4
    r = e.reduce()
    assert abs(r[1] / M) < 5.0 * 0.5 / np.sqrt(M)
    assert abs(r[2] / M - 1.0 / (2 * beta)) < 5.0 * np.sqrt(2.0) * 0.25 / np.sqrt(M)
    e.close()
