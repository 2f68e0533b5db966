"""Float32 policy parameters (the all-Float32 model) without a device: the host twin of the new
arithmetic (tests/aux/f32_param_twin.c) against numpy restatements, its normals as a distribution, and the host logic that
carries the parameter type from Move to the engine's configuration."""
import ctypes as C

import numpy as np
import pytest

import f32_param_twin as T
import montecarlo_amd as ma
from montecarlo_amd import _capi

N_WORDS = 10_000_000


@pytest.fixture(scope="module")
def normals():
    words = T.normal_words(20260304, 0, N_WORDS, 17)
    z, u = T.box_muller_words(words)
    return words, z, u


def edge_words():
    """radius integer (y:x) >> 12 = 0, 1, 2^52 - 1 crossed with angle bits all 0 / all 1 (the spare bits set, to show they are ignored)"""
    radius = {0: (0x00000FFF, 0x00000000), 1: (0x00001FFF, 0x00000000), (1 << 52) - 1: (0xFFFFFFFF, 0xFFFFFFFF)}
    out = []
    for _, (x, y) in radius.items():
        for w in (0x000000FF, 0xFFFFFFFF):
            out.append([x, y, 0xDEADBEEF, w])
    return np.array(out, dtype=np.uint32)


def ulp_error(z, ref):
    return np.abs(z.astype(np.float64) - ref) / np.spacing(np.abs(z)).astype(np.float64)


def test_box_muller_f32_within_8_ulp_of_the_formula_in_float64(normals):
    """Largest error of z against sqrt(-2 log u) (sin, cos)(pi w) evaluated in Float64 by numpy, over 2e7 normals and the edge
    words: <= 8 ulp of Float32 on |z| >= 2^-10 (measured: 4.7 ulp, mean 0.52)."""
    words, z, u = normals
    assert np.array_equal(u, T.radius_uniform_reference(words))       # the uniform's construction is specification: bit for bit
    assert u.min() > 0.0 and u.max() <= 1.0
    words = np.concatenate([words, edge_words()])
    ze, ue = T.box_muller_words(edge_words())
    z, u = np.concatenate([z, ze]), np.concatenate([u, ue])
    ref = T.box_muller_reference(words, u)
    big = np.abs(ref) >= 2.0 ** -10
    err = ulp_error(z, ref)
    worst = float(err[big].max())
    print(f"box_muller_f32: max {worst:.3f} ulp, mean {float(err[big].mean()):.3f} ulp over {int(big.sum())} normals")
    assert worst <= 8.0
    # below 2^-10 the error is bounded absolutely (8 ulp of 2^-10)
    assert np.abs(z.astype(np.float64) - ref)[~big].max() <= 8 * 2.0 ** -33


def test_support_reaches_beyond_7_sigma_and_u_is_never_zero():
    w = edge_words()
    z, u = T.box_muller_words(w)
    assert np.all(u > 0) and np.all(np.isfinite(z))
    # radius integer 0 -> u = 2^-53: the largest radius, sqrt(106 log 2) = 8.5717
    assert u[0] == np.float32(2.0 ** -53)
    assert np.abs(z[:2]).max() == pytest.approx(np.sqrt(106 * np.log(2.0)), rel=1e-6) and np.abs(z[:2]).max() >= 7.0
    # radius integer 2^52 - 1 -> N = 2^53 - 1 rounds to 2^53: u = 1, z = 0 exactly
    assert np.all(u[4:] == 1.0) and np.all(z[4:] == 0.0)
    # relative resolution towards 0: neighbouring radius integers near 0 give different uniforms (a 24-bit grid would not)
    assert u[0] != u[2]
    # the spare bits (x[11:0], z, w[7:0]) do not enter
    w2 = w.copy()
    w2[:, 0] &= np.uint32(0xFFFFF000)
    w2[:, 2] = 0
    w2[:, 3] &= np.uint32(0xFFFFFF00)
    assert np.array_equal(T.box_muller_words(w2)[0].view(np.uint32), z.view(np.uint32))


def test_angle_is_exact_and_equally_spaced():
    """24 angle bits: w = (2^24 - (word >> 8)) 2^-23, every one of them an exact Float32; sin and cos at the table angles are exact."""
    for word, s, c in ((0xFFFFFFFF, 0.0, 1.0), (0x00000000, 0.0, 1.0), (0x80000000, 0.0, -1.0), (0x40000000, -1.0, 0.0), (0xC0000000, 1.0, 0.0)):
        sp, cp = C.c_float(), C.c_float()
        T.load().twin_sincospi_f32(word, C.byref(sp), C.byref(cp))
        if word == 0xFFFFFFFF:                                   # w = 2^-23: sin(pi w) = pi 2^-23 to Float32 accuracy, not 0
            assert sp.value == pytest.approx(np.pi * 2.0 ** -23, rel=1e-6) and cp.value == 1.0
        else:
            assert (sp.value, cp.value) == (s, c)


def test_ten_million_normals_are_standard_normal(normals):
    from scipy import stats
    _, z, _ = normals
    x = z[:, 0].astype(np.float64)                               # one normal per word: 1e7 independent draws
    n = x.size
    assert abs(x.mean()) < 5.0 / np.sqrt(n)
    assert abs(x.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
    assert abs(np.mean(x ** 4) - 3.0) < 5.0 * np.sqrt(96.0 / n)          # Var(z^4) = 105 - 9
    # chi^2 of a 200-bin histogram on [-4, 4] plus the two tails, 5 sigma of the chi^2 distribution
    n_bins = 200
    edges = np.linspace(-4.0, 4.0, n_bins + 1)
    obs = np.concatenate([np.histogram(x, bins=edges)[0], [np.sum(x < -4.0), np.sum(x >= 4.0)]]).astype(np.float64)
    p = np.concatenate([np.diff(stats.norm.cdf(edges)), [stats.norm.cdf(-4.0)] * 2])
    expect = p * n
    keep = expect >= 20
    chi2 = float(np.sum((obs[keep] - expect[keep]) ** 2 / expect[keep]))
    dof = int(keep.sum()) - 1
    assert dof >= 150
    assert abs(chi2 - dof) < 5.0 * np.sqrt(2.0 * dof), (chi2, dof)
    # the second normal of the pair, and the pair's independence at second order
    y = z[:, 1].astype(np.float64)
    assert abs(y.mean()) < 5.0 / np.sqrt(n) and abs(y.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
    assert abs(np.mean(x * y)) < 5.0 / np.sqrt(n)


def _numpy_mc_step(oracle, pot, beta, sigma, z, u, x, e):
    """mc_step! (metropolis.jl:176-190) with Particle{Float32}, sigma::Float32, z = randn(rng, Float32), written with
    numpy.float32 scalars under Julia's promotion rules -- independent of the twin's C."""
    f32, f64 = np.float32, np.float64
    lib = oracle.load()
    potential = (lambda v: v * v) if pot == 0 else (lambda v: (v * v - f32(1.0)) * (v * v - f32(1.0)))
    two_pi = f64(2.0) * f64(np.pi)

    def logq(delta):
        q = (-(delta * delta)) / (f32(2.0) * (sigma * sigma))                       # Float32
        return f64(q) - f64(lib.amo_log(float(two_pi * f64(sigma * sigma)))) / f64(2.0)
    with np.errstate(over="ignore", invalid="ignore"):
        delta = f32(0.0) + sigma * z
        lf = logq(delta)
        e1 = e
        x = x + delta
        e = potential(x)
        dlogp = ((-e) * beta) - ((-e1) * beta)
        delta = -delta
        lb = logq(delta)
        alpha = min(1.0, lib.amo_exp(float((f64(dlogp) + lb) - lf)))
        if alpha > u:
            return 1, x, e
        x = x + delta
        return 0, x, potential(x)


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
def test_twin_sweep_equals_the_numpy_float32_restatement(oracle, potential):
    """x, e and the accept decision of 10^4 steps, bit for bit, given the twin's own (z, u)."""
    M, steps = 3, 10_000
    sim = T.TwinSim(M, potential=potential, beta=2.0, sigma=[np.float32(0.35)], seed=5, chain_offset=6)
    sim.init_uniform(-2.0, 2.0)
    x, e = sim.x.copy(), sim.e.copy()
    z, u = sim.make_steps(steps, record=True)
    pot = 0 if potential == "harmonic" else 1
    acc = np.zeros(M, dtype=np.int64)
    for c in range(M):
        xc, ec = x[c], e[c]
        for t in range(steps):
            a, xc, ec = _numpy_mc_step(oracle, pot, np.float32(2.0), np.float32(0.35), z[t, c], u[t, c], xc, ec)
            acc[c] += a
        assert xc.view(np.uint32) == sim.x[c].view(np.uint32) and ec.view(np.uint32) == sim.e[c].view(np.uint32)
    assert np.array_equal(acc, sim.acc[0]) and np.all(sim.tot[0] == steps)
    assert 0.3 * steps < acc.min() and acc.max() < steps                 # both branches of the decision are exercised


def test_accept_and_pick_uniforms_are_the_float64_forms(oracle):
    """The twin's u is the oracle's accept uniform of the same step, and with Float64 parameters the oracle picks the same moves:
    the word layout of spec v5 is untouched."""
    M, steps = 64, 50
    kw = dict(potential="harmonic", beta=2.0, weight=[0.3, 0.45, 0.25], seed=9)
    tw = T.TwinSim(M, sigma=[np.float32(0.2), np.float32(0.7), np.float32(1.5)], **kw)
    ref = oracle.OracleSim(M, sigma=[float(np.float32(0.2)), float(np.float32(0.7)), float(np.float32(1.5))], dtype="f32", **kw)
    tw.init_uniform(-2, 2)
    ref.init_uniform(-2, 2)
    assert np.array_equal(tw.state()[0], ref.state()[0])
    tw.make_steps(steps)
    ref.make_steps(steps)
    assert np.array_equal(tw.counters()[1], ref.counters()[1])           # total_calls per move and chain: the same picks


# ---- host logic: the parameter type from Move to the engine's configuration ------------------------------------------------------

def _gauss(p, w=1.0):
    return ma.Move(ma.Displacement(0.0), ma.StandardGaussian(), p, w)


class Recording:
    """engine double: keeps the keyword arguments Metropolis builds the engine with"""
    last = None

    def __init__(self, **kw):
        Recording.last = kw
        self.n_moves = len(kw["sigma"])

    def sync(self):
        pass


def test_move_remembers_float32_parameters():
    m = _gauss(np.float32([0.1]))
    assert m.param_dtype == "f32" and m.parameters.dtype == np.float32 and m.sigma == float(np.float32(0.1))
    assert _gauss(np.float32(0.1)).param_dtype == "f32" and _gauss([np.float32(0.1)]).param_dtype == "f32"
    for p in ([0.1], 0.1, np.array([0.1]), {"sigma": 0.1}):
        m = _gauss(p)
        assert m.param_dtype == "f64" and m.parameters.dtype == np.float64
    from montecarlo_amd.simulation import julia_repr
    assert julia_repr(_gauss(np.float32([0.1])).parameters) == "Float32[0.1]"
    assert julia_repr(_gauss([0.1]).parameters) == "[0.1]"


def test_metropolis_passes_param_dtype_and_refuses_mixtures():
    chains32 = ma.ParticleChains.uniform(8, 2.0, dtype="f32")
    met = ma.Metropolis(chains32, pool=[_gauss(np.float32([0.1]), 0.5), _gauss(np.float32([0.7]), 0.5)], engine_factory=Recording)
    assert met.param_dtype == "f32" and Recording.last["param_dtype"] == "f32" and Recording.last["dtype"] == "f32"
    assert Recording.last["sigma"] == [float(np.float32(0.1)), float(np.float32(0.7))]
    met = ma.Metropolis(chains32, pool=[_gauss([0.1])], engine_factory=Recording)
    assert met.param_dtype == "f64" and "param_dtype" not in Recording.last                # today's callers: nothing new is passed
    with pytest.raises(ValueError, match="one type"):
        ma.Metropolis(chains32, pool=[_gauss(np.float32([0.1]), 0.5), _gauss([0.7], 0.5)], engine_factory=Recording)
    with pytest.raises(ValueError, match="Float32 chains"):
        ma.Metropolis(ma.ParticleChains.uniform(8, 2.0), pool=[_gauss(np.float32([0.1]))], engine_factory=Recording)


def test_config_struct_carries_param_dtype_in_the_old_reserved_slot():
    names = [f[0] for f in _capi.AmcConfig._fields_]
    assert names[-2:] == ["state_dtype", "param_dtype"] and "reserved" not in names
    assert C.sizeof(_capi.AmcConfig) == 96 and _capi.AmcConfig.param_dtype.offset == 92 and _capi.AmcConfig.param_dtype.size == 4


def test_engine_refuses_unknown_param_dtype_before_touching_a_device():
    with pytest.raises(_capi.AmcError, match="param_dtype"):
        _capi.HipEngine(n_chains=4, param_dtype="f16")


def test_checkpoint_names_the_parameter_type_and_restore_refuses_the_other(tmp_path):
    from montecarlo_amd import storage

    class Eng(Recording):
        step = 0
        estimator_step = 0

        def download_state(self, want_e=True):
            return np.zeros(8), None

        def counter_totals(self):
            return np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)

        def download_counters(self):
            return np.zeros((1, 8), dtype=np.int64), np.zeros((1, 8), dtype=np.int64)

    chains = ma.ParticleChains.uniform(8, 2.0, dtype="f32")
    met32 = ma.Metropolis(chains, pool=[_gauss(np.float32([0.1]))], engine_factory=Eng)
    fn = storage.checkpoint(met32, str(tmp_path))
    assert str(np.load(fn)["param_dtype"]) == "f32"
    met64 = ma.Metropolis(ma.ParticleChains.uniform(8, 2.0, dtype="f32"), pool=[_gauss([float(np.float32(0.1))])], engine_factory=Eng)
    with pytest.raises(ValueError, match="param_dtype"):
        storage.restore(met64, str(tmp_path))
