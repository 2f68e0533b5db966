"""Choosing the next beta of a population-annealing run, without a GPU (DESIGN.md section 3.14 "Choosing the next beta"): the host
twin's own invariants, the step it chooses against the closed form of a Gaussian population, and the Python layer
(PopulationAnnealing(adaptive=...) over the engine_factory seam: reaching beta_end, the calls behind it, log Z, checkpoint / resume,
the refusals)."""
import ctypes as C
import io
import math

import numpy as np
import pytest

import montecarlo_amd as ma

import anneal_search_twin as S
import anneal_twin as A
import oracle_lib as O

POOL = lambda s=0.8: (ma.Move(ma.Displacement(), ma.StandardGaussian(), [s], 1.0),)


def start_x(M):
    ids = np.arange(M)
    return 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)


def rho_at(pot, x, step, f32):
    """rho of one step, from the twin's own sums with the extreme the rule takes for it."""
    ne = S.energies(pot, x, f32)
    ne_hi, ne_lo = S.extremes(ne)
    a_max = float(S.product(ne_hi if step > 0.0 else ne_lo, step, f32))
    return S.rho_of(S.sums(ne, step, a_max, f32), len(x))


# ---- the twin's invariants -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("beta,limit", [(0.5, 8.0), (3.0, 0.25)])
@pytest.mark.parametrize("M,potential,rounds", [(2, "harmonic", 3), (65, "double_well", 1), (257, "harmonic", 6), (1000, "double_well", 4)])
def test_bracket_invariants(oracle, M, potential, rounds, beta, limit, dtype):
    f32 = dtype == "f32"
    x = start_x(M)
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    pot = O._potential_id(potential)
    target = 0.8
    b, diag, trace = S.next_beta(pot, x, beta, limit, target, rounds, f32)
    D = S.span(beta, limit, f32)
    status, done, step, rho_lo, hi, rho_hi = diag[0], diag[1], A.bits_f64(diag[2]), A.bits_f64(diag[3]), A.bits_f64(diag[4]), A.bits_f64(diag[5])
    assert min(beta, limit) <= b <= max(beta, limit)                 # the answer lies between beta and the limit
    if status == S.LIMIT:
        assert b == limit and done == 1 and all(S.rho_of(s, M) >= target for s in trace[0])
        return
    assert status in (S.OK, S.BELOW_RESOLUTION) and done == rounds
    assert rho_hi < target and rho_at(pot, x, hi, f32) == rho_hi     # hi fails
    lo = step if status == S.OK else 0.0
    if status == S.OK:
        assert rho_lo >= target and rho_at(pot, x, lo, f32) == rho_lo   # lo passes
    else:
        assert rho_lo == 1.0 and step == hi                          # rho(0) = 1 by definition; the smallest step resolved is taken
    # |hi - lo| <= |D| 8^-R: each round keeps one of eight parts of the bracket, each rounded once to T
    eps = 2.0 ** -23 if f32 else 2.0 ** -52
    assert abs(hi - lo) <= abs(D) * 8.0 ** -rounds + 2.0 * rounds * eps * abs(D)
    assert (hi > lo) == (D > 0.0) and abs(lo) < abs(hi) <= abs(D)
    T = np.float32 if f32 else np.float64
    assert b == float(T(beta) + T(step)) or b == limit


def test_one_chain_always_reaches_the_limit(oracle):
    for beta, limit in ((0.5, 40.0), (40.0, 0.5)):
        b, diag, trace = S.next_beta(O._potential_id("double_well"), np.array([1.7]), beta, limit, 0.999, 2, False)
        assert b == limit and diag[0] == S.LIMIT and diag[1] == 1
        assert all(s == [2 ** 30, 2 ** 30, 0] for s in trace[0]) and all(s == [0, 0, 0] for s in trace[1])


def test_statuses_of_the_twin(oracle):
    pot = O._potential_id("harmonic")
    x = start_x(50)
    assert S.next_beta(pot, x, 1.5, 1.5, 0.5, 3, False)[:2] == (1.5, [S.LIMIT, 0, 0, 0, 0, 0, 0, 0])            # D = 0
    b, diag, trace = S.next_beta(pot, np.full(7, np.nan), 1.0, 2.0, 0.5, 2, False)
    assert b == 2.0 and diag[0] == S.ALL_NAN and diag[6] == diag[7] == S.NAN_BITS and not np.any(np.array(trace))
    x[3] = np.inf                                                     # e = +Inf: heating gives it a = +Inf
    b, diag, _ = S.next_beta(pot, x, 2.0, 1.0, 0.5, 2, False)
    assert b == 1.0 and diag[0] == S.INF and diag[1] == 0
    b, diag, _ = S.next_beta(pot, x, 1.0, 2.0, 0.5, 2, False)          # cooling: the chain has no weight, the search goes on
    assert diag[0] in (S.OK, S.LIMIT) and 1.0 < b <= 2.0
    b, diag, _ = S.next_beta(pot, np.full(4, np.inf), 1.0, 2.0, 0.5, 2, False)
    assert b == 2.0 and diag[0] == S.NO_WEIGHT
    x = np.full(300, 30.0)
    x[17] = 0.0                                                       # one dominant chain: e = 900 against e = 0
    b, diag, _ = S.next_beta(pot, x, 0.5, 2.0, 0.5, 2, False)
    assert diag[0] == S.BELOW_RESOLUTION and A.bits_f64(diag[2]) == 1.5 / 64.0 and b == 0.5 + 1.5 / 64.0
    x[x > 0.0] = 1.0e10                                               # e = 1e20: even a step of 2^-53 leaves the others no weight
    b, diag, _ = S.next_beta(pot, x, 1.0, 1.0 + 2.0 ** -50, 0.5, 1, False)
    assert diag[0] == S.STALLED and b == 1.0 and A.bits_f64(diag[2]) == 2.0 ** -53      # the smallest step resolved does not change beta


# ---- a Gaussian population against the closed form ----------------------------------------------------------------------------------------
def gaussian_rho(r):
    """ESS / M of reweighting e = x^2 at beta by exp(-Delta e), r = Delta / beta: E[w^k] = (1 + k r)^(-1/2)."""
    return math.sqrt(1.0 + 2.0 * r) / (1.0 + r)


@pytest.mark.parametrize("seed,target", [(11, 0.9), (12, 0.75)])
def test_gaussian_population_against_the_closed_form(oracle, seed, target):
    """x ~ N(0, 1 / (2 beta)) under e = x^2: rho(r) = sqrt(1 + 2 r) / (1 + r) falls from 1, and the search returns the r at which the
    SAMPLE's rho crosses the target.  The sample's rho at the exact root r* differs from rho(r*) by its sampling error: with
    m_k = mean(w^k), rho = m_1^2 / m_2 has the first-order variance (delta method)
        var = [4 mu_1^2 / mu_2^2 Var(w) + mu_1^4 / mu_2^4 Var(w^2) - 4 mu_1^3 / mu_2^3 Cov(w, w^2)] / M,    mu_k = (1 + k r*)^(-1/2),
    and the root moves by that error over |rho'(r*)| = r* / (sqrt(1 + 2 r*) (1 + r*)^2).  Tolerance on r: FIVE such standard
    deviations (a correct search fails about once in 10^6 samples) plus the width of the final bracket, span 8^-rounds / beta."""
    M, beta, limit, rounds = 4000, 1.0, 5.0, 6
    lo, hi = 0.0, 4.0
    for _ in range(200):                                              # the root of rho(r) = target by bisection (rho decreases)
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if gaussian_rho(mid) >= target else (lo, mid)
    root = 0.5 * (lo + hi)
    mu = [None] + [(1.0 + k * root) ** -0.5 for k in (1, 2, 3, 4)]
    var = (4.0 * mu[1] ** 2 / mu[2] ** 2 * (mu[2] - mu[1] ** 2) + mu[1] ** 4 / mu[2] ** 4 * (mu[4] - mu[2] ** 2)
           - 4.0 * mu[1] ** 3 / mu[2] ** 3 * (mu[3] - mu[1] * mu[2])) / M
    slope = root / (math.sqrt(1.0 + 2.0 * root) * (1.0 + root) ** 2)
    tol = 5.0 * math.sqrt(var) / slope + (limit - beta) * 8.0 ** -rounds / beta
    x = np.random.default_rng(seed).normal(0.0, math.sqrt(1.0 / (2.0 * beta)), M)
    b, diag, _ = S.next_beta(O._potential_id("harmonic"), x, beta, limit, target, rounds, False)
    got = A.bits_f64(diag[2]) / beta
    print(f"target {target}: chosen r = {got!r}, root of the closed form {root!r}, tolerance {tol!r} (sigma_rho = {math.sqrt(var)!r})")
    assert diag[0] == S.OK and b == beta + A.bits_f64(diag[2])
    assert abs(got - root) <= tol


# ---- the C ABI's argument checks (no device is touched) ----------------------------------------------------------------------------------
def test_the_entry_refuses_null_arguments(amc):
    lib = amc.load()
    res, args = amc.SIGNATURES["amc_anneal_next_beta"]
    assert args[1:4] == [C.c_double, C.c_double, C.c_int] and res is C.c_int
    out = C.c_double(0.0)
    assert lib.amc_anneal_next_beta(None, 2.0, 0.5, 6, C.byref(out), None, None) == -1 and b"amc_anneal_next_beta" in lib.amc_last_error()
    assert amc.AMC_ANNEAL_SEARCH_CANDIDATES == S.CANDIDATES and amc.AMC_ANNEAL_SEARCH_WORDS == S.WORDS
    assert amc.AMC_ANNEAL_SEARCH_MAX_ROUNDS == S.MAX_ROUNDS and amc.AMC_ANNEAL_SEARCH_STALLED == S.STALLED
    assert ma.ANNEAL_SEARCH_STATUS[S.BELOW_RESOLUTION] == "BELOW_RESOLUTION" and len(ma.ANNEAL_SEARCH_STATUS) == 7


# ---- the Python layer over the engine_factory seam ----------------------------------------------------------------------------------------
def build(path, steps, adaptive, *, every=2, beta=0.5, families=False, M=64, potential="double_well", x=None, callbacks=(),
          factory=S.AnnealSearchTwinEngine, seed=4, sigma=0.5, **pa):
    chains = ma.ParticleChains(M, beta, potential, x=x) if x is not None else ma.ParticleChains.uniform(M, beta, potential=potential)
    al = [dict(algorithm=ma.Metropolis, pool=POOL(sigma), seed=seed, engine_factory=factory),
          dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, every),
               adaptive=adaptive, families=families, **pa)]
    if callbacks:
        al.append(dict(algorithm=ma.StoreCallbacks, callbacks=tuple(callbacks), scheduler=ma.build_schedule(steps, 0, every)))
    return ma.Simulation(chains, al, steps, path=str(path))


def test_adaptive_run_reaches_the_end_and_then_rests(oracle, tmp_path):
    plan = dict(beta_end=2.5, target=0.8, rounds=3)
    sim = build(tmp_path, 40, plan, families=True, callbacks=(ma.callback_anneal_beta, ma.callback_anneal_log_z))
    pa, eng = sim.algorithms[1], sim.algorithms[0].engine
    assert not pa.finished
    ma.run(sim)
    rec, log = pa.records(), pa.search_log()
    n = rec.shape[0]
    assert pa.finished and pa.beta == 2.5 and sim.chains.beta == 2.5 and A.f64_bits(eng.beta) == A.f64_bits(2.5)     # bit for bit
    assert 2 <= n < 20 and eng.anneal_step == n and log.shape == (n, 8)         # 20 calls were due: the later ones appended nothing
    assert log[-1, 0] == S.LIMIT and set(log[:-1, 0].tolist()) <= {S.OK, S.BELOW_RESOLUTION}
    done = pa.betas_done()
    assert np.all(np.diff(np.concatenate([[0.5], done])) > 0.0) and done[-1] == 2.5
    # every step kept the target: rho at the step chosen, from the search's own record
    assert all(A.bits_f64(r[3]) >= 0.8 for r in log)
    assert np.all(np.isfinite(pa.log_z())) and pa.survival().shape == (n,)
    # a further scheduled call launches nothing
    x = eng.download_state()[0].copy()
    pa.make_step(sim)
    assert pa.records().shape[0] == n and pa.search_log().shape[0] == n and eng.anneal_step == n
    assert np.array_equal(eng.download_state()[0].view(np.uint64), x.view(np.uint64))
    rows = [ln.split() for ln in open(tmp_path / "anneal_beta.dat").read().splitlines()]
    assert [float(r[-1]) for r in rows[-3:]] == [2.5, 2.5, 2.5]
    # the same run stepped by hand on a twin of its own
    ref = S.AnnealSearchTwinEngine(n_chains=64, potential="double_well", beta=0.5, sigma=[0.5], weight=[1.0], seed=4)
    ref.init_uniform(-2.0, 2.0)
    while ref.beta != 2.5:
        ref.sweep(2)
        ref.anneal(ref.anneal_next_beta(2.5, 0.8, 3)[0])
    assert np.array_equal(ref.anneal_records(), rec)
    buf = io.StringIO()
    pa.write_algorithm(buf, ma.build_schedule(40, 0, 2))
    assert "Calls: 20\n\t\tBetas: adaptive, ESS / M >= 0.8 per step, to 2.5 (3 rounds)\n" in buf.getvalue()


def test_heating_run(oracle, tmp_path):
    sim = build(tmp_path, 30, dict(beta_end=0.25, target=0.7), beta=3.0, M=65)
    ma.run(sim)
    pa = sim.algorithms[1]
    done = pa.betas_done()
    assert pa.finished and pa.beta == 0.25 and np.all(np.diff(np.concatenate([[3.0], done])) < 0.0)
    assert pa.adaptive == dict(beta_end=0.25, target=0.7, rounds=6)


# ---- log Z of the harmonic well from an adaptive run --------------------------------------------------------------------------------------
LOGZ_M, LOGZ_EVERY, LOGZ_STEPS = 2000, 4, 48
LOGZ_FROM, LOGZ_TO = 0.5, 4.0
LOGZ_PLAN = dict(beta_end=LOGZ_TO, target=0.85, rounds=4)
LOGZ_SPREAD = 0.01994                                           # measured, see the test's docstring
LOGZ_TOL = 5.0 * LOGZ_SPREAD


def adaptive_log_z(path, seed):
    x = np.random.default_rng(seed).normal(0.0, math.sqrt(1.0 / (2.0 * LOGZ_FROM)), LOGZ_M)      # equilibrium at the first beta: e = x^2
    sim = build(path, LOGZ_STEPS, LOGZ_PLAN, every=LOGZ_EVERY, beta=LOGZ_FROM, M=LOGZ_M, potential="harmonic", x=x, seed=seed, sigma=0.8)
    ma.run(sim)
    pa = sim.algorithms[1]
    assert pa.finished
    return float(pa.log_z()[-1]), pa.records().shape[0]


@pytest.mark.parametrize("seed", [101, 202])
def test_log_z_of_the_harmonic_well(oracle, tmp_path, seed):
    """log(Z(4) / Z(0.5)) = log(0.5 / 4) / 2 for e = x^2, from one adaptive run of 2000 chains (target 0.85, 4 rounds) with 4 sweeps
    (sigma = 0.8) between the steps, by the method of test_anneal_host.test_log_z_of_the_harmonic_well: the tolerance is the twin's own
    spread.  Over the 24 seeds 1 .. 24 at this population size the estimate (three steps in every run) has mean -1.03374 (exact: -1.03972) and standard
    deviation 0.01994 (sample, n - 1); five standard deviations, 0.0997, so that a correct twin fails about once in 10^6 runs."""
    got, n = adaptive_log_z(tmp_path, seed)
    want = 0.5 * math.log(LOGZ_FROM / LOGZ_TO)
    print(f"log Z estimate {got!r} from {n} steps, exact {want!r}, tolerance {LOGZ_TOL}")
    assert abs(got - want) <= LOGZ_TOL


# ---- checkpoint / resume ------------------------------------------------------------------------------------------------------------------
def test_a_resumed_adaptive_run_ends_on_the_same_bits(oracle, tmp_path):
    plan = dict(beta_end=3.0, target=0.97, rounds=3)
    whole = build(tmp_path / "w", 40, plan, families=True)
    ma.run(whole)
    first = build(tmp_path / "a", 6, plan, families=True)             # stops three steps in, far from the end
    ma.run(first)
    assert not first.algorithms[1].finished and first.algorithms[1].records().shape[0] == 3
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    second = build(tmp_path / "b", 34, plan, families=True)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    assert second.algorithms[1].beta == first.algorithms[1].beta and second.algorithms[0].engine.anneal_step == 3
    ma.run(second)
    e1, e2 = whole.algorithms[0].engine, second.algorithms[0].engine
    assert whole.algorithms[1].finished and second.algorithms[1].finished and e1.beta == e2.beta == 3.0
    assert np.array_equal(e1.download_state()[0].view(np.uint64), e2.download_state()[0].view(np.uint64))
    assert np.array_equal(whole.algorithms[1].records(), second.algorithms[1].records()) and e1.anneal_step == e2.anneal_step
    assert np.array_equal(e1.download_families(), e2.download_families())
    assert all(np.array_equal(a, b) for a, b in zip(e1.download_counters(), e2.download_counters()))
    n = whole.algorithms[1].records().shape[0]
    assert np.array_equal(whole.algorithms[1].search_log()[3:], second.algorithms[1].search_log()) and n > 4


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_adaptive_argument(oracle, tmp_path):
    good = dict(beta_end=2.0, target=0.5)
    with pytest.raises(ValueError, match="PopulationAnnealing: both betas and adaptive are given"):
        build(tmp_path / "a", 4, good, betas=[1.0, 2.0])
    with pytest.raises(ValueError, match="PopulationAnnealing: betas is missing"):
        build(tmp_path / "b", 4, None)
    with pytest.raises(ValueError, match=r"adaptive\['target'\] is missing \(it has no default\)"):
        build(tmp_path / "c", 4, dict(beta_end=2.0))
    with pytest.raises(ValueError, match=r"adaptive\['beta_end'\] is missing"):
        build(tmp_path / "d", 4, dict(target=0.5))
    for bad in (0.0, 1.0, -0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match=r"adaptive\['target'\] = .* must lie strictly between 0 and 1"):
            build(tmp_path / "e", 4, dict(beta_end=2.0, target=bad))
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError, match=r"adaptive\['rounds'\] = .* must be an integer in \[1, 16\]"):
            build(tmp_path / "f", 4, dict(good, rounds=bad))
    with pytest.raises(ValueError, match=r"adaptive\['beta_end'\] = inf is not finite"):
        build(tmp_path / "g", 4, dict(beta_end=math.inf, target=0.5))
    with pytest.raises(ValueError, match=r"adaptive has unknown keys \['beta'\]"):
        build(tmp_path / "h", 4, dict(good, beta=3.0))
    with pytest.raises(ValueError, match="adaptive = 3 is not a dict"):
        build(tmp_path / "i", 4, 3)
    with pytest.raises(ValueError, match="PopulationAnnealing: this engine cannot choose the next beta"):
        build(tmp_path / "j", 4, good, factory=A.AnnealTwinEngine)
    with pytest.raises(ValueError, match=r"PopulationAnnealing: this engine has no annealing step \(streams > 1"):
        build(tmp_path / "k", 4, good, factory=O.OracleEngine)
    ladder = ma.ParticleChains.ladder(8, [0.5, 1.0], potential="harmonic")
    with pytest.raises(ValueError, match="PopulationAnnealing: the chains carry a per-chain beta array"):
        ma.Simulation(ladder, [dict(algorithm=ma.Metropolis, pool=POOL(), seed=4, engine_factory=S.AnnealSearchTwinEngine),
                               dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=[2], adaptive=good)], 4,
                      path=str(tmp_path / "l"))


def test_a_stalled_search_raises(oracle, tmp_path):
    x = np.full(64, 1.0e10)
    x[5] = 0.0                                                        # one dominant chain (e = 1e20 against 0): every candidate fails, and 1 + 2^-53 is 1
    sim = build(tmp_path, 4, dict(beta_end=1.0 + 2.0 ** -50, target=0.5, rounds=1), beta=1.0, potential="harmonic", x=x)
    with pytest.raises(ValueError, match="PopulationAnnealing: the search stalled at beta = 1.0"):
        ma.run(sim)
    assert sim.algorithms[0].engine.anneal_step == 0 and sim.algorithms[1].search_log().shape == (0, 8)
