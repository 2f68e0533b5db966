"""K == 1 harmonic sweeps whose accept filter takes -beta delta (x + xn) in Float32 in the place of the exact dlogp (amc_model.h,
harmonic_filter_y), and the forms that keep the exact dlogp beside them: every form, on ensembles inside, across and outside the guard, is bit-equal to the oracle and to the same
handle with every decision forced through accept_exact (AMC_EXACT_ACCEPT); and the device's y equals the numpy model's bit for bit."""
import numpy as np
import pytest

import filter_argument_model as F

pytestmark = pytest.mark.gpu

M = (1 << 16) + 3          # odd: a ragged last block and a lone last chain
STEPS = 8


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _x0(kind, rng, beta):
    if kind == "uniform":
        return rng.uniform(-2, 2, M)
    if kind == "log_uniform":                      # +-[2^8, 2^60]: straddles the guard
        return np.sign(rng.standard_normal(M)) * 2.0 ** rng.uniform(8, 60, M)
    if kind == "at_the_bound":                     # |s| = |2 x + delta| around L: x at L / 2, one ulp below, one above, both signs
        L = 2.0 ** F.setup(beta, 2.0 ** -30)[2]
        v = np.array([L / 2, np.nextafter(L / 2, 0), np.nextafter(L / 2, np.inf)])
        return np.tile(np.concatenate([v, -v]), M // 6 + 1)[:M]
    assert kind == "special"
    v = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1040, 1.5, -0.25])
    return np.tile(v, M // len(v) + 1)[:M]


# (x0, sigma, beta): one thing away from the base ensemble at a time
BASE = ("uniform", 0.1, 2.0)
ENSEMBLES = [BASE, ("log_uniform", 0.1, 2.0), ("at_the_bound", 0.1, 2.0), ("special", 0.1, 2.0)]
ENSEMBLES += [("uniform", s, 2.0) for s in (1e-3, 3.0, 1e6)]
ENSEMBLES += [("uniform", 0.1, b) for b in (0.0, 2.0 ** -20, 2.0 ** 10, 2.0 ** 11, np.inf)]
# On the product form: K == 1 with one beta -- the pool-wide counter (sweep_kernel without the step log), per-chain counters (with it),
# and the fused PGMC time steps of both (pg_estimate_kernel, SWEEP == 3 / 1: several steps, so a learning step changes sigma
# before the launch that follows forms its filter constants).  On the exact dlogp beside them: a beta array, K == 2.
FORMS = ["k1_pool_counter", "k1_chain_counters", "k1_beta_array", "k2", "pgmc_step", "pgmc_k1_pool_counter", "pgmc_k1_chain_counters"]
PGMC_STEPS = 3


def _run(factory, form, x0, sigma, beta, pgmc_steps=PGMC_STEPS, **extra):
    k2 = form in ("k2", "pgmc_step")
    kw = dict(n_chains=M, potential="harmonic", beta=beta, sigma=[sigma, sigma / 2] if k2 else [sigma],
              weight=[0.6, 0.4] if k2 else [1.0], seed=41, **extra)
    if form in ("k1_pool_counter", "pgmc_k1_pool_counter"):
        kw["per_chain_counters"] = False
    e = factory(**kw)
    e.upload_state(x0, np.full(M, beta) if form == "k1_beta_array" else None)
    if form == "pgmc_step":
        e.pgmc_steps(1, [1], 2, [1], [0.05], [0.0])
    elif form.startswith("pgmc_k1"):
        e.sweep(1)
        e.pgmc_steps(pgmc_steps, [0], 2, [1], [0.05], [0.0])      # VPG on the pool's only move
    else:
        for _ in range(3):
            e.sweep(1)                               # single-sweep launches
        e.sweep(STEPS - 3)                           # and a fused one
    x, en = e.download_state()
    acc, tot = e.counter_totals()
    out = [bits(x), bits(en), np.asarray(acc), np.asarray(tot)]
    if kw.get("per_chain_counters", True):
        out += list(e.download_counters())           # the step log, folded
    e.close()
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ens", ENSEMBLES, ids=[f"{k}-s{s:g}-b{b:g}" for k, s, b in ENSEMBLES])
def test_forms_equal_the_oracle_and_the_exact_decision(gpu, oracle, monkeypatch, form, ens):
    kind, sigma, beta = ens
    x0 = _x0(kind, np.random.default_rng(7), beta)
    # Non-finite positions, and beta = Inf (0 * Inf in the summands), make the policy gradient NaN, and what a learning step does with a NaN gradient differs between the
    # engine and the oracle's twin in code this file is not about (the K == 2 form shows it too: sigma kept against sigma = NaN).
    # There the K == 1 time-step forms run ONE step, as the K == 2 form does: no learned sigma enters a proposal.
    n = 1 if kind == "special" or not np.isfinite(beta) else PGMC_STEPS
    got = _run(gpu.HipEngine, form, x0, sigma, beta, n)
    monkeypatch.setenv("AMC_EXACT_ACCEPT", "1")
    exact = _run(gpu.HipEngine, form, x0, sigma, beta, n)
    monkeypatch.delenv("AMC_EXACT_ACCEPT")
    want = _run(oracle.OracleEngine, form, x0, sigma, beta, n)
    for i, (g, x, w) in enumerate(zip(got, exact, want)):
        assert np.array_equal(g, x), f"{form}: output {i} differs from the run with every decision by accept_exact"
        assert np.array_equal(g, w), f"{form}: output {i} differs from the oracle"


def test_device_argument_equals_the_model(gpu):
    rng = np.random.default_rng(11)
    n = 1 << 16
    for beta, sigma in ((2.0, 0.1), (2.0 ** 10, 3.0), (2.0 ** -20, 1e-3), (2.0, 1e6), (np.inf, 0.1), (0.0, 0.1), (2.0 ** 11, 0.1)):
        L = 2.0 ** F.setup(beta, 2.0 ** -30)[2] if np.isfinite(beta) else 2.0 ** 13
        x = rng.uniform(-1, 1, n) * 2.0 ** rng.uniform(-20, np.log2(L) + 1, n)          # both sides of the guard
        d = sigma * np.clip(rng.standard_normal(n), -8.5, 8.5)
        x[:8] = [np.inf, -np.inf, np.nan, 0.0, -0.0, L / 2, np.nextafter(L / 2, 0), -L / 2]
        d[8:12] = [0.0, -0.0, 2.0 ** -100, L]
        got = gpu.selftest_filter_argument(beta, sigma, x, d)
        want = F.y_model(x, d, beta, sigma)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (beta, sigma)
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), (beta, sigma)
