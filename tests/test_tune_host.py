"""Tuning the widths per rung (DESIGN.md section 3.13 "Tuning the widths"), the parts that need no GPU: the rule on its host twin
(tests/tune_twin.py) by hand and against the product's own inline function run on the CPU (tests/aux/tune_rule_host.cpp, under the
address and undefined-behaviour sanitizers), the contraction of the map with the closed-form acceptance of the harmonic well, and
the Python layer -- every ValueError, the scheduled algorithm, the checkpoint fields -- over an engine double.  The device side is
tests/test_gpu_tune.py: the device is bit-equal to this twin."""
import os
import subprocess

import numpy as np
import pytest

import montecarlo_amd as ma

import exchange_twin as X
import tune_twin as TT

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "montecarlo_amd", "csrc")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- worked by hand (dyadic rationals: the arithmetic is exact) ------------------------------------------------------------------------
def test_the_rule_by_hand():
    # a = 3/4, q = 1.5, v = 1 + 1 (1.5 - 1) = 1.5; half the step with gamma = 0.5
    assert TT.tune_rule(1.0, 3, 4, 0.5, 1.0, 1) == (0, 1.5)
    assert TT.tune_rule(1.0, 3, 4, 0.5, 0.5, 1) == (0, 1.25)
    # a = 1/8, q = 0.25 -> 0.5: at most a factor of two down; a = 1, q = 4 -> 2: at most a factor of two up
    assert TT.tune_rule(2.0, 1, 8, 0.5, 1.0, 1) == (0, 1.0)
    assert TT.tune_rule(2.0, 8, 8, 0.25, 1.0, 1) == (0, 4.0)
    # a == target: the width is a fixed point, bit for bit
    assert TT.tune_rule(0.30000000000000004, 11, 25, 0.44, 1.0, 1)[0] == 0
    assert TT.tune_rule(0.7, 1, 2, 0.5, 0.3, 1) == (0, 0.7)
    # the statuses
    assert TT.tune_rule(0.7, 0, 0, 0.5, 1.0, 1) == (1, 0.7) and TT.tune_rule(0.7, 3, 9, 0.5, 1.0, 10) == (1, 0.7)
    assert TT.tune_rule(0.7, 5, 4, 0.5, 1.0, 1) == (2, 0.7) and TT.tune_rule(0.7, 1, 4, 0.5, 1.0, 1, inconsistent=True) == (2, 0.7)
    assert TT.tune_rule(1.0, 3, 4, 0.5, 1.0, 1, 0.1, 1.25) == (3, 1.25) and TT.tune_rule(2.0, 0, 8, 0.5, 1.0, 1, 1.5, 9.0) == (3, 1.5)


# ---- the product's own rule on the CPU, under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_host(tmp_path_factory):
    """run(entries, target, gamma, min_calls, lo, hi) -> [(status, out)] of tests/aux/tune_rule_host.cpp, which calls amc_tune.h's
    tune_rule; built once, with -fsanitize=address,undefined: a stand-alone program, nothing is loaded into this process."""
    d = tmp_path_factory.mktemp("tune_rule")
    exe = str(d / "tune_rule_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "aux", "tune_rule_host.cpp"), "-o", exe], check=True, capture_output=True)

    def run(entries, target, gamma, min_calls, lo, hi):
        text = "".join(f"{float(s).hex()} {int(A)} {int(T)} {int(bool(bad))}\n" for s, A, T, bad in entries)
        r = subprocess.run([exe, float(target).hex(), float(gamma).hex(), float(lo).hex(), float(hi).hex(), str(int(min_calls))], input=text,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [ln.split() for ln in r.stdout.splitlines()]
        assert len(rows) == len(entries)
        return [(int(st), float.fromhex(v)) for st, v in rows]
    return run


def edge_entries(target, min_calls):
    out = []
    for s in (1e-100, 1e100, 0.5, 0.30000000000000004, 3.7e-3):
        for T in (0, min_calls - 1, min_calls, min_calls + 1, 1000, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1025, 2 ** 64 - 1):
            T = max(T, 0)
            for A in (0, T, min(T + 1, 2 ** 64 - 1), T // 2, T // 3, (2 ** 63 - 513) if T >= 2 ** 63 else T // 7):
                out.append((s, A, T, False))
        out.append((s, 10, 100, True))
    # q exactly 0.5 and 2.0 (target 0.5: a = 0.25 and a = 1), and just inside / outside
    for A, T in ((1, 4), (4, 4), (256, 1024), (255, 1024), (257, 1024), (1023, 1024)):
        out.append((0.7, A * 1000, T * 1000, False))
    return out


def test_the_inline_rule_equals_the_twin_on_the_cpu(rule_host):
    rng = np.random.default_rng(91)
    seen = set()
    configs = [(0.5, 1.0, 1000, 1e-100, 1e100), (0.44, 0.3, 1, 1e-100, 1e100), (0.5, 1.0, 1, 0.4, 0.6), (0.234, 0.0625, 50, 1e-3, 10.0),
               (0.44, 1.0, 1, 1e-100, 1e-100), (0.44, 1.0, 1, 1e100, 1e100)]
    for target, gamma, min_calls, lo, hi in configs:
        entries = edge_entries(target, min_calls)
        for _ in range(700):
            T = int(rng.integers(0, 10 ** int(rng.integers(1, 19))))
            A = int(T * rng.random()) if rng.random() < 0.9 else T + int(rng.integers(0, 3))
            s = float(10.0 ** rng.uniform(-100, 100)) if rng.random() < 0.3 else float(rng.uniform(1e-3, 5.0))
            entries.append((s, A, T, rng.random() < 0.03))
        got = rule_host(entries, target, gamma, min_calls, lo, hi)
        for (s, A, T, bad), (st_c, out_c) in zip(entries, got):
            st, out = TT.tune_rule(s, A, T, target, gamma, min_calls, lo, hi, bad)
            seen.add(st)
            assert st_c == st and bits(out_c) == bits(out), (s, A, T, bad, target, gamma, min_calls, lo, hi, st, st_c, out, out_c)
            if st in (1, 2):
                assert bits(out) == bits(s)
    assert seen == {0, 1, 2, 3}


# ---- the map contracts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [0.5, 0.44, 0.234])
@pytest.mark.parametrize("start", [0.01, 100.0])
def test_the_map_converges_monotonically(target, start):
    """sigma <- sigma a(sigma) / target with a(sigma) = (2 / pi) atan(c / sigma), the harmonic well's closed form: g' = 1 - (u / (1 + u^2)) /
    atan(u), u = c / sigma, lies in (0, 1) everywhere, so after the clamped phase (a factor of two per call) the error keeps its sign and
    shrinks by a ratio below 1 at every call.  Derived, not measured: the ratio tends to g' at the fixed point (0.363 at a = 0.5)."""
    beta = 1.3
    c = np.sqrt(2.0 / beta)
    fixed = c / np.tan(np.pi * target / 2.0)
    s = start * c
    errs, clamped = [], []
    for _ in range(40):
        a = float(TT.harmonic_acceptance(s, beta))
        clamped.append(not 0.5 <= a / target <= 2.0)
        n = 10 ** 15
        st, s = TT.tune_rule(s, round(a * n), n, target, 1.0, 1)
        assert st == 0
        errs.append(float(s) - fixed)
    first = clamped.index(False)
    assert not any(clamped[first:])                  # (the clamped phase, which may be empty -- a <= 1 keeps q <= 2 at target 0.5 --, never returns)
    free = [e for e in errs[first:] if abs(e) > 1e-9 * fixed]
    assert len(free) >= 5
    assert all(np.sign(e) == np.sign(free[0]) for e in free)
    ratios = [b / a for a, b in zip(free, free[1:])]
    assert all(0.0 < r < 1.0 for r in ratios), ratios
    u = c / fixed
    assert abs(ratios[-1] - (1.0 - (u / (1.0 + u * u)) / np.arctan(u))) < 1e-3
    if target == 0.5:
        assert abs(ratios[-1] - 0.3634) < 1e-3


# ---- the C ABI's argument checks that come before any device --------------------------------------------------------------------------
def test_null_handles_are_refused(amc):
    lib = amc.load()
    assert lib.amc_tune_rung_sigma(None, 0.5, 1.0, 1, 1e-3, 1e3, None) == -1 and b"amc_tune_rung_sigma" in lib.amc_last_error()
    assert lib.amc_tune_status(None, None, 0, None) == -1 and lib.amc_set_tuned(None, 0) == -1
    assert lib.amc_rung_window_counts(None, None, None) == -1 and lib.amc_rung_window_restart(None) == -1
    assert lib.amc_rung_window_base(None, None, None) == -1 and lib.amc_set_rung_window_base(None, None, None) == -1


# ---- the Python layer over an engine double -----------------------------------------------------------------------------------------------
class TuneEngine(X.TwinEngine):
    """TwinEngine with the table, window and tuning entries of HipEngine.  A double of the HOST logic only: the table it keeps is tuned
    by the twin's rule from the twin's counters; its sweeps go on with the pool's sigma."""

    table = None

    def set_ladder(self, n_rungs):
        super().set_ladder(n_rungs)
        self.table, self.base, self.n_tuned_, self.st = None, None, 0, None

    def set_rung_sigma(self, sigma):
        self.table = None if sigma is None else np.array(sigma, dtype=np.float64).reshape(self.n_moves, self.n_rungs)
        self.n_tuned_, self.st = 0, None

    def rung_sigma(self):
        assert self.table is not None
        return self.table.copy()

    def rung_counter_totals(self):
        acc, tot = self.download_counters()
        return (acc.reshape(self.n_moves, -1, self.n_rungs).sum(axis=1), tot.reshape(self.n_moves, -1, self.n_rungs).sum(axis=1))

    def _base(self):
        return np.zeros((2, self.n_moves, self.n_rungs), dtype=np.int64) if self.base is None else self.base

    def rung_window_counts(self):
        acc, tot = self.rung_counter_totals()
        b = self._base()
        bad = (acc < b[0]) | (tot < b[1])
        return np.where(bad, -1, acc - b[0]), np.where(bad, -1, tot - b[1])

    def rung_window_restart(self):
        self.base = np.array(self.rung_counter_totals())

    def rung_window_base(self):
        b = self._base()
        return b[0].copy(), b[1].copy()

    def set_rung_window_base(self, acc, tot):
        self.base = np.array([acc, tot], dtype=np.int64).reshape(2, self.n_moves, self.n_rungs)

    def tune_rung_sigma(self, target, gamma, min_calls, lo, hi, counts=None):
        A, T = self.rung_window_counts() if counts is None else counts
        self.st = np.zeros(self.table.shape, dtype=np.int64)
        for i in np.ndindex(*self.table.shape):
            self.st[i], self.table[i] = TT.tune_rule(self.table[i], max(A[i], 0), max(T[i], 0), target, gamma, min_calls, lo, hi, A[i] < 0)
        self.n_tuned_ += int(np.any((self.st == 0) | (self.st == 3)))
        self.rung_window_restart()

    def tune_status(self):
        return (np.zeros(self.table.shape, dtype=np.int64) if self.st is None else self.st.copy()), self.n_tuned_

    def set_tuned(self, n):
        self.n_tuned_ = int(n)


TAB = np.array([[0.5, 0.4, 0.3], [0.2, 0.15, 0.1]])


def _sim(path, steps, tab=TAB, tune=None, store=False):
    chains = ma.ParticleChains.ladder(6, [0.5, 1.0, 2.0], x=np.linspace(-1.5, 1.5, 18))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 0.625), ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.2], 0.375))
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=7, engine_factory=TuneEngine, rung_sigma=tab),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2))]
    if tune is not None:
        al.append(dict(algorithm=ma.TuneRungSigma, dependencies=(ma.Metropolis,), **tune))
    if store:
        al.append(dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_rung_sigma, ma.callback_rung_window_acceptance),
                       scheduler=ma.build_schedule(steps, 0, 4)))
    return ma.Simulation(chains, al, steps, path=str(path))


@pytest.mark.parametrize("kw,words", [
    (dict(target=0.0), "target"), (dict(target=1.0), "target"), (dict(target=np.nan), "target"),
    (dict(gamma=0.0), "gamma"), (dict(gamma=1.5), "gamma"), (dict(gamma=np.nan), "gamma"),
    (dict(min_calls=0), "min_calls"), (dict(min_calls=2.5), "min_calls"),
    (dict(sigma_min=0.0), "sigma_min"), (dict(sigma_max=1e101), "sigma_max"), (dict(sigma_min=2.0, sigma_max=1.0), "sigma_min"),
    (dict(sigma_min=np.nan), "sigma_min")])
def test_value_errors_of_the_python_layer(oracle, tmp_path, kw, words):
    sim = _sim(tmp_path, 4)
    ma.run(sim)
    met = sim.algorithms[0]
    before = met.engine.rung_sigma()
    with pytest.raises(ValueError, match=words):
        met.tune_rung_sigma(**kw)
    assert np.array_equal(met.engine.rung_sigma(), before) and met.engine.tune_status()[1] == 0
    with pytest.raises(ValueError, match="TuneRungSigma.*" + words):
        _sim(tmp_path / "b", 4, tune=dict(scheduler=[2], **kw))


def test_refusals_without_a_ladder_or_a_table(oracle, tmp_path):
    sim = _sim(tmp_path, 4, tab=None)
    met = sim.algorithms[0]
    for call in (met.tune_rung_sigma, met.rung_window_acceptance, met.restart_rung_window):
        with pytest.raises(ValueError, match="no ladder"):
            call()
    ma.run(sim)
    with pytest.raises(ValueError, match="no widths per rung"):
        met.tune_rung_sigma()
    with pytest.raises(ValueError, match="no widths per rung"):
        _sim(tmp_path / "b", 4, tab=None, tune=dict(scheduler=[2]))
    with pytest.raises(ValueError, match="no widths per rung"):
        ma.callback_rung_sigma(sim)
    assert met.rung_window_acceptance().shape == (2, 3)          # the window needs no table


def test_the_window_and_the_tuning_through_metropolis(oracle, tmp_path):
    sim = _sim(tmp_path, 12)
    ma.run(sim)
    met = sim.algorithms[0]
    acc, tot = met.engine.rung_counter_totals()
    assert np.array_equal(met.rung_window_acceptance(), acc / tot) and np.array_equal(met.rung_window_acceptance(), met.rung_acceptance())
    st = met.tune_rung_sigma(target=0.5, gamma=1.0, min_calls=1)
    want = np.array([[TT.tune_rule(TAB[i], acc[i], tot[i], 0.5, 1.0, 1)[1] for i in ((k, 0), (k, 1), (k, 2))] for k in range(2)])
    assert st.shape == (2, 3) and np.all(st == 0)
    assert np.array_equal(bits(met.rung_sigma), bits(want)) and np.array_equal(bits(ma.callback_rung_sigma(sim)), bits(want))
    assert np.all(np.isnan(met.rung_window_acceptance()))                          # an empty window: 0 / 0
    st = met.tune_rung_sigma(target=0.5, min_calls=1)
    assert np.all(st == 1) and np.array_equal(bits(met.rung_sigma), bits(want))
    # counters replaced behind the window: inconsistent cells are NaN, status 2, and keep their width
    met.engine.sweep(3)
    a, t = met.engine.download_counters()
    met.engine.upload_counters(np.where(np.arange(18) % 3 == 1, 0, a), t)
    wa = met.rung_window_acceptance()
    assert np.all(np.isnan(wa[:, 1])) and np.all(np.isfinite(wa[:, [0, 2]]))
    st = met.tune_rung_sigma(target=0.5, min_calls=1)
    assert np.all(st[:, 1] == 2) and np.all(st[:, [0, 2]] == 0) and np.array_equal(bits(met.rung_sigma[:, 1]), bits(want[:, 1]))


def test_the_algorithm_the_summary_and_the_callbacks(oracle, tmp_path):
    tune = dict(scheduler=[4, 8, 12, 16], target=0.5, gamma=0.5, min_calls=2, sigma_min=1e-3, sigma_max=10.0, until=12)
    runs = []
    for fuse in (True, False):
        sim = _sim(tmp_path / str(fuse), 16, tune=tune, store=True)
        ma.run(sim, fuse=fuse)
        runs.append(sim)
    a, b = (s.algorithms[0] for s in runs)
    assert np.array_equal(bits(a.rung_sigma), bits(b.rung_sigma)) and not np.array_equal(a.rung_sigma, TAB)
    assert np.array_equal(bits(a.engine.download_state()[0]), bits(b.engine.download_state()[0]))
    alg = runs[0].algorithms[2]
    assert [t for t, _ in alg.statuses] == [4, 8, 12] and a.engine.tune_status()[1] == 3           # until: no tuning at 16
    summary = open(tmp_path / "True" / "summary.log").read()
    for line in ("TuneRungSigma", "Target: 0.5", "Gamma: 0.5", "Min calls: 2", "Sigma min: 0.001", "Sigma max: 10.0", "Until: 12"):
        assert line in summary
    assert sorted(f for f in os.listdir(tmp_path / "True") if f.endswith(".dat")) == ["rung_sigma.dat", "rung_window_acceptance.dat"]


def test_checkpoints_carry_the_window_only_when_it_was_used(oracle, tmp_path):
    plain = _sim(tmp_path / "p", 6)
    ma.run(plain)
    ma.checkpoint(plain.algorithms[0], str(tmp_path / "ckp"))
    tuned = _sim(tmp_path / "t", 6, tune=dict(scheduler=[3], target=0.5, min_calls=1))
    ma.run(tuned)
    met = tuned.algorithms[0]
    ma.checkpoint(met, str(tmp_path / "ck"))
    p, t = np.load(tmp_path / "ckp" / "checkpoint_rank0.npz"), np.load(tmp_path / "ck" / "checkpoint_rank0.npz")
    assert set(t.files) - set(p.files) == {"rung_window_accepted", "rung_window_total", "n_tuned"}
    assert np.array_equal(bits(t["rung_sigma"]), bits(met.engine.table)) and int(t["n_tuned"]) == 1
    again = _sim(tmp_path / "r", 6, tune=dict(scheduler=[3], target=0.5, min_calls=1))
    m2 = again.algorithms[0]
    ma.restore(m2, str(tmp_path / "ck"))
    assert np.array_equal(bits(m2.engine.table), bits(met.engine.table)) and m2.engine.tune_status()[1] == 1
    assert all(np.array_equal(u, v) for u, v in zip(m2.engine.rung_window_base(), met.engine.rung_window_base()))
    again.algorithms[2].initialise(again)                      # a resumed run keeps the window it was given
    assert all(np.array_equal(u, v) for u, v in zip(m2.engine.rung_window_base(), met.engine.rung_window_base()))
