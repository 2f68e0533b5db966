"""Random operation walks over a handle with a temperature ladder, against the host twins composed into one reference object.

The ladder features (exchange steps, per-rung sums, walker tracking, widths per rung) and the sliced
single-sweep launches (section 6 "Slices") each have a twin and a test file of their own, and all of those walk one hand-written
sequence.  This module draws the configuration and the sequence:

    LadderReference   the surface of montecarlo_amd._capi.HipEngine that the walk uses, computed by the twins alone --
                      oracle_lib.OracleSim, f32_param_twin.TwinSim or rung_sigma_twin.RungSigmaTwin underneath, track_twin.TrackTwin
                      above, rung_sums_twin.records, track_twin.flow_counts, numpy for the bin rule and the strided counter sums.  What
                      set_ladder, set_rung_sigma(None), set_tracking and the setters reset or keep follows the text of DESIGN.md
                      section 3.13 and include/amc.h.  It shares no code with the product.
    draw_case         one configuration (a plain dict; x0 and beta are functions of it: make_state)
    run_walk          the operations, drawn one by one; both sides take each, the observers compare bit for bit / integer for integer
    run_case          engine and reference of a case, the walk, the comparison at the end

The engine side is anything with HipEngine's surface: the host tests run the walk with a second reference object in its place.
"""
import os

import numpy as np
import pytest

import exchange_twin as X
import f32_param_twin as F
import oracle_lib as O
import rung_sigma_twin as RT
import rung_sums_twin as RS
import track_twin as T

DEFAULT_CASES, DEFAULT_SEED = 40, 20261019       # drawn cases behind the pinned ones (AMC_LADDER_FUZZ_CASES, AMC_LADDER_FUZZ_SEED)
MAX_CHAINS = 6200
MAX_EXCHANGE_STEPS = 40          # per walk: the twin's exchange step is a Python loop over the gaps
T_X_LIMIT = 1 << 48              # amc_exchange refuses a step index that has reached 2^48
TWO32 = 1 << 32


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def hist_row(x, lo, hi, n_bins):
    """The bin rule of amc_histogram written out: NaN, < lo, >= hi, then min(int((x - lo) inv_w), n_bins - 1); a row is the bins,
    then below, at / above, NaN."""
    out = np.zeros(n_bins + 3, dtype=np.uint64)
    inv_w = n_bins / (hi - lo)
    nan = np.isnan(x)
    below, above = (x < lo) & ~nan, (x >= hi) & ~nan
    inside = ~(nan | below | above)
    b = np.minimum(((x[inside] - lo) * inv_w).astype(np.int64), n_bins - 1)
    out[:n_bins] = np.bincount(b, minlength=n_bins).astype(np.uint64)
    out[n_bins], out[n_bins + 1], out[n_bins + 2] = below.sum(), above.sum(), nan.sum()
    return out


class LadderReference:
    """HipEngine's surface for a handle with a ladder, from the twins.  Constructor arguments as HipEngine's."""

    ladder_class = T.TrackTwin       # (the host tests put a defective subclass here)

    def __init__(self, *, n_chains, chain_offset=0, n_chains_global=None, potential="harmonic", beta=1.0, sigma=(1.0,), weight=(1.0,),
                 seed=1, sweepstep=1, per_chain_counters=True, dtype="f64", param_dtype="f64"):
        self.n_chains, self.offset = int(n_chains), int(chain_offset)
        self.n_global = int(n_chains_global if n_chains_global is not None else self.offset + self.n_chains)
        self.potential, self.seed, self.sweepstep = potential, int(seed), int(sweepstep)
        self.dtype, self.param_dtype = dtype, param_dtype
        self.pool_sigma = [float(s) for s in sigma]          # the shared sigma_k: amc_set_parameters writes it whether or not a table is set
        self.weight = [float(w) for w in weight]
        self.n_moves = len(self.pool_sigma)
        self.per_chain_counters = bool(per_chain_counters) or self.n_moves > 1
        self.beta = np.full(self.n_chains, float(beta))
        self.table = None                                    # widths per rung, shape (K, R), while set
        self.sim = self._plain_sim()
        self.n_rungs = 0
        self.tw = None
        self._t_x = 0                                        # a property of the handle: survives clearing and re-setting the ladder

    # -- the simulation underneath -------------------------------------------------------------------------------------------------------
    def _plain_sim(self):
        if self.param_dtype == "f32":
            assert self.dtype == "f32" and self.sweepstep == 1
            return F.TwinSim(self.n_chains, chain_offset=self.offset, potential=self.potential, beta=1.0,
                             sigma=[np.float32(s) for s in self.pool_sigma], weight=self.weight, seed=self.seed)
        return O.OracleSim(self.n_chains, chain_offset=self.offset, potential=self.potential, beta=1.0, sigma=self.pool_sigma,
                           weight=self.weight, seed=self.seed, sweepstep=self.sweepstep, dtype=self.dtype)

    def _rung_sim(self, table):
        return RT.RungSigmaTwin(self.n_chains, table, chain_offset=self.offset, weight=self.weight, potential=self.potential, beta=1.0,
                                seed=self.seed, sweepstep=self.sweepstep, dtype=self.dtype)

    def _set_counters(self, sim, acc, tot):
        acc, tot = np.ascontiguousarray(acc, dtype=np.int64), np.ascontiguousarray(tot, dtype=np.int64)
        if isinstance(sim, O.OracleSim):
            p = O.C.POINTER(O.C.c_int64)
            sim.lib.amo_set_counters(sim.h, acc.ctypes.data_as(p), tot.ctypes.data_as(p))
        else:                                                # TwinSim, RungSigmaTwin: numpy arrays of their own
            sim.acc[:], sim.tot[:] = acc, tot

    def _switch(self, new):
        """x, beta, the step index and the per-chain counters go across; e follows x."""
        old = self.sim
        new.set_x(old.state()[0])
        new.set_beta(self.beta)
        new.step = old.step
        self._set_counters(new, *old.counters())
        old.close()
        self.sim = new
        if self.tw is not None:
            self.tw.sim, self.tw.state = new, X._State(new)

    def close(self):
        if hasattr(self.sim, "close"):
            self.sim.close()

    # -- state ----------------------------------------------------------------------------------------------------------------------------
    def upload_state(self, x, beta=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if beta is not None:
            self.beta = np.array(beta, dtype=np.float64)
        if isinstance(self.sim, F.TwinSim):
            X._State(self.sim).put(x, self.sim.pot)
            self.sim.beta[:] = self.beta.astype(np.float32)
        else:
            self.sim.set_x(x)
            self.sim.set_beta(self.beta)

    def download_state(self, want_e=True):
        x, e = self.sim.state()
        return x, (e if want_e else None)

    def download_counters(self):
        return self.sim.counters()

    def counter_totals(self):
        acc, tot = self.sim.counters()
        return acc.sum(axis=1), tot.sum(axis=1)

    def upload_counters(self, accepted, total):
        K, M = self.n_moves, self.n_chains
        self._set_counters(self.sim, np.asarray(accepted).reshape(K, M), np.asarray(total).reshape(K, M))

    @property
    def step(self):
        return int(self.sim.t if isinstance(self.sim, F.TwinSim) else self.sim.step)

    estimator_step = 0               # the walk makes no estimator call, and nothing else moves t_est

    # -- sweeps ---------------------------------------------------------------------------------------------------------------------------
    def sweep(self, n=1):
        if n > 0:
            self.sim.make_steps(int(n))

    sweep_launches = sweep           # n launches of one sweep each: identical to n calls of sweep(1)

    def set_parameters(self, k, p):
        s = float(np.asarray(p, dtype=np.float64).reshape(-1)[0])
        self.pool_sigma[int(k)] = s
        if self.table is None:                               # with a table the sweeps do not use the shared sigma_k
            self.sim.set_sigma(int(k), s)

    def get_parameters(self, k):
        return np.array([self.pool_sigma[int(k)]])

    # -- the ladder -----------------------------------------------------------------------------------------------------------------------
    def set_ladder(self, n_rungs):
        """Zeroes the gap counters, turns tracking off, clears the table; t_x stays."""
        R = int(n_rungs)
        assert 2 <= R <= 64 and self.n_chains % R == 0 and self.offset % R == 0 and self.n_global % R == 0
        if self.tw is not None:
            self._t_x = self.tw.t_x
        self.set_rung_sigma(None)
        self.tw = self.ladder_class(self.sim, self.beta, R, seed=self.seed, potential=self.potential, chain_offset=self.offset,
                                    f32=self.dtype == "f32")
        self.tw.t_x = self._t_x
        self.n_rungs = R

    def exchange(self, n=1):
        self.tw.exchange(int(n))

    def sweep_exchange(self, n_rounds, sweeps_per_round=1):
        for _ in range(int(n_rounds)):
            self.sweep(sweeps_per_round)
            self.exchange(1)

    def exchange_counters(self):
        return self.tw.counters()

    def set_exchange_counters(self, accepted, attempted):
        self.tw.accepted[:] = np.asarray(accepted, dtype=np.int64)
        self.tw.attempted[:] = np.asarray(attempted, dtype=np.int64)

    @property
    def exchange_step(self):
        return self.tw.t_x

    @exchange_step.setter
    def exchange_step(self, t):
        assert 0 <= int(t) < T_X_LIMIT
        self.tw.t_x = int(t)

    def histogram_rungs(self, lo, hi, n_bins):
        x, R = self.sim.state()[0], self.n_rungs
        return np.stack([self.hist_row(x[r::R], float(lo), float(hi), int(n_bins)) for r in range(R)])

    hist_row = staticmethod(hist_row)

    def reduce_rungs(self, columns=RS.ALL):
        x, e = self.sim.state()
        return RS.records(x, e, self.n_rungs, int(columns))

    def reduce_state_records(self):
        """The sum e, sum x, sum x^2 records of amc_reduce: kind-R sums whose summands are the chain PAIRS'
        sums, a lone last chain by itself -- fl(e_2p + e_2p+1), fl(x_2p + x_2p+1), fl(fl(x_2p^2) + fl(x_2p+1^2))."""
        x, e = self.sim.state()
        if x.size % 2:
            x, e = np.append(x, 0.0), np.append(e, 0.0)
        with np.errstate(all="ignore"):
            xx = x * x
            cols = (e[0::2] + e[1::2], x[0::2] + x[1::2], xx[0::2] + xx[1::2])
        return np.stack([O.xsum_r(c) for c in cols])

    # -- walker tracking ------------------------------------------------------------------------------------------------------------------
    @property
    def tracking(self):
        return self.tw is not None and self.tw.lab is not None

    def set_tracking(self, on=True):
        self.tw.set_tracking(bool(on))

    def labels(self):
        assert self.tracking
        return self.tw.lab & np.uint8(63), self.tw.lab >> np.uint8(6)

    def set_labels(self, walker, direction):
        assert self.tracking
        lab = (np.asarray(walker, dtype=np.int64) | (np.asarray(direction, dtype=np.int64) << 6)).astype(np.uint8)
        T.check_labels(lab, self.n_rungs)
        self.tw.lab = lab

    def flow_rungs(self):
        assert self.tracking
        return T.flow_counts(self.tw.lab, self.n_rungs)

    def tracking_counters(self):
        assert self.tracking
        return self.tw.round_trips, self.tw.up_trips

    def set_tracking_counters(self, round_trips, up_trips):
        assert self.tracking
        self.tw.round_trips, self.tw.up_trips = int(round_trips), int(up_trips)

    # -- widths per rung ------------------------------------------------------------------------------------------------------------------
    def set_rung_sigma(self, sigma):
        if sigma is None:
            if self.table is not None:                       # the sweeps read the pool's sigma_k again, as it is now
                self.table = None
                self._switch(self._plain_sim())
            return
        assert self.n_rungs and self.per_chain_counters and self.param_dtype == "f64" and self.n_moves * self.n_rungs <= 64
        self.table = np.array(sigma, dtype=np.float64).reshape(self.n_moves, self.n_rungs)
        self._switch(self._rung_sim(self.table_as_read()))

    def table_as_read(self):
        """sigma[k][r] is entry k R + r."""
        return self.table

    def rung_sigma(self):
        assert self.table is not None
        return self.table.copy()

    def rung_counter_totals(self):
        acc, tot = self.sim.counters()
        R = self.n_rungs
        return (np.stack([acc[:, r::R].sum(axis=1) for r in range(R)], axis=1), np.stack([tot[:, r::R].sum(axis=1) for r in range(R)], axis=1))


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def expected_slices(M, S):
    """Slices that hold pairs: whole blocks of 256 pairs are dealt out (amc_slices.h; test_gpu_sliced_launches.expected_slices)."""
    return min(S, -(-((M + 1) // 2) // 256))


def crossing_offset(R, M):
    """An even multiple of R with offset < 2^32 < offset + M where M allows it (the middle of the shard then lies near 2^32)."""
    return ((TWO32 - M // 2) // (2 * R)) * 2 * R


def draw_case(rng):
    R = int(rng.choice([2, 3, 4, 5, 7, 8, 16, 63, 64]))
    L = int(rng.choice([1, 2, 3, 85, 171, 257, 513, 1025]))
    L = max(1, min(L, MAX_CHAINS // R))
    M = R * L
    K = int(rng.choice([1, 1, 2, 3, 9]))
    w = rng.dirichlet(np.ones(K) * rng.choice([0.5, 1.0, 5.0]))
    if rng.random() < 0.3:                                   # weights on the 2^-12 grid: every cell of the pick table closed
        w = np.maximum(1, np.round(w * 4096)) / 4096
        w[-1] += 1.0 - w.sum()
        if w[-1] <= 0:
            w = np.full(K, 1.0 / K)
    w = w / w.sum()
    dtype = str(rng.choice(["f64", "f64", "f32"]))
    sweepstep = int(rng.choice([1, 1, 2, 3]))
    # Float32 parameters: where f32_param_twin.TwinSim has the pool -- Float32 state, one step per sweep, sigma Float32 values
    param_dtype = "f32" if dtype == "f32" and sweepstep == 1 and rng.random() < 0.5 else "f64"
    sigma = [float(np.exp(rng.uniform(np.log(1e-2), np.log(10.0)))) for _ in range(K)]
    if param_dtype == "f32":
        sigma = [float(np.float32(s)) for s in sigma]
    per_chain = bool(K > 1 or rng.random() < 0.5)
    kind = int(rng.integers(0, 6))
    offset = [0, 2 * R, 2 * R * 2 ** 19, 2 * R * (2 ** 31 + 3), 2 * R * 2 ** 38, crossing_offset(R, M)][kind]
    case = dict(
        R=R, n_chains=M, chain_offset=int(offset),
        potential=str(rng.choice(["harmonic", "double_well"])),
        sigma=sigma, weight=[float(v) for v in w],
        seed=int(rng.integers(0, 2 ** 63)), sweepstep=sweepstep, dtype=dtype, param_dtype=param_dtype, per_chain_counters=per_chain,
        beta_kind=str(rng.choice(["geometric", "random", "equal"])), beta_ratio=float(rng.uniform(1.05, 2.0)),
        plant=bool(rng.random() < 0.15), state_seed=int(rng.integers(0, 2 ** 31)),
        # handles that can take the sliced route (K = 1, pool-wide counter, one step per sweep) get the knobs that force it
        slices=int(rng.choice([2, 3])) if K == 1 and not per_chain and sweepstep == 1 else 0,
        walk_seed=int(rng.integers(0, 2 ** 31)), n_ops=int(rng.integers(14, 29)), script=[],
    )
    return case


def make_state(case):
    """(x0, beta) of a case: x0 normal(0, 1.5), through Float32 for Float32 state, with a NaN, +Inf, -Inf and 1e200 planted where the
    case says so; beta a geometric ladder, random per chain (not periodic in R) or all equal."""
    rng = np.random.default_rng([case["state_seed"], 77])
    M, R = case["n_chains"], case["R"]
    x0 = rng.normal(0.0, 1.5, M)
    if case["beta_kind"] == "geometric":
        beta = (0.5 * case["beta_ratio"] ** np.arange(R))[np.arange(M) % R]
    elif case["beta_kind"] == "random":
        beta = rng.uniform(0.2, 3.0, M)
    else:
        beta = np.full(M, 0.5 * case["beta_ratio"])
    if case["plant"]:
        where = rng.choice(M, size=min(4, M), replace=False)
        for c, v in zip(where, [np.nan, np.inf, -np.inf, 1e200]):
            x0[c] = v
    if case["dtype"] == "f32":
        with np.errstate(over="ignore"):
            x0 = x0.astype(np.float32).astype(np.float64)
    return x0, beta


def engine_kwargs(case):
    return dict(n_chains=case["n_chains"], chain_offset=case["chain_offset"], n_chains_global=case["chain_offset"] + case["n_chains"],
                potential=case["potential"], beta=1.0, sigma=case["sigma"], weight=case["weight"], seed=case["seed"],
                sweepstep=case["sweepstep"], per_chain_counters=case["per_chain_counters"], dtype=case["dtype"],
                param_dtype=case["param_dtype"])


def create(factory, case):
    """An engine of the case; a case with slices finds the knobs of the sliced route while its handle is created."""
    if not case["slices"]:
        return factory(**engine_kwargs(case))
    mp = pytest.MonkeyPatch()
    mp.setenv("AMC_SWEEP_SLICES", str(case["slices"]))
    mp.setenv("AMC_SWEEP_SLICE_MIN_CHAINS", "0")
    mp.setenv("AMC_DEBUG_PLAN", "1")
    try:
        return factory(**engine_kwargs(case))
    finally:
        mp.undo()


def check_case(case):
    """The engine's preconditions."""
    R, M, off = case["R"], case["n_chains"], case["chain_offset"]
    K = len(case["sigma"])
    assert 2 <= R <= 64 and 0 < M <= MAX_CHAINS and M % R == 0 and off % R == 0 and (off + M) % R == 0 and off % 2 == 0
    assert len(case["weight"]) == K and abs(sum(case["weight"]) - 1.0) < 1e-12 and all(1e-100 <= s <= 1e100 for s in case["sigma"])
    assert case["per_chain_counters"] or K == 1
    assert case["param_dtype"] == "f64" or (case["dtype"] == "f32" and case["sweepstep"] == 1
                                            and all(float(np.float32(s)) == s for s in case["sigma"]))
    assert not case["slices"] or (K == 1 and not case["per_chain_counters"] and case["sweepstep"] == 1)
    assert 0 <= case["seed"] < 2 ** 63


def pinned_case(R, L, script, **kw):
    case = dict(R=R, n_chains=R * L, chain_offset=0, potential="harmonic", sigma=[0.6], weight=[1.0], seed=20260311, sweepstep=1,
                dtype="f64", param_dtype="f64", per_chain_counters=True, beta_kind="geometric", beta_ratio=1.4, plant=False,
                state_seed=R * 1000 + L, slices=0, walk_seed=R + L, n_ops=len(script) + 6, script=[list(op) for op in script])
    case.update(kw)
    return case


# Combinations the random draw meets too seldom for a default list of a few dozen cases: each case starts with a fixed script and goes
# on with drawn operations.
PINNED = [
    # a table under tracking and exchange steps; counts uploaded just below the 16-bit mark and swept across it with the table set; the
    # table rewritten and cleared behind queued sweeps; the pool's sigma written while the table hides it, and once more after clearing
    pinned_case(4, 171, [("track",), ("table",), ("single", 2), ("exchange", 3), ("sigma",), ("recount", 65_530), ("multi", 9),
                         ("rung_totals",), ("counters",), ("table",), ("launches", 3), ("sweep_exchange", 3, 2), ("rung_hist", 7, True),
                         ("clear",), ("sigma",), ("single", 3), ("state",), ("walkers",), ("gaps",), ("rung_hist", 200, True),
                         ("rung_hist", 4000, True)],
                sigma=[0.8, 0.11], weight=[0.625, 0.375], chain_offset=2 * 4 * 2 ** 19),
    # chain id 2^32 inside the shard (an offset that 2, 3 and 9 divide), the exchange step index walking over 2^32, another ladder in
    # the middle of the run, the last step indices below 2^48
    pinned_case(3, 171, [("track",), ("tx", TWO32 - 1), ("exchange", 4), ("sweep_exchange", 2, 1), ("state",), ("gaps",), ("walkers",),
                         ("ladder", 9), ("exchange", 3), ("gaps",), ("tx", T_X_LIMIT - 3), ("exchange", 3), ("state",)],
                potential="double_well", beta_kind="random", chain_offset=((TWO32 - 256) // 18) * 18),
    # equal beta: every swap is accepted, walkers travel end to end; the all-Float32 model; labels uploaded between steps of different parity
    pinned_case(3, 85, [("track",), ("exchange", 8), ("walkers",), ("exchange", 1), ("labels",), ("exchange", 1), ("sweep_exchange", 3, 0),
                        ("walkers",), ("untrack",), ("exchange", 2), ("track",), ("exchange", 3), ("walkers",)],
                dtype="f32", param_dtype="f32", sigma=[0.5], beta_kind="equal", chain_offset=6 * (2 ** 31 + 3)),
    # the sliced route on a handle with a ladder: double well, 5 blocks of pairs in 3 slices, exchange steps between the sliced calls
    pinned_case(4, 513, [("launches", 4), ("exchange", 1), ("launches", 2), ("exchange", 2), ("launches", 7), ("state",), ("counters",),
                         ("gaps",), ("tx", TWO32), ("sweep_exchange", 2, 1), ("launches", 3), ("reduce",)],
                potential="double_well", per_chain_counters=False, slices=3, chain_offset=8),
    # ... harmonic, 2 slices, non-finite positions, tracking
    pinned_case(2, 1025, [("track",), ("launches", 3), ("exchange", 3), ("launches", 2), ("walkers",), ("rung_sums", 7), ("rung_hist", 200, False),
                          ("state",)],
                per_chain_counters=False, slices=2, plant=True, beta_kind="random", chain_offset=4 * 2 ** 38),
    # Float32 state with the slice knobs set: its kernels are compiled at run time, so its launches stay whole
    pinned_case(7, 171, [("launches", 3), ("exchange", 2), ("launches", 2), ("state",), ("rung_sums", 5), ("counters",)],
                dtype="f32", per_chain_counters=False, slices=2, plant=True),
]


def case_list(seed, n_cases, pinned=PINNED):
    return [dict(c) for c in pinned] + [draw_case(np.random.default_rng([seed, i])) for i in range(n_cases)]


# ---- the walk --------------------------------------------------------------------------------------------------------------------------
def fbits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_floats(a, b):
    """Bit for bit; a NaN against a NaN (its sign and payload are no part of any definition here)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(fbits(a)[~na], fbits(b)[~nb])


def same_ints(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.astype(np.int64), b.astype(np.int64))


MUTATORS = ["single", "single", "multi", "launches", "launches", "exchange", "exchange", "exchange", "sweep_exchange", "sweep_exchange",
            "table", "table", "clear", "sigma", "track", "track", "untrack", "labels", "xcounters", "tx", "ladder", "recount"]
OBSERVERS = ["state", "counters", "gaps", "walkers", "rung_sums", "rung_hist", "rung_totals", "reduce"]
OPERATIONS = sorted(set(MUTATORS)) + OBSERVERS
T_X_VALUES = [0, 1, TWO32 - 1, TWO32, 1 << 47, T_X_LIMIT - 3]
RECOUNT_STEPS = [0, 17, 65_530, 65_535, 65_536, 70_000]


def other_ladders(ref):
    """The R' != R that this shard can take: divisors of n_chains and of the offset (and so of the global count)."""
    return [r for r in range(2, 65) if r != ref.n_rungs and ref.n_chains % r == 0 and ref.offset % r == 0]


def possible(ref, name):
    """Whether the handle, as it is now, takes operation `name`."""
    if name == "table":
        return ref.per_chain_counters and ref.param_dtype == "f64" and ref.n_moves * ref.n_rungs <= 64
    if name == "clear":
        return ref.table is not None
    if name in ("labels", "walkers", "untrack"):
        return ref.tracking
    if name == "ladder":
        return bool(other_ladders(ref))
    if name in ("recount", "rung_totals"):
        return ref.per_chain_counters
    return True


def draw_op(rng, ref, steps_left):
    """One operation the handle can take, with its scalar arguments: a tuple (name, ...).  Arrays are drawn when it is applied."""
    for _ in range(64):
        name = str(rng.choice(OBSERVERS if rng.random() < 0.4 else MUTATORS))
        if not possible(ref, name):
            continue
        if name == "single":
            return (name, int(rng.integers(1, 6)))
        if name == "multi":
            return (name, int(rng.integers(2, 12)))
        if name == "launches":
            return (name, int(rng.integers(1, 8)))
        if name == "exchange":
            n = min(int(rng.integers(1, 7)), steps_left, T_X_LIMIT - ref.exchange_step)
            if n > 0:
                return (name, n)
            continue
        if name == "sweep_exchange":
            n = min(int(rng.integers(1, 5)), steps_left, T_X_LIMIT - ref.exchange_step)
            if n > 0:
                return (name, n, int(rng.integers(0, 4)))
            continue
        if name == "tx":
            return (name, int(rng.choice(T_X_VALUES)))
        if name == "ladder":                # seldom: it turns tracking off and clears the table
            if rng.random() < 0.7:
                continue
            return (name, int(rng.choice(other_ladders(ref))))
        if name == "recount":
            return (name, int(rng.choice(RECOUNT_STEPS)))
        if name == "rung_sums":
            return (name, int(rng.integers(1, 8)))
        if name == "rung_hist":
            return (name, int(rng.choice([7, 200, 4000])), bool(rng.random() < 0.5))
        return (name,)
    return ("state",)


def histogram_range(rng, ref, n_bins, at_edge):
    """(lo, hi): a range around the bulk; or, `at_edge`, one whose hi lies one ulp above a chain's position x_c, with lo such that
    (x_c - lo) inv_w rounds to n_bins -- the position the rule clamps into the last bin -- where a few tries find one."""
    lo, hi = float(rng.uniform(-3.0, -0.5)), float(rng.uniform(0.5, 3.0))
    if not at_edge:
        return lo, hi
    x = ref.download_state()[0]
    finite = np.flatnonzero(np.isfinite(x) & (np.abs(x) < 100.0))
    if finite.size == 0:
        return lo, hi
    for _ in range(16):
        xc = float(x[int(rng.choice(finite))])
        hi = float(np.nextafter(xc, np.inf))
        lo = hi - float(rng.uniform(1.0, 6.0))
        if int((xc - lo) * (n_bins / (hi - lo))) == n_bins:
            break
    return lo, hi


def apply_op(op, sides, rng, ref):
    """`sides` take a mutating operation of a handle in the state `ref` is in; its arrays are drawn here from rng."""
    name = op[0]
    K, M, R = ref.n_moves, ref.n_chains, ref.n_rungs
    if name == "single":
        for s in sides:
            for _ in range(op[1]):
                s.sweep(1)
    elif name == "multi":
        for s in sides:
            s.sweep(op[1])
    elif name == "launches":
        for s in sides:
            s.sweep_launches(op[1])
    elif name == "exchange":
        for s in sides:
            s.exchange(op[1])
    elif name == "sweep_exchange":
        for s in sides:
            s.sweep_exchange(op[1], op[2])
    elif name == "table":                   # distinct entries spread over [1e-3, 10]
        tab = np.exp(np.linspace(np.log(1e-3), np.log(10.0), K * R) + rng.uniform(-0.01, 0.01, K * R))
        tab = rng.permutation(tab).reshape(K, R)
        for s in sides:
            s.set_rung_sigma(tab)
    elif name == "clear":
        for s in sides:
            s.set_rung_sigma(None)
    elif name == "sigma":
        k, v = int(rng.integers(0, K)), float(np.exp(rng.uniform(np.log(1e-2), np.log(10.0))))
        if ref.param_dtype == "f32":
            v = float(np.float32(v))
        for s in sides:
            s.set_parameters(k, [v])
    elif name in ("track", "untrack"):
        for s in sides:
            s.set_tracking(name == "track")
    elif name == "labels":                  # a permutation per ladder, the ends' directions as they must be, the others any
        w = np.argsort(rng.random((M // R, R)), axis=1)
        d = rng.integers(0, 3, (M // R, R))
        d[:, 0], d[:, R - 1] = T.UP, T.DOWN
        trips = (int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2 ** 40)))
        for s in sides:
            s.set_labels(w.reshape(-1), d.reshape(-1))
            s.set_tracking_counters(*trips)
    elif name == "xcounters":
        att = rng.integers(0, 2 ** 40, R - 1)
        acc = (att * rng.uniform(0, 1, R - 1)).astype(np.int64)
        for s in sides:
            s.set_exchange_counters(acc, att)
    elif name == "tx":
        for s in sides:
            s.exchange_step = op[1]
    elif name == "ladder":
        for s in sides:
            s.set_ladder(op[1])
    elif name == "recount":                 # step counts on both sides of the 16-bit mark, as test_gpu_fuzz's recount
        tot = rng.multinomial(op[1], ref.weight, size=M).T.astype(np.int64)
        acc = (tot * rng.uniform(0, 1, tot.shape)).astype(np.int64)
        for s in sides:
            s.upload_counters(acc, tot)
    else:
        raise ValueError(op)


def observe(op, eng, ref, rng, fail):
    name = op[0]
    if name == "state":
        (x, e), (xo, eo) = eng.download_state(), ref.download_state()
        if not same_floats(x, xo):
            fail("positions differ", np.flatnonzero(fbits(x) != fbits(xo))[:8])
        if not same_floats(e, eo):
            fail("energies differ", np.flatnonzero(fbits(e) != fbits(eo))[:8])
    elif name == "counters":
        if ref.per_chain_counters:
            (a, t), (ao, to) = eng.download_counters(), ref.download_counters()
        else:
            (a, t), (ao, to) = eng.counter_totals(), ref.counter_totals()
        if not (same_ints(a, ao) and same_ints(t, to)):
            fail("Move counters differ")
    elif name == "gaps":
        (a, t), (ao, to) = eng.exchange_counters(), ref.exchange_counters()
        if not (same_ints(a, ao) and same_ints(t, to)):
            fail("gap counters differ", (a, ao, t, to))
        if eng.exchange_step != ref.exchange_step:
            fail("exchange step index differs", (eng.exchange_step, ref.exchange_step))
    elif name == "walkers":
        (w, d), (wo, do) = eng.labels(), ref.labels()
        if not (same_ints(w, wo) and same_ints(d, do)):
            fail("labels differ", np.flatnonzero((w != wo) | (d != do))[:8])
        if not same_ints(eng.flow_rungs(), ref.flow_rungs()):
            fail("flow counts differ")
        if tuple(eng.tracking_counters()) != tuple(ref.tracking_counters()):
            fail("trip counters differ", (eng.tracking_counters(), ref.tracking_counters()))
    elif name == "rung_sums":
        got, want = eng.reduce_rungs(op[1]), ref.reduce_rungs(op[1])
        if not (got.shape == want.shape and np.array_equal(fbits(got), fbits(want))):
            fail("per-rung records differ", np.argwhere(fbits(got) != fbits(want))[:4])
    elif name == "rung_hist":
        lo, hi = histogram_range(rng, ref, op[1], op[2])
        got, want = eng.histogram_rungs(lo, hi, op[1]), ref.histogram_rungs(lo, hi, op[1])
        if not same_ints(got, want):
            fail(f"per-rung histograms of [{lo!r}, {hi!r}) differ", np.argwhere(np.asarray(got) != np.asarray(want))[:4])
    elif name == "rung_totals":
        (a, t), (ao, to) = eng.rung_counter_totals(), ref.rung_counter_totals()
        if not (same_ints(a, ao) and same_ints(t, to)):
            fail("Move counters per rung differ")
    elif name == "reduce":
        got = eng.reduce_state_records() if hasattr(eng, "reduce_state_records") else np.asarray(eng.reduce_exact()[0])[:3]
        want = ref.reduce_state_records()
        if not np.array_equal(fbits(got), fbits(want)):
            fail("records of sum e, sum x, sum x^2 differ", np.argwhere(fbits(got) != fbits(want))[:4])
    else:
        raise ValueError(op)


def run_walk(engine, reference, rng, n_ops, case=None, script=(), after_op=None):
    """`script`, then operations drawn from rng until n_ops are done; the comparison of everything at the end.  Returns
    dict(ops=[...], events={...}): what ran, and which of the combinations the host test counts it met.  after_op(op) is called after
    the engine has taken a mutating operation."""
    ops, events = [], set()
    case = case or {}

    def fail(what, detail=None):
        raise AssertionError(f"after operation {len(ops) - 1} {ops[-1] if ops else ''}: {what}" + (f"\n{detail}" if detail is not None else "") +
                             f"\ncase = {case!r}\noperations = {ops!r}")

    ref = reference
    steps_left = MAX_EXCHANGE_STEPS
    cleared = 0                  # a table cleared (1), then set_parameters (2), then a sweep
    ladder_changed = False
    cross_in = None              # steps until a chain's count crosses 65 536, after an upload while a table is set
    sliced_calls = 0
    crossing = case.get("chain_offset", 0) < TWO32 < case.get("chain_offset", 0) + ref.n_chains
    queue = [tuple(op) for op in script]
    if not queue:                           # most walks start with tracking on, and with a table where the handle takes one
        queue += [("track",)] * bool(rng.random() < 0.6) + [("table",)] * bool(rng.random() < 0.6 and possible(ref, "table"))
    while len(ops) < max(n_ops, len(script)):
        op = queue.pop(0) if queue else draw_op(rng, ref, steps_left)
        name = op[0]
        ops.append(op)
        if name in OBSERVERS:
            observe(op, engine, ref, rng, fail)
            if name == "walkers" and case.get("beta_kind") == "equal" and min(ref.tracking_counters()) >= 1:
                events.add("equal beta with tracking: a round trip and an up trip")
            continue
        if not possible(ref, name):
            fail("the script asks for an operation the handle cannot take")
        n_x = op[1] if name in ("exchange", "sweep_exchange") else 0
        if n_x:
            t0, R = ref.exchange_step, ref.n_rungs
            if ref.table is not None and ref.tracking:
                events.add("table, tracking and exchange on one handle")
            if ladder_changed:
                events.add("set_ladder to another R, then exchange steps")
            if any(t >= TWO32 and X.gaps_of_step(R, t) for t in range(t0, t0 + n_x)):
                events.add("exchange step index >= 2^32 with swaps attempted")
            if crossing:
                events.add("chain ids cross 2^32 inside the shard")
            if ref.param_dtype == "f32" and ref.tracking:
                events.add("Float32 parameters with tracking")
            if sliced_calls:
                events.add("exchange steps between sliced calls")
            steps_left -= n_x
        n_sweeps = op[1] if name in ("single", "multi", "launches") else op[1] * op[2] if name == "sweep_exchange" else 0
        if n_sweeps:
            if cleared == 2:
                events.add("a table cleared, then set_parameters, then a sweep")
            if cross_in is not None and ref.table is not None:
                cross_in -= n_sweeps * ref.sweepstep
                if cross_in <= 0:
                    events.add("counts cross 65 536 after an upload while a table is set")
                    cross_in = None
        if name == "launches" and case.get("slices") and op[1] >= 2:
            sliced_calls += 1
            if expected_slices(ref.n_chains, case["slices"]) >= 2:
                events.add("sliced route with a ladder, at least 2 slices")
                if case["potential"] == "double_well":
                    events.add("double well on the sliced route")
            if case["dtype"] == "f32":
                events.add("Float32 state on a handle with the slice knobs")
        if name == "clear":
            cleared = 1
        elif name == "sigma" and cleared == 1:
            cleared = 2
        elif name in ("table", "ladder"):
            cleared = 0
        if name == "ladder":
            ladder_changed = True
        if name == "recount":
            cross_in = 65_536 - op[1] if ref.table is not None and 0 < 65_536 - op[1] <= 64 else None
        elif name in ("clear", "ladder"):
            cross_in = None
        arrays = int(rng.integers(0, 2 ** 62))     # both sides draw the operation's arrays from generators with this one seed
        try:
            apply_op(op, (engine,), np.random.default_rng(arrays), ref)
        except AssertionError:
            raise
        except Exception as exc:               # a refusal by the engine of something the reference takes
            fail(f"the engine refused: {exc!r}")
        if after_op is not None:
            after_op(op)
        apply_op(op, (ref,), np.random.default_rng(arrays), ref)
    if case.get("plant"):
        events.add("non-finite positions")
    # the end: everything
    ops.append(("end",))
    for name in OBSERVERS:
        if possible(ref, name):
            observe((name, 7) if name == "rung_sums" else (name, 200, False) if name == "rung_hist" else (name,), engine, ref, rng, fail)
    if engine.step != ref.step:
        fail("step index differs", (engine.step, ref.step))
    if engine.exchange_step != ref.exchange_step:
        fail("exchange step index differs", (engine.exchange_step, ref.exchange_step))
    if engine.estimator_step != ref.estimator_step:
        fail("estimator step index differs", (engine.estimator_step, ref.estimator_step))
    return dict(ops=ops[:-1], events=events)


def run_case(factory, case, reference_factory=LadderReference, after_op=None):
    """Engine and reference of `case`, state and ladder, the walk; both closed whatever happens."""
    check_case(case)
    x0, beta = make_state(case)
    ref = create(reference_factory, case)
    eng = None
    try:
        eng = create(factory, case)
        for s in (eng, ref):
            s.upload_state(x0, beta)
            s.set_ladder(case["R"])
        rng = np.random.default_rng([case["walk_seed"], 5])
        return run_walk(eng, ref, rng, case["n_ops"], case=case, script=case.get("script", ()), after_op=after_op)
    finally:
        ref.close()
        if eng is not None:
            eng.close()
