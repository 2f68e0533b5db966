"""Random operation walks over a handle with a temperature ladder, against the host twins composed into one reference object.

The ladder features (exchange steps, per-rung sums, walker tracking, widths per rung) and the sliced
single-sweep launches (section 6 "Slices") each have a twin and a test file of their own, and all of those walk one hand-written
sequence.  This module draws the configuration and the sequence:

    LadderReference   the surface of montecarlo_amd._capi.HipEngine that the walk uses, computed by the twins alone --
                      oracle_lib.OracleSim, f32_param_twin.TwinSim or rung_sigma_twin.RungSigmaTwin underneath, track_twin.TrackTwin
                      above, rung_sums_twin.records, track_twin.flow_counts, numpy for the bin rule and the strided counter sums.  What
                      set_ladder, set_rung_sigma(None), set_tracking and the setters reset or keep follows the text of DESIGN.md
                      section 3.13 and include/amc.h.  It shares no code with the product.
                      The ladder tools on top: respace_twin.RespaceTwin (the ladder class), tune_twin.tune_rule with the window and
                      its base, bridge_twin.records / merge, corr_twin.observable / sample_records with one group per rung,
                      blocks_twin with first = chain_offset // R -- and, from the header's text alone, what a respacing that is
                      taken, set_rung_sigma, set_ladder, set_blocks and upload_state zero or keep, and which calls are refused with
                      AMC_ERR_STATE (Refused).  HipEngine has no read of the per-chain beta but ladder(): that is the "get_ladder"
                      observer.
    draw_case        one configuration (a plain dict; x0 and beta are functions of it: make_state)
    run_walk          the operations, drawn one by one; both sides take each, the observers compare bit for bit / integer for integer
    run_case          engine and reference of a case, the walk, the comparison at the end

The engine side is anything with HipEngine's surface: the host tests run the walk with a second reference object in its place.
"""
import os

import numpy as np
import pytest

import blocks_twin as BL
import bridge_twin as BT
import corr_twin as CT
import exchange_twin as X
import f32_param_twin as F
import oracle_lib as O
import respace_twin as RP
import rung_sigma_twin as RT
import rung_sums_twin as RS
import track_twin as T
import tune_twin as TU

DEFAULT_CASES, DEFAULT_SEED = 40, 20261019       # drawn cases behind the pinned ones (AMC_LADDER_FUZZ_CASES, AMC_LADDER_FUZZ_SEED)
MAX_CHAINS = 6200
MAX_EXCHANGE_STEPS = 40          # per walk: the twin's exchange step is a Python loop over the gaps
T_X_LIMIT = 1 << 48              # amc_exchange refuses a step index that has reached 2^48
TWO32 = 1 << 32
MAX_SNAPSHOTS, MAX_SAMPLES = 12, 20      # per walk: below the second reallocation of a blocked accumulator (slot 16, then 32)
ERR_STATE = -5                   # AMC_ERR_STATE


class Refused(RuntimeError):
    """What the reference raises where the header says AMC_ERR_STATE; worded as _capi._check words an AmcError."""

    def __init__(self, what):
        super().__init__(f"amc error {ERR_STATE}: {what}")


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

    ladder_class = RP.RespaceTwin    # (the host tests put a defective subclass here)

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
        self.partition = None                                # (B, C) while a partition is set
        self.corr = None                                     # the mark: dict(observable, origin, records, steps, series)
        self._bridge_clear()

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
        self.corr = None                                     # chain slots are reassigned: the mark is forgotten
        if beta is not None:
            self.beta = np.array(beta, dtype=np.float64)
            if self.tw is not None:
                self.tw.beta = self.beta.astype(np.float32).astype(np.float64) if self.dtype == "f32" else self.beta.copy()
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
        """Zeroes the gap counters, turns tracking off, clears the table, the bridge accumulator, the mark, the partition, the window
        base and the records of respacing and tuning; t_x stays."""
        R = int(n_rungs)
        assert 2 <= R <= 64 and self.n_chains % R == 0 and self.offset % R == 0 and self.n_global % R == 0
        if self.tw is not None:
            self._t_x = self.tw.t_x
        self.set_rung_sigma(None)
        self.tw = self.ladder_class(self.sim, self.beta, R, seed=self.seed, potential=self.potential, chain_offset=self.offset,
                                    f32=self.dtype == "f32")
        self.tw.t_x = self._t_x
        self.n_rungs = R
        self.partition, self.corr = None, None
        self._bridge_clear()
        self.base = np.zeros((2, self.n_moves, R), dtype=np.int64)
        self._tune_reset()

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
        """(the tuning record starts afresh; the window base stays)"""
        self._tune_reset()
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

    # -- the window and the tuning (tune_twin.tune_rule; the bookkeeping as tune_twin.TuneTwin keeps it) --------------------------------
    def _tune_reset(self):
        self.tune_st = np.zeros((self.n_moves, max(self.n_rungs, 1)), dtype=np.int64)
        self.n_tuned = 0

    def _window(self):
        acc, tot = self.rung_counter_totals()
        bad = (acc < self.base[0]) | (tot < self.base[1])
        return np.where(bad, -1, acc - self.base[0]), np.where(bad, -1, tot - self.base[1]), bad

    def rung_window_counts(self):
        a, t, _ = self._window()
        return a, t

    def rung_window_restart(self):
        self.base[0], self.base[1] = self.rung_counter_totals()

    def rung_window_base(self):
        return self.base[0].copy(), self.base[1].copy()

    def set_rung_window_base(self, accepted, total):
        K, R = self.n_moves, self.n_rungs
        self.base = np.stack([np.asarray(accepted, dtype=np.int64).reshape(K, R), np.asarray(total, dtype=np.int64).reshape(K, R)])

    def window_base_for_tuning(self):
        """(the host tests put a defect here)"""
        return self.base

    def tune_rung_sigma(self, target=0.44, gamma=1.0, min_calls=1000, sigma_lo=1e-100, sigma_hi=1e100, counts=None):
        if self.table is None:
            raise Refused("no table set")
        K, R = self.table.shape
        if counts is None:
            saved, self.base = self.base, self.window_base_for_tuning()
            A, Tt, bad = self._window()
            self.base = saved
        else:
            A, Tt = np.asarray(counts[0]).reshape(K, R), np.asarray(counts[1]).reshape(K, R)
            bad = np.zeros((K, R), dtype=bool)
        new = self.table.copy()
        for k in range(K):
            for r in range(R):
                self.tune_st[k, r], new[k, r] = TU.tune_rule(self.table[k, r], A[k, r], Tt[k, r], target, gamma, min_calls, sigma_lo, sigma_hi,
                                                             bool(bad[k, r]))
        if np.any((self.tune_st == TU.OK) | (self.tune_st == TU.CLAMPED)):
            self.n_tuned += 1
        self.rung_window_restart()                           # a tuning ends the window in every case
        if not np.array_equal(new.view(np.uint64), self.table.view(np.uint64)):
            self.table = new
            self._switch(self._rung_sim(self.table_as_read()))

    def tune_status(self):
        assert self.table is not None
        return self.tune_st.copy(), self.n_tuned

    # -- respacing (respace_twin) -------------------------------------------------------------------------------------------------------------
    def respace_ladder(self, rule, gamma=1.0, eps=0.0, counts=None):
        R = self.n_rungs
        if rule == RP.FLOW and counts is None and not self.tracking:
            raise Refused("rule flow with the handle's own counts while tracking is off")
        if counts is not None:
            c = np.asarray(counts, dtype=np.int64).reshape(-1)
            counts = (c[:R - 1], c[R - 1:]) if rule == RP.ACCEPTANCE else c.reshape(R, 3)
        if self.tw.respace(rule, gamma, eps, counts) == 0:
            self.beta = self.tw.beta.copy()
            self._respaced()

    def _respaced(self):
        """A respacing that is taken zeroes the bridge records and the count, every block's rows too; the mask stays."""
        self.bridge_rec, self.bridge_n = np.zeros((self.n_rungs, BT.COLS, BT.WORDS)), 0
        self.bridge_blk = None

    def respace_status(self):
        return self.tw.status, self.tw.n_respaced

    def ladder(self):
        return self.tw.ladder()

    # -- bridge sums (bridge_twin; per block blocks_twin) -----------------------------------------------------------------------------------
    def _bridge_clear(self):
        self.bridge_mask, self.bridge_n = 0, 0
        self.bridge_rec = np.zeros((max(self.n_rungs, 1), BT.COLS, BT.WORDS))
        self.bridge_blk = None                               # records[B][R][6][12] while a partition is set and a snapshot is in

    def _f32(self):
        return self.dtype == "f32"

    def _first_ladder(self):
        return self.offset // self.n_rungs

    def bridge_accumulate(self, columns=BT.ALL):
        columns, R = int(columns), self.n_rungs
        assert 0 < columns <= BT.ALL
        if self.bridge_mask and columns != self.bridge_mask:
            raise Refused("another column mask while one is fixed")
        self.bridge_mask = columns
        e = self.sim.state()[1]
        self.bridge_rec = BT.merge([self.bridge_rec, BT.records(e, self.tw.beta, R, columns, self._f32())])
        if self.partition is not None:
            B, C = self.partition
            blk = BL.bridge_records(e, self.tw.beta, R, B, C, columns, self._f32(), first=self.block_first())
            self.bridge_blk = blk if self.bridge_blk is None else BT.merge([self.bridge_blk, blk])
        self.bridge_n += 1

    def bridge_fetch(self, reset=False):
        out = self.bridge_rec.copy(), self.bridge_n
        if reset:
            self._bridge_clear()
        return out

    def set_bridge(self, records=None, n_snapshots=0):
        if records is not None and self.partition is not None:
            raise Refused("merged records while a partition is set")
        self._bridge_clear()
        if records is None or int(n_snapshots) == 0:
            return
        self.bridge_rec = np.array(records, dtype=np.float64).reshape(self.n_rungs, BT.COLS, BT.WORDS)
        self.bridge_n = int(n_snapshots)
        self.bridge_mask = sum(1 << c for c in range(BT.COLS) if self.bridge_rec[:, c].any())

    # -- time correlation, one group per rung (corr_twin; per block blocks_twin) ------------------------------------------------------------
    def _observe(self, kind):
        return CT.observable(kind, self.potential, self.sim.state()[0], self._f32())

    def corr_steps_entry(self):
        """steps[s]: the MH step index at the call (the host tests put a defect here)."""
        return self.step

    def corr_mark(self, observable="energy"):
        a = self._observe(observable)
        self.corr = dict(observable=CT.OBSERVABLES[observable], origin=a, records=[self.corr_sample_records(a, a)],
                         steps=[self.corr_steps_entry()], series=[a])

    def corr_sample_records(self, origin, values):
        return CT.sample_records(origin, values, self.n_rungs)

    def corr_sample(self):
        if self.corr is None:
            raise Refused("no mark")
        o = self._observe(self.corr["observable"])
        self.corr["records"].append(self.corr_sample_records(self.corr["origin"], o))
        self.corr["steps"].append(self.corr_steps_entry())
        if self.corr["series"] is not None:
            self.corr["series"].append(o)

    def corr_fetch(self):
        if self.corr is None:
            return np.zeros((0, self.n_rungs, CT.COLS, CT.WORDS)), np.zeros(0, dtype=np.uint64), 0
        return np.stack(self.corr["records"]), np.array(self.corr["steps"], dtype=np.uint64), self.corr["observable"]

    def corr_origin(self):
        if self.corr is None:
            raise Refused("no mark")
        return self.corr["origin"].copy()

    def set_corr(self, observable, origin, records, steps):
        if self.partition is not None:
            raise Refused("a plain mark while a partition is set")
        rec = np.array(records, dtype=np.float64).reshape(-1, self.n_rungs, CT.COLS, CT.WORDS)
        self.corr = dict(observable=CT.OBSERVABLES[observable], origin=np.array(origin, dtype=np.float64), records=list(rec),
                         steps=[int(s) for s in steps], series=None)

    def corr_clear(self):
        self.corr = None

    # -- jackknife blocks -----------------------------------------------------------------------------------------------------------------
    def set_blocks(self, n_blocks, chunk=0):
        """Clears the bridge accumulator and forgets the mark on every call that succeeds."""
        B = int(n_blocks)
        assert B == 0 or 2 <= B <= 64
        self.partition = None if B == 0 else (B, int(chunk) if int(chunk) else max(1, 256 // self.n_rungs))
        self._bridge_clear()
        self.corr = None

    def block_first(self):
        """The global index of local ladder 0 (the host tests put a defect here)."""
        return self._first_ladder()

    def bridge_fetch_blocks(self, reset=False):
        if self.partition is None:
            raise Refused("no partition")
        B = self.partition[0]
        rec = np.zeros((B, self.n_rungs, BT.COLS, BT.WORDS)) if self.bridge_blk is None else self.bridge_blk.copy()
        out = rec, self.bridge_n
        if reset:
            self._bridge_clear()
        return out

    def corr_fetch_blocks(self):
        if self.partition is None:
            raise Refused("no partition")
        B, C = self.partition
        if self.corr is None:
            return np.zeros((B, 0, self.n_rungs, CT.COLS, CT.WORDS)), np.zeros(0, dtype=np.uint64), 0
        rec = BL.corr_records(self.corr["series"], self.n_rungs, B, C, first=self.block_first())
        return rec, np.array(self.corr["steps"], dtype=np.uint64), self.corr["observable"]


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
    # -- the ladder tools ------------------------------------------------------------------------------------------------------------
    # a flow respacing that is taken, with a bridge mask fixed, a partition set and a mark standing: the block rows and the count are
    # zeroed, the mask, the mark and its samples stay, the labels and the gap counters start afresh
    pinned_case(4, 85, [("track",), ("blocks", 3, 5), ("exchange", 8), ("single", 2), ("bridge", BT.ACCEPTANCE_SET), ("mark", "energy"),
                        ("exchange", 6), ("sample",), ("bridge", BT.ACCEPTANCE_SET), ("bridge_blocks",),
                        ("respace", RP.FLOW, 1.0, 0.01, "own"), ("respace_status",), ("bridge_blocks",), ("corr_blocks",), ("walkers",),
                        ("gaps",), ("refused", "mask"), ("sample",), ("bridge", BT.ACCEPTANCE_SET), ("bridge_blocks",), ("corr_blocks",),
                        ("get_ladder",)],
                beta_ratio=1.15, chain_offset=8 * 2 ** 19),
    # Move counters uploaded behind the window base: status 2 and a new window; a table written then resets the record and keeps the
    # base; the tuning after it reads the window from that base
    pinned_case(3, 85, [("table",), ("single", 4), ("window_restart",), ("recount", 0), ("window",),
                        ("tune", 0.44, 1.0, 1, 1e-100, 1e100, False), ("tune_status",), ("window",), ("multi", 3), ("table",),
                        ("tune_status",), ("window",), ("multi", 5), ("tune", 0.44, 0.5, 1, 0.05, 0.5, False), ("tune_status",), ("window",),
                        ("state",), ("mark", "x"), ("corr_fetch",), ("mark", "energy"), ("corr_put",), ("corr_fetch",)],
                sigma=[0.8, 0.11], weight=[0.625, 0.375]),
    # a partition with a chunk of one ladder on a shard that holds chain id 2^32, R = 3
    pinned_case(3, 171, [("blocks", 64, 1), ("bridge", BT.ALL), ("mark", "x"), ("single", 2), ("exchange", 2), ("sample",), ("bridge", BT.ALL),
                         ("bridge_blocks",), ("corr_blocks",), ("bridge_fetch",), ("corr_fetch",), ("blocks_off",), ("refused", "fetch_blocks"),
                         ("bridge_fetch",), ("corr_fetch",), ("mark", "x"), ("single", 1), ("sample",), ("corr_fetch",), ("corr_clear",),
                         ("corr_put",), ("sample",), ("corr_fetch",), ("bridge", BT.E), ("bridge_fetch",), ("bridge_reset",),
                         ("bridge_put", True), ("bridge", BT.E), ("bridge_fetch",)],
                potential="double_well", chain_offset=((TWO32 - 256) // 18) * 18),
    # Float32 state: the respacing rounds the ladder once, the bridge differences are formed in Float32 from the rounded values
    pinned_case(5, 85, [("exchange", 8), ("respace", RP.ACCEPTANCE, 0.7, 0.01, "own"), ("respace_status",), ("get_ladder",), ("bridge", BT.ALL),
                        ("bridge_fetch",), ("single", 2), ("bridge", BT.ALL), ("bridge_fetch",), ("get_ladder",), ("upload", True), ("get_ladder",),
                        ("bridge", BT.ALL), ("bridge_fetch",), ("mark", "energy"), ("exchange", 1), ("sample",), ("corr_fetch",),
                        ("upload", False), ("corr_fetch",), ("corr_put",), ("sample",), ("corr_fetch",)],
                dtype="f32", sigma=[0.5]),
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
            "table", "table", "clear", "sigma", "track", "track", "untrack", "labels", "xcounters", "tx", "ladder", "recount",
            # the ladder tools
            "bridge", "bridge", "bridge", "bridge_reset", "bridge_put", "respace", "respace", "respace", "tune", "tune", "tune",
            "window_restart", "window_base", "mark", "mark", "sample", "sample", "sample", "corr_clear", "corr_put", "corr_put", "corr_put", "blocks", "blocks",
            "blocks_off", "upload", "refused", "refused"]
OLD_OBSERVERS = ["state", "counters", "gaps", "walkers", "rung_sums", "rung_hist", "rung_totals", "reduce"]
NEW_OBSERVERS = ["get_ladder", "respace_status", "tune_status", "window", "bridge_fetch", "corr_fetch", "bridge_blocks", "corr_blocks"]
OBSERVERS = OLD_OBSERVERS + NEW_OBSERVERS
OBSERVER_DRAW = OBSERVERS + ["bridge_fetch", "corr_fetch"]      # the two whose records the walk hands back later
NEW_OPERATIONS = ["bridge", "bridge_reset", "bridge_put", "respace", "tune", "window_restart", "window_base", "mark", "sample", "corr_clear",
                  "corr_put", "blocks", "blocks_off", "upload", "refused"] + NEW_OBSERVERS
OPERATIONS = sorted(set(MUTATORS)) + OBSERVERS
OBSERVER_SHARE = 0.36            # of the draws; the host test holds the walks to at most 40 % observers
MIN_MUTATORS = 8                 # mutating operations taken by every walk
T_X_VALUES = [0, 1, TWO32 - 1, TWO32, 1 << 47, T_X_LIMIT - 3]
RECOUNT_STEPS = [0, 17, 65_530, 65_535, 65_536, 70_000]
REFUSALS = ["mask", "sample", "put_bridge", "put_corr", "fetch_blocks", "tune", "flow"]


def other_ladders(ref):
    """The R' != R that this shard can take: divisors of n_chains and of the offset (and so of the global count)."""
    return [r for r in range(2, 65) if r != ref.n_rungs and ref.n_chains % r == 0 and ref.offset % r == 0]


def new_context():
    """What a walk keeps beside the two sides: snapshots and samples taken, and what the fetch observers have returned (the records that
    bridge_put, corr_put and the refused restores hand back)."""
    return dict(snapshots=0, samples=0, bridge=None, corr=None)


def windowed(ref):
    """The amc_rung_window_* entries: a ladder, per-chain counters, K R <= 64."""
    return ref.per_chain_counters and ref.n_moves * ref.n_rungs <= 64


def stash_fits(ref, stash):
    return stash is not None and stash["R"] == ref.n_rungs


def refusals(ref, ctx):
    """The calls of the fixed list that the handle, as it is now, must refuse with AMC_ERR_STATE."""
    out = []
    if ref.bridge_mask:
        out.append("mask")
    if ref.corr is None:
        out.append("sample")
    if ref.partition is not None and stash_fits(ref, ctx["bridge"]):
        out.append("put_bridge")
    if ref.partition is not None and stash_fits(ref, ctx["corr"]):
        out.append("put_corr")
    if ref.partition is None:
        out.append("fetch_blocks")
    if ref.table is None:
        out.append("tune")
    if not ref.tracking:
        out.append("flow")
    return out


def possible(ref, name, ctx=None):
    """Whether the handle, as it is now, takes operation `name`."""
    ctx = ctx if ctx is not None else new_context()
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
    if name == "bridge":
        return ctx["snapshots"] < MAX_SNAPSHOTS
    if name == "bridge_put":
        return ref.partition is None
    if name in ("tune", "tune_status"):
        return ref.table is not None
    if name in ("window_restart", "window_base", "window"):
        return windowed(ref)
    if name == "sample":
        return ref.corr is not None and ctx["samples"] < MAX_SAMPLES
    if name == "mark":
        return ctx["samples"] < MAX_SAMPLES
    if name == "corr_put":
        return ref.partition is None and stash_fits(ref, ctx["corr"])
    if name in ("blocks_off", "bridge_blocks", "corr_blocks"):
        return ref.partition is not None
    if name == "refused":
        return bool(refusals(ref, ctx))
    return True


def draw_op(rng, ref, steps_left, ctx=None, mutator=False):
    """One operation the handle can take, with its scalar arguments: a tuple (name, ...).  Arrays are drawn when it is applied.
    `mutator`: no observer."""
    ctx = ctx if ctx is not None else new_context()
    for _ in range(64):
        name = str(rng.choice(OBSERVER_DRAW if not mutator and rng.random() < OBSERVER_SHARE else MUTATORS))
        if not possible(ref, name, ctx):
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
            if rng.random() < 0.4:
                continue
            return (name, int(rng.choice(other_ladders(ref))))
        if name == "recount":
            return (name, int(rng.choice(RECOUNT_STEPS)))
        if name == "rung_sums":
            return (name, int(rng.integers(1, 8)))
        if name == "rung_hist":
            return (name, int(rng.choice([7, 200, 4000])), bool(rng.random() < 0.5))
        if name == "bridge":                # the first one after a reset draws the mask
            if ref.bridge_mask:
                return (name, ref.bridge_mask)
            return (name, int(rng.choice([BT.ACCEPTANCE_SET, BT.ALL, BT.E, int(rng.integers(1, BT.ALL + 1))])))
        if name == "bridge_put":
            return (name, bool(stash_fits(ref, ctx["bridge"]) and rng.random() < 0.7))
        if name == "respace":
            rule = RP.FLOW if rng.random() < 0.5 else RP.ACCEPTANCE
            counts = str(rng.choice(["own", "own", "explicit", "explicit", "zero", "flat"]))
            if rule == RP.FLOW and counts == "own" and not ref.tracking:
                rule = RP.ACCEPTANCE
            gamma = 1.0 if rng.random() < 0.5 else float(1.0 - rng.random())         # (0, 1]
            return (name, rule, gamma, float(rng.choice([0.0, 0.01, 0.5])), counts)
        if name == "tune":
            lo, hi = [(1e-100, 1e100), (1e-100, 1e100), (0.05, 0.5), (0.9, 1.1)][int(rng.integers(0, 4))]
            gamma = 1.0 if rng.random() < 0.5 else float(1.0 - rng.random())
            return (name, float(rng.choice([0.2, 0.44, 0.7])), gamma, int(rng.choice([1, 50, 10 ** 6])), lo, hi, bool(rng.random() < 0.4))
        if name == "mark":
            return (name, str(rng.choice(["energy", "x"])))
        if name == "blocks":
            return (name, int(rng.choice([2, 3, 32, 64])), int(rng.choice([0, 1, 5, ref.n_chains // ref.n_rungs])))
        if name == "upload":
            return (name, bool(rng.random() < 0.5))
        if name == "refused":
            return (name, str(rng.choice(refusals(ref, ctx))))
        return (name,)
    return ("single", 1) if mutator else ("state",)


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


def apply_op(op, sides, rng, ref, ctx=None):
    """`sides` take a mutating operation of a handle in the state `ref` is in; its arrays are drawn here from rng.  `ctx`: the walk's
    context (new_context), for the operations that hand earlier fetches back."""
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
    elif name == "bridge":
        for s in sides:
            s.bridge_accumulate(op[1])
    elif name == "bridge_reset":
        for s in sides:
            s.bridge_fetch(reset=True)
    elif name == "bridge_put":
        stash = ctx["bridge"] if op[1] else None
        for s in sides:
            s.set_bridge(*((stash["records"], stash["n"]) if stash else (None, 0)))
    elif name == "respace":
        counts = respace_counts(rng, op[1], op[4], R, M // R)
        for s in sides:
            s.respace_ladder(op[1], op[2], op[3], counts)
    elif name == "tune":
        counts = None
        if op[6]:                           # a global window: a few thousand calls per cell, or none at all in some
            tot = rng.integers(0, 5000, (K, R))
            if rng.random() < 0.3:
                tot = tot * rng.integers(0, 2, (K, R))
            counts = ((tot * rng.uniform(0, 1, (K, R))).astype(np.int64), tot.astype(np.int64))
        for s in sides:
            s.tune_rung_sigma(op[1], op[2], op[3], op[4], op[5], counts)
    elif name == "window_restart":
        for s in sides:
            s.rung_window_restart()
    elif name == "window_base":             # around the counters as they stand: some cells end up ahead of them
        acc, tot = ref.rung_counter_totals()
        bt = np.maximum(0, tot + rng.integers(-40, 8, tot.shape))
        ba = np.minimum(bt, np.maximum(0, acc + rng.integers(-40, 3, acc.shape)))
        for s in sides:
            s.set_rung_window_base(ba, bt)
    elif name == "mark":
        for s in sides:
            s.corr_mark(op[1])
    elif name == "sample":
        for s in sides:
            s.corr_sample()
    elif name == "corr_clear":
        for s in sides:
            s.corr_clear()
    elif name == "corr_put":
        c = ctx["corr"]
        for s in sides:
            s.set_corr(c["observable"], c["origin"], c["records"], c["steps"])
    elif name == "blocks":
        for s in sides:
            s.set_blocks(op[1], op[2])
    elif name == "blocks_off":
        for s in sides:
            s.set_blocks(0, 0)
    elif name == "upload":
        x = rng.normal(0.0, 1.5, M)
        if ref.dtype == "f32":
            x = x.astype(np.float32).astype(np.float64)
        beta = None
        if op[1]:                           # a geometric ladder of another ratio, or per-chain values that no ladder repeats
            beta = (0.4 * rng.uniform(1.05, 2.0) ** np.arange(R))[np.arange(M) % R] if rng.random() < 0.7 else rng.uniform(0.2, 3.0, M)
        for s in sides:
            s.upload_state(x, beta)
    else:
        raise ValueError(op)


def respace_counts(rng, rule, kind, R, L):
    """The GLOBAL counts of a respacing: None (the handle's own); "explicit" ones that the rule can use; "zero": a count the rule
    divides by is zero (status 2); "flat": no weight to spread (status 1)."""
    if kind == "own":
        return None
    if rule == RP.ACCEPTANCE:
        att = rng.integers(1, 50 * L + 2, R - 1)
        acc = (att * rng.uniform(0, 1, R - 1)).astype(np.int64)
        if kind == "zero":
            j = int(rng.integers(0, R - 1))
            att[j] = acc[j] = 0
        if kind == "flat":
            acc = att.copy()
        return np.concatenate([att, acc]).astype(np.uint64)
    n = np.zeros((R, 3), dtype=np.int64)
    f = np.sort(rng.uniform(0, 1, R))[::-1]
    if kind == "flat":
        f[:] = 0.5
    tot = rng.integers(1, 50 * L + 2, R)
    n[:, 1] = np.round(f * tot).astype(np.int64)
    n[:, 2] = tot - n[:, 1]
    n[:, 0] = rng.integers(0, L + 1, R)
    if kind == "zero":
        n[int(rng.integers(0, R)), 1:] = 0
    return n.astype(np.uint64)


def refuse(which, side, ref, ctx):
    """The call `which` of the fixed list on `side`: the exception it raised, or None when the side took it."""
    try:
        if which == "mask":
            side.bridge_accumulate(BT.ALL if ref.bridge_mask != BT.ALL else BT.E)
        elif which == "sample":
            side.corr_sample()
        elif which == "put_bridge":
            side.set_bridge(ctx["bridge"]["records"], ctx["bridge"]["n"])
        elif which == "put_corr":
            c = ctx["corr"]
            side.set_corr(c["observable"], c["origin"], c["records"], c["steps"])
        elif which == "fetch_blocks":
            side.bridge_fetch_blocks()
        elif which == "tune":
            side.tune_rung_sigma(0.44, 1.0, 1, 1e-100, 1e100, None)
        elif which == "flow":
            side.respace_ladder(RP.FLOW, 1.0, 0.0, None)
        else:
            raise ValueError(which)
    except (AssertionError, ValueError):
        raise
    except Exception as exc:
        return exc
    return None


def is_state_error(exc):
    """An AmcError (the engine) or a Refused (the reference) that carries AMC_ERR_STATE."""
    return type(exc).__name__ in ("AmcError", "Refused") and str(exc).startswith(f"amc error {ERR_STATE}:")


def observe(op, eng, ref, rng, fail, ctx=None):
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
    elif name == "get_ladder":             # (the mutator "ladder" is set_ladder)
        got, want = eng.ladder(), ref.ladder()
        if not same_floats(got, want):
            fail("the ladder differs", (got, want))
    elif name == "respace_status":
        if tuple(eng.respace_status()) != tuple(ref.respace_status()):
            fail("respacing status differs", (eng.respace_status(), ref.respace_status()))
    elif name == "tune_status":
        (st, n), (sto, no) = eng.tune_status(), ref.tune_status()
        if not same_ints(st, sto) or n != no:
            fail("tuning status differs", (st, n, sto, no))
        if not same_words(eng.rung_sigma(), ref.rung_sigma()):
            fail("the table differs", (eng.rung_sigma(), ref.rung_sigma()))
    elif name == "window":
        for what, (a, t), (ao, to) in (("counts", eng.rung_window_counts(), ref.rung_window_counts()),
                                       ("base", eng.rung_window_base(), ref.rung_window_base())):
            if not (same_ints(a, ao) and same_ints(t, to)):
                fail(f"window {what} differ", (a, ao, t, to))
    elif name == "bridge_fetch":
        (rec, n), (reco, no) = eng.bridge_fetch(), ref.bridge_fetch()
        if n != no or not same_words(rec, reco):
            fail("bridge records differ", (n, no, np.argwhere(fbits(rec) != fbits(reco))[:4] if np.shape(rec) == np.shape(reco) else None))
        if ctx is not None and no > 0:
            ctx["bridge"] = dict(R=ref.n_rungs, records=reco, n=no)
    elif name == "corr_fetch":
        (rec, st, ob), (reco, sto, obo) = eng.corr_fetch(), ref.corr_fetch()
        if ob != obo or not same_ints(st, sto) or not same_words(rec, reco):
            fail("correlation records differ", (ob, obo, st, sto))
        if obo:
            org, orgo = eng.corr_origin(), ref.corr_origin()
            if not same_floats(org, orgo):
                fail("the origin differs", np.flatnonzero(fbits(org) != fbits(orgo))[:8])
            if ctx is not None:
                ctx["corr"] = dict(R=ref.n_rungs, observable=obo, origin=orgo, records=reco, steps=sto)
    elif name == "bridge_blocks":
        (blk, n), (blko, no) = eng.bridge_fetch_blocks(), ref.bridge_fetch_blocks()
        if n != no or not same_words(blk, blko):
            fail("bridge records per block differ", (n, no, np.shape(blk), np.shape(blko)))
        if not same_words(BL.merge_blocks(blk), eng.bridge_fetch()[0]):
            fail("the merge over the blocks is not the merged bridge fetch")
    elif name == "corr_blocks":
        (blk, st, ob), (blko, sto, obo) = eng.corr_fetch_blocks(), ref.corr_fetch_blocks()
        if ob != obo or not same_ints(st, sto) or not same_words(blk, blko):
            fail("correlation records per block differ", (ob, obo, st, sto, np.shape(blk), np.shape(blko)))
        if len(sto) and not same_words(BL.merge_blocks(blk), eng.corr_fetch()[0]):
            fail("the merge over the blocks is not the merged correlation fetch")
    else:
        raise ValueError(op)


def same_words(a, b):
    """Records word for word (every word of a record is an integer held in a Float64: no NaN)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(fbits(a), fbits(b))


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
    ctx = new_context()
    taken = 0                    # mutating operations taken
    respaced_under_mark = tuned = retabled = False
    wanted = 0 if script else MIN_MUTATORS      # (a pinned case runs its script and n_ops operations, no more)
    while len(ops) < max(n_ops, len(script)) or taken < wanted:
        op = queue.pop(0) if queue else draw_op(rng, ref, steps_left, ctx, mutator=len(ops) >= max(n_ops, len(script)))
        name = op[0]
        ops.append(op)
        if name in OBSERVERS:
            if not possible(ref, name, ctx):
                fail("the script asks for an observation the handle cannot give")
            observe(op, engine, ref, rng, fail, ctx)
            if name == "walkers" and case.get("beta_kind") == "equal" and min(ref.tracking_counters()) >= 1:
                events.add("equal beta with tracking: a round trip and an up trip")
            continue
        if not possible(ref, name, ctx) or (name == "refused" and op[1] not in refusals(ref, ctx)):
            fail("the script asks for an operation the handle cannot take")
        if name == "refused":                  # both sides refuse with AMC_ERR_STATE; the observers that follow show nothing moved
            for side, who in ((engine, "the engine"), (ref, "the reference")):
                exc = refuse(op[1], side, ref, ctx)
                if exc is None or not is_state_error(exc):
                    fail(f"{who} did not refuse with AMC_ERR_STATE: {exc!r}")
            continue
        taken += 1
        before = dict(n=ref.bridge_n, marked=ref.corr is not None, respaced=ref.respace_status()[1])
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
            apply_op(op, (engine,), np.random.default_rng(arrays), ref, ctx)
        except AssertionError:
            raise
        except Exception as exc:               # a refusal by the engine of something the reference takes
            fail(f"the engine refused: {exc!r}")
        if after_op is not None:
            after_op(op)
        apply_op(op, (ref,), np.random.default_rng(arrays), ref, ctx)
        # the combinations of the ladder tools that the host test counts
        if name == "bridge":
            ctx["snapshots"] += 1
            if crossing and ref.partition is not None:
                events.add("partition on a shard across 2^32")
        elif name in ("mark", "sample"):
            ctx["samples"] += 1
            if name == "sample" and respaced_under_mark:
                events.add("respacing with a mark standing, then a sample")
            if name == "mark":
                respaced_under_mark = False
                if crossing and ref.partition is not None:
                    events.add("partition on a shard across 2^32")
        elif name == "respace":
            took = ref.respace_status()[1] > before["respaced"]
            if before["n"]:
                events.add("respacing taken with snapshots accumulated" if took else
                           "respacing not taken (status != 0) with snapshots accumulated")
            if took and ref.partition is not None:
                events.add("respacing taken under a partition")
            if took and ref.dtype == "f32":
                events.add("Float32 ladder respaced")
            respaced_under_mark = respaced_under_mark or before["marked"]
            if op[4] != "own" and ref.offset > 0:
                events.add("explicit counts on a shard that does not start at 0")
        elif name == "tune":
            st = ref.tune_status()[0]
            if np.any(st == TU.INCONSISTENT):
                events.add("tuning with an inconsistent window")
            if np.any(st == TU.CLAMPED):
                events.add("tuning that clamps")
            if tuned and retabled:
                events.add("table rewritten between two tunings")
            tuned, retabled = True, False
            if op[6] and ref.offset > 0:
                events.add("explicit counts on a shard that does not start at 0")
        elif name == "table":
            retabled = tuned
        elif name in ("clear", "ladder"):
            tuned = retabled = False
        elif name == "upload" and before["marked"]:
            events.add("upload with a mark standing")
        elif name == "blocks" and before["n"]:
            events.add("set_blocks with snapshots accumulated")
        if ref.corr is None:
            respaced_under_mark = False
    if case.get("plant"):
        events.add("non-finite positions")
    # the end: everything
    ops.append(("end",))
    for name in OBSERVERS:
        if possible(ref, name, ctx):
            observe((name, 7) if name == "rung_sums" else (name, 200, False) if name == "rung_hist" else (name,), engine, ref, rng, fail)
    if engine.step != ref.step:
        fail("step index differs", (engine.step, ref.step))
    if engine.exchange_step != ref.exchange_step:
        fail("exchange step index differs", (engine.exchange_step, ref.exchange_step))
    if engine.estimator_step != ref.estimator_step:
        fail("estimator step index differs", (engine.estimator_step, ref.estimator_step))
    return dict(ops=ops[:-1], events=events, taken=taken)


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
