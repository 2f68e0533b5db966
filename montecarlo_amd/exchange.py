"""``ReplicaExchange``: parallel tempering along a temperature ladder, on the device.

An extension over the reference.  There a user who wants replica exchange writes an ``AriannaAlgorithm`` whose ``make_step!`` walks
``simulation.chains`` and swaps neighbours (the plugin protocol, src/algorithms.jl:6-37, hands every algorithm the chains); here the
chains live in HBM behind the C ABI, so the engine provides the cross-chain move (include/amc.h) and this
algorithm schedules it like any other.

Ladder l is the R consecutive global chain ids [l R, (l + 1) R); the rung of chain c is c mod R and its beta is whatever the per-chain
beta array holds (``ParticleChains.ladder`` tiles a list of betas).  One exchange step attempts, in every ladder, the gaps of one
parity; the parity alternates from step to step.  An accepted swap exchanges the POSITIONS of the two chains: beta, the Move counters
and everything else indexed by chain stay with the rung, so ``x[r::R]`` is always the sample at beta_r.

``track=True`` turns walker tracking on (DESIGN.md section 3.13 "Walker tracking"): the engine carries one label per chain -- which
replica sits there and which end of the ladder it visited last -- through every accepted swap, and ``flow()`` / ``round_trips()``
answer whether replicas actually travel between the hot and the cold end, which the acceptance per gap alone cannot.

``bridge=True`` accumulates the bridge sums (DESIGN.md section 3.13 "Bridge sums") on the device while the run goes on: per rung the
reproducible sums of the energy, its square and the neighbour-reweighting factors.  ``log_z_ratios()`` / ``log_z()`` turn them into
free-energy differences along the ladder, ``heat_capacity()`` into the heat capacity per rung.
"""
from __future__ import annotations

import numpy as np

from . import jackknife, sharding
from ._capi import (AMC_BRIDGE_ALL, AMC_BRIDGE_E, AMC_BRIDGE_EE, AMC_BRIDGE_MB, AMC_BRIDGE_MF, AMC_BRIDGE_WB, AMC_BRIDGE_WF, AMC_MAX_MOVES,
                    AMC_RED_HEADER, AMC_REDUCE_ALL, AMC_REDUCE_E, AMC_REDUCE_X, AMC_REDUCE_XX, AMC_XSUM_WORDS, xsum_round)
from .metropolis import Metropolis
from .simulation import AriannaAlgorithm, Simulation, _calls
from .system import potential as _potential


# Records per all-reduce of rung_sums: amc_allreduce_xsum takes what the communicator's buffers hold, never less than the records of
# one callback reduction (AMC_RED_HEADER + AMC_MAX_MOVES per rank, amc_comm_init); the 3 R records of a ladder reach 192.
XSUM_CHUNK = AMC_RED_HEADER + AMC_MAX_MOVES


class ReplicaExchange(AriannaAlgorithm):
    """ReplicaExchange(chains; dependencies=(Metropolis,), n_rungs=R): one exchange step of the Metropolis' engine per scheduled time.

    Listed behind its Metropolis, a time step at which both are due is [sweep; exchange], and ``run(fuse=True)`` queues a stretch
    of such rounds that nothing else observes with one engine call (``sweep_exchange``): the same launches, the same results.

    ``bridge``: False, True (the acceptance set E | EE | MF | MB, what the default estimators read) or a mask of AMC_BRIDGE_* bits;
    after every ``bridge_every``-th exchange step one snapshot of the bridge sums is queued behind it (nothing synchronises), and a
    fused stretch is cut at those steps, so fused and stepwise runs accumulate the same records.

    ``blocks=B`` (2..64) keeps the bridge sums per block of ladders, block of ladder l = (l div block_chunk) mod B (DESIGN.md section
    3.16; ``block_chunk`` None: max(1, 256 div R) ladders), and ``log_z_ratios`` / ``log_z`` / ``heat_capacity`` take ``error=True``:
    (value, se), se from the delete-one-block jackknife over the B blocks.  The values themselves do not change by a bit."""

    BRIDGE_DEFAULT = AMC_BRIDGE_E | AMC_BRIDGE_EE | AMC_BRIDGE_MF | AMC_BRIDGE_MB

    mutates_chains = True          # a callback due behind it at the same t observes the state AFTER the swaps (simulation._observed_next)

    def __init__(self, chains, dependencies=None, n_rungs=None, path=None, track=False, bridge=False, bridge_every=1, blocks=None,
                 block_chunk=None, **extras):
        assert dependencies is not None and len(dependencies) == 1 and isinstance(dependencies[0], Metropolis)
        self.metropolis: Metropolis = dependencies[0]
        if n_rungs is None:
            n_rungs = getattr(chains, "n_rungs", None)
        if n_rungs is None:
            raise ValueError("ReplicaExchange: n_rungs is missing (and the chains were not made by ParticleChains.ladder)")
        self.n_rungs = int(n_rungs)
        self.track = bool(track)
        if bridge is True:
            self.bridge = self.BRIDGE_DEFAULT
        elif bridge is False or bridge is None:
            self.bridge = 0
        else:
            self.bridge = int(bridge)
            if self.bridge <= 0 or self.bridge & ~AMC_BRIDGE_ALL:
                raise ValueError(f"ReplicaExchange: bridge = {bridge!r} is neither a bool nor a non-empty mask of AMC_BRIDGE_* bits")
        if int(bridge_every) != bridge_every or int(bridge_every) < 1:
            raise ValueError(f"ReplicaExchange: bridge_every = {bridge_every!r} must be an integer >= 1")
        self.bridge_every = int(bridge_every)
        self.metropolis.bridge = self.bridge           # (storage.checkpoint: the accumulator is state while the bridge is on)
        self.blocks = jackknife.check_blocks("ReplicaExchange", blocks, block_chunk, len(chains) // self.n_rungs, self.n_rungs)
        if self.blocks:                                # (storage.checkpoint: the records per block are state; an Autocorrelation shares them)
            jackknife.ask_blocks("ReplicaExchange", self.metropolis, self.blocks)
        self.rank, _ = sharding.world()

    def initialise(self, simulation: Simulation) -> None:
        self.metropolis.set_ladder(self.n_rungs)       # (the per-chain beta array is on the device by now: Metropolis comes first)
        if self.blocks:
            jackknife.refuse_annealing("ReplicaExchange", simulation)
            jackknife.use_blocks(self.metropolis, self.blocks)
        if self.track and not self.metropolis.tracking:     # (on already: storage.restore brought the labels back)
            self.metropolis.engine.set_tracking(True)
            self.metropolis.tracking = True

    def _bridge_due(self) -> bool:
        """The exchange step just queued was a ``bridge_every``-th one (the engine's step index: a resumed run keeps the rhythm)."""
        return self.metropolis.engine.exchange_step % self.bridge_every == 0

    def make_step(self, simulation: Simulation) -> None:
        self.metropolis.engine.exchange(1)
        self.metropolis.invalidate_reductions()
        if self.bridge and self._bridge_due():
            self.metropolis.engine.bridge_accumulate(self.bridge)

    def make_rounds(self, simulation: Simulation, n_rounds: int, sweeps_per_round: int) -> None:
        """n_rounds x [sweeps_per_round x make_step!(::Metropolis); make_step!(::ReplicaExchange)] as one engine call -- with the
        bridge on, one call up to each exchange step behind which a snapshot is due, then the snapshot."""
        if not self.bridge:
            self.metropolis.sweep_exchange(n_rounds, sweeps_per_round)
            return
        eng, left = self.metropolis.engine, int(n_rounds)
        while left > 0:
            n = min(left, self.bridge_every - eng.exchange_step % self.bridge_every)
            self.metropolis.sweep_exchange(n, sweeps_per_round)
            left -= n
            if self._bridge_due():
                eng.bridge_accumulate(self.bridge)

    def acceptance(self) -> np.ndarray:
        """Accepted / attempted swaps per gap over ALL shards, R - 1 ratios (0/0 = NaN before the first attempt)."""
        acc, att = self.metropolis.engine.exchange_counters()
        tot = sharding.allreduce_sum(np.concatenate([acc, att]).astype(np.float64), self.metropolis.engine)
        n = self.n_rungs - 1
        with np.errstate(invalid="ignore", divide="ignore"):
            return tot[:n] / tot[n:]

    def _need_tracking(self, what: str) -> None:
        if not self.track:
            raise ValueError(f"{what} needs walker tracking: build the ReplicaExchange with track=True")

    def flow(self) -> np.ndarray:
        """The flow fraction per rung over ALL shards, R values: of the replicas at rung r that have visited an end, the share that
        last visited rung 0 -- f(0) = 1, f(R - 1) = 0, 0/0 = NaN where no replica has been to an end yet.  A ladder that works
        falls about linearly in between; a step marks the bottleneck.  The host waits for the queued steps."""
        self._need_tracking("ReplicaExchange.flow")
        eng = self.metropolis.engine
        n = sharding.allreduce_sum(eng.flow_rungs().astype(np.float64).reshape(-1), eng).reshape(self.n_rungs, 3)
        with np.errstate(invalid="ignore", divide="ignore"):
            return n[:, 1] / (n[:, 1] + n[:, 2])

    def round_trips(self) -> np.ndarray:
        """(round_trips, up_trips) over ALL shards since tracking was turned on: arrivals at rung 0 of a replica that last visited
        rung R - 1, and arrivals at rung R - 1 of one that last visited rung 0.  The host waits for the queued steps."""
        self._need_tracking("ReplicaExchange.round_trips")
        eng = self.metropolis.engine
        return sharding.allreduce_sum(np.array(eng.tracking_counters(), dtype=np.float64), eng)

    def rung_sums(self, columns: int = AMC_REDUCE_ALL) -> np.ndarray:
        """Per rung the means of e, x and x^2 over the ladders of ALL shards: an array of shape (R, 3), column c = 0 <e>, 1 <x>,
        2 <x^2> (NaN for a column ``columns``, AMC_REDUCE_* bits, does not name).  Reproducible sums formed on the device
        (amc_reduce_rungs_exact): the shards' integer records are merged, rounded once and divided by the
        global ladder count, so the bits do not depend on the split into shards.  The host waits for the queued steps."""
        eng = self.metropolis.engine
        rec = np.ascontiguousarray(eng.reduce_rungs(columns), dtype=np.float64).reshape(-1, AMC_XSUM_WORDS)
        merged = np.concatenate([sharding.allreduce_xsum(rec[i:i + XSUM_CHUNK], eng).reshape(-1, AMC_XSUM_WORDS)
                                 for i in range(0, rec.shape[0], XSUM_CHUNK)])
        sums = xsum_round(merged).reshape(self.n_rungs, 3)
        asked = np.array([bool(int(columns) & bit) for bit in (AMC_REDUCE_E, AMC_REDUCE_X, AMC_REDUCE_XX)])
        out = sums / float(len(self.metropolis.chains) // self.n_rungs)
        out[:, ~asked] = np.nan
        return out

    # ---- bridge sums: free-energy differences along the ladder (DESIGN.md section 3.13 "Bridge sums") ----
    def _need_bridge(self, what: str, columns: int) -> None:
        if not self.bridge:
            raise ValueError(f"{what} needs the bridge sums: build the ReplicaExchange with bridge=True")
        if columns & ~self.bridge:
            raise ValueError(f"{what} reads bridge columns {columns & ~self.bridge} that the mask bridge = {self.bridge} leaves out")

    def _same_snapshots(self, what: str, n: int) -> None:
        """Every shard holds ``n`` snapshots: the means divide by n times the global ladders."""
        counts = sharding.allreduce_sum(np.array([float(n), float(n) * float(n), 1.0]), self.metropolis.engine)
        if counts[0] != n * counts[2] or counts[1] != float(n) * float(n) * counts[2]:
            raise RuntimeError(f"{what}: this shard holds {n} snapshots, the shards' mean is {counts[0] / counts[2]}")

    def bridge_sums(self):
        """(sums, n_snapshots): the accumulated bridge sums over the ladders of ALL shards, an array of shape (R, 6) in the column
        order E, EE, WF, WB, MF, MB -- NaN where a column is outside the mask or a rung has no such summand (WF, MF at rung R - 1, WB, MB
        at rung 0) --, and the number of snapshots in them.  The shards' integer records are merged and rounded once (as rung_sums),
        so the bits do not depend on the split into shards; a record that met a NaN or an infinity reads NaN / +-Inf.  The host
        waits for the queued steps; the accumulator goes on."""
        if not self.bridge:
            raise ValueError("ReplicaExchange.bridge_sums needs the bridge sums: build the ReplicaExchange with bridge=True")
        eng = self.metropolis.engine
        rec, n = eng.bridge_fetch(reset=False)
        self._same_snapshots("ReplicaExchange.bridge_sums", n)
        rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, AMC_XSUM_WORDS)
        merged = np.concatenate([sharding.allreduce_xsum(rec[i:i + XSUM_CHUNK], eng).reshape(-1, AMC_XSUM_WORDS)
                                 for i in range(0, rec.shape[0], XSUM_CHUNK)])
        empty = ~merged.any(axis=1)
        sums = xsum_round(merged)
        sums[empty] = np.nan
        return sums.reshape(self.n_rungs, 6), n

    def _bridge_means(self, what: str, columns: int):
        self._need_bridge(what, columns)
        sums, n = self.bridge_sums()
        with np.errstate(invalid="ignore", divide="ignore"):
            return sums, sums / (float(n) * float(len(self.metropolis.chains) // self.n_rungs))

    def _merged(self, rec) -> np.ndarray:
        """Records merged over the shards, XSUM_CHUNK of them per all-reduce (rung_sums)."""
        eng = self.metropolis.engine
        flat = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, AMC_XSUM_WORDS)
        return np.concatenate([sharding.allreduce_xsum(flat[i:i + XSUM_CHUNK], eng).reshape(-1, AMC_XSUM_WORDS)
                               for i in range(0, flat.shape[0], XSUM_CHUNK)]).reshape(np.shape(rec))

    def bridge_blocks(self):
        """(records[B][R][6][AMC_XSUM_WORDS], n_snapshots, ladders[B]): the accumulated bridge sums per jackknife block over ALL
        shards -- the shards' records merged block by block -- and the ladders of every block.  Needs ``blocks``.  The host waits."""
        if not self.bridge or not self.blocks:
            raise ValueError("ReplicaExchange.bridge_blocks needs bridge=True and blocks=B")
        rec, n = self.metropolis.engine.bridge_fetch_blocks(reset=False)
        self._same_snapshots("ReplicaExchange.bridge_blocks", n)
        return self._merged(rec), n, jackknife.block_counts(len(self.metropolis.chains) // self.n_rungs, *self.blocks)

    def _estimate(self, what: str, columns: int, fn, error: bool):
        """fn(sums[R][6], means[R][6]) of the accumulated bridge sums; with ``error`` (value, se), the same fn on every leave-one-out
        merge of the blocks (jackknife.jackknife)."""
        if not error:
            return fn(*self._bridge_means(what, columns))
        self._need_bridge(what, columns)
        if not self.blocks:
            raise ValueError(f"{what}: error=True needs the sums per block: build the ReplicaExchange with blocks=B")
        rec, n, ladders = self.bridge_blocks()

        def of_merge(values, n_ladders):
            sums = np.where(values == 0.0, np.nan, values)      # (an all-zero record: a column outside the mask, an end rung's missing slot)
            with np.errstate(invalid="ignore", divide="ignore"):
                return fn(sums, sums / (float(n) * float(n_ladders)))
        return jackknife.jackknife(rec, ladders, of_merge)

    def log_z_ratios(self, method: str = "acceptance", error: bool = False):
        """log(Z_(r+1) / Z_r) for the R - 1 gaps of the ladder, Z_r = integral of exp(-beta_r U), from the accumulated bridge sums.

        "acceptance" (default): Bennett's identity with the Metropolis function at C = 0, log S_MF[r] - log S_MB[r + 1] -- both
            rungs hold the same number of samples, so the count cancels.  Its summands lie in [0, 1]: finite variance whatever the
            ladder.  R - 1 numbers.
        "exponential": the two one-sided exponential averages, shape (2, R - 1): row 0 log(S_WF[r] / N) (forward, samples of rung r),
            row 1 -log(S_WB[r + 1] / N) (backward, samples of rung r + 1), N = snapshots x global ladders.  The backward average has
            INFINITE variance once beta_(r+1) >= 2 beta_r for a harmonic well (exp((beta_(r+1) - beta_r) e) under exp(-beta_(r+1) e):
            its second moment diverges): read it as a diagnostic, not as an estimate, on a coarse ladder.
        "ti": thermodynamic integration by the trapezoid, -(<e>_r + <e>_(r+1)) (beta_(r+1) - beta_r) / 2, beta from betas().
        An estimate that reads a flagged record (a NaN or an infinity among its summands) is NaN; so is every estimate before the
        first snapshot.  ``error=True`` (needs ``blocks``): (estimates, their jackknife standard errors).  The host waits for the
        queued steps."""
        return self._estimate(*self._ratios_of(method), error)

    def _ratios_of(self, method: str):
        """(what, columns, fn) of log_z_ratios(method)."""
        what = f"ReplicaExchange.log_z_ratios({method!r})"
        if method == "acceptance":
            def fn(sums, mean):
                return np.log(sums[:-1, 4]) - np.log(sums[1:, 5])
            columns = AMC_BRIDGE_MF | AMC_BRIDGE_MB
        elif method == "exponential":
            def fn(sums, mean):
                return np.stack([np.log(mean[:-1, 2]), -np.log(mean[1:, 3])])
            columns = AMC_BRIDGE_WF | AMC_BRIDGE_WB
        elif method == "ti":
            b = self.betas()

            def fn(sums, mean):
                return -0.5 * (mean[:-1, 0] + mean[1:, 0]) * (b[1:] - b[:-1])
            columns = AMC_BRIDGE_E
        else:
            raise ValueError(f"ReplicaExchange.log_z_ratios: method {method!r} is none of 'acceptance', 'exponential', 'ti'")

        def finite(sums, mean):
            with np.errstate(invalid="ignore", divide="ignore"):
                out = fn(sums, mean)
            out[~np.isfinite(out)] = np.nan
            return out
        return what, columns, finite

    def log_z(self, method: str = "acceptance", error: bool = False):
        """log(Z_r / Z_0) per rung, R values: the cumulative sum of log_z_ratios(method) with log Z_0 = 0 ("exponential": shape (2, R)).
        ``error=True``: (values, se), the jackknife of the cumulative sum itself -- the gaps of one ladder are correlated, so their
        errors do not add."""
        what, columns, ratios = self._ratios_of(method)

        def fn(sums, mean):
            d = ratios(sums, mean)
            return np.concatenate([np.zeros(d.shape[:-1] + (1,)), np.cumsum(d, axis=-1)], axis=-1)
        return self._estimate(what.replace("log_z_ratios", "log_z"), columns, fn, error)

    def heat_capacity(self, error: bool = False):
        """beta_r^2 (<e^2> - <e>^2) per rung, R values, from the accumulated bridge sums; beta from betas().  ``error=True``: (values,
        se)."""
        b = self.betas()

        def fn(sums, mean):
            out = b * b * (mean[:, 1] - mean[:, 0] * mean[:, 0])
            out[~np.isfinite(out)] = np.nan
            return out
        return self._estimate("ReplicaExchange.heat_capacity", AMC_BRIDGE_E | AMC_BRIDGE_EE, fn, error)

    def restart_bridge(self) -> None:
        """The accumulator of the bridge sums starts again from nothing (a burn-in ends here).  The host waits for the queued steps."""
        if not self.bridge:
            raise ValueError("ReplicaExchange.restart_bridge needs the bridge sums: build the ReplicaExchange with bridge=True")
        self.metropolis.engine.bridge_fetch(reset=True)

    def betas(self) -> np.ndarray:
        """The ladder as the device holds it now, R beta values (Float32 state: the Float32 values, widened).  The host waits for
        the queued steps."""
        return self.metropolis.engine.ladder()

    def respace(self, rule: str = "flow", gamma: float = 1.0, eps: float = 0.01):
        """Respace the ladder on the device (DESIGN.md section 3.13 "Respacing"): "flow" puts the rungs where the flow fraction
        falls (the feedback-optimised ladder; needs track=True), "acceptance" equalises the rejection rate per gap; ``gamma`` in
        (0, 1] damps the move, ``eps`` in [0, 1) is the floor of a gap's weight.  With one shard the engine uses its own counters and
        nothing is read back before the ladder is; with several the counts are summed over the shards as acceptance() and flow() sum
        them and every shard is given the sums, so all compute the same ladder.  A respacing that is taken (status 0) zeroes the gap
        counters and restarts the tracking: the measurement belongs to a ladder.  ``chains.beta_array`` follows, so a checkpoint
        written afterwards carries the new ladder.  Returns (status, n_respaced) (amc_respace_status).
        Changing beta during a run breaks detailed balance: respace during burn-in (see RespaceLadder)."""
        if rule == "flow":
            self._need_tracking('ReplicaExchange.respace("flow")')
        elif rule != "acceptance":
            raise ValueError(f"ReplicaExchange.respace: rule {rule!r} is neither 'flow' nor 'acceptance'")
        met = self.metropolis
        eng = met.engine
        counts = None
        if sharding.world()[1] > 1:
            if rule == "acceptance":
                acc, att = eng.exchange_counters()
                local = np.concatenate([att, acc])
            else:
                local = eng.flow_rungs().reshape(-1)
            counts = np.rint(sharding.allreduce_sum(local.astype(np.float64), eng)).astype(np.int64)
        eng.respace_ladder(rule, gamma, eps, counts=counts)
        met.invalidate_reductions()
        status = eng.respace_status()
        if status[0] == 0 and met.chains.beta_array is not None:
            ladder = eng.ladder()
            met.chains.beta_array[:] = np.tile(ladder, len(met.chains) // self.n_rungs)
        return status

    def write_algorithm(self, io, scheduler) -> None:
        io.write("\tReplicaExchange\n")
        io.write(f"\t\tCalls: {_calls(scheduler)}\n")
        io.write(f"\t\tRungs: {self.n_rungs}\n")
        io.write(f"\t\tLadders: {len(self.metropolis.chains) // self.n_rungs}\n")


class RespaceLadder(AriannaAlgorithm):
    """RespaceLadder(chains; dependencies=(ReplicaExchange,), rule="flow", gamma=1.0, eps=0.01, until=None): one respacing of the
    ReplicaExchange's ladder per scheduled time (ReplicaExchange.respace), and none after time step ``until``.

    A BURN-IN tool: changing beta in the middle of a run breaks detailed balance, so the samples taken while the ladder still moves
    are not samples of the final ladder's ensemble.  Schedule it over the first part of the run, or give ``until``, and measure
    afterwards.  An algorithm of its own, so the schedule decides when it runs; a time step at which it is due ends a fused stretch
    of ``run(fuse=True)`` like any other algorithm that is due."""

    mutates_chains = True          # (beta moves: a callback due behind it at the same t observes the new ladder)

    def __init__(self, chains, dependencies=None, rule="flow", gamma=1.0, eps=0.01, until=None, path=None, **extras):
        assert dependencies is not None and len(dependencies) == 1 and isinstance(dependencies[0], ReplicaExchange)
        self.exchange: ReplicaExchange = dependencies[0]
        if rule not in ("flow", "acceptance"):
            raise ValueError(f"RespaceLadder: rule {rule!r} is neither 'flow' nor 'acceptance'")
        if rule == "flow" and not self.exchange.track:
            raise ValueError('RespaceLadder: rule "flow" needs walker tracking: build the ReplicaExchange with track=True')
        self.rule, self.gamma, self.eps = rule, float(gamma), float(eps)
        self.until = None if until is None else int(until)
        self.statuses = []         # (t, status) of every respacing asked for

    def make_step(self, simulation: Simulation) -> None:
        if self.until is not None and simulation.t > self.until:
            return
        status, _ = self.exchange.respace(self.rule, self.gamma, self.eps)
        self.statuses.append((simulation.t, status))

    def write_algorithm(self, io, scheduler) -> None:
        io.write("\tRespaceLadder\n")
        io.write(f"\t\tCalls: {_calls(scheduler)}\n")
        io.write(f"\t\tRule: {self.rule}\n")
        io.write(f"\t\tGamma: {self.gamma}\n")
        io.write(f"\t\tEps: {self.eps}\n")
        io.write(f"\t\tUntil: {self.until}\n")


class TuneRungSigma(AriannaAlgorithm):
    """TuneRungSigma(chains; dependencies=(Metropolis,), target=0.44, gamma=1.0, min_calls=1000, sigma_min=1e-100, sigma_max=1e100,
    until=None): one tuning of the Metropolis' widths per rung per scheduled time (Metropolis.tune_rung_sigma), and none after time
    step ``until``.  The window of the acceptance it reads starts when the run starts and restarts at every tuning, so each tuning
    measures the table in force since the one before.

    A BURN-IN tool: changing sigma in the middle of a run breaks detailed balance across the change, so the samples taken while the
    widths still move are not samples of one chain.  Schedule it over the first part of the run, or give ``until``, and measure
    afterwards.  Scheduled behind a RespaceLadder it also answers a ladder that has moved: the widths follow the new beta at the next
    tuning.  An algorithm of its own, so the schedule decides when it runs; a time step at which it is due ends a fused stretch of
    ``run(fuse=True)`` like any other algorithm that is due."""

    mutates_chains = True          # (as RespaceLadder: a callback due behind it at the same t is served after the tuning, not from the launch in front)

    def __init__(self, chains, dependencies=None, target=0.44, gamma=1.0, min_calls=1000, sigma_min=1e-100, sigma_max=1e100, until=None,
                 path=None, **extras):
        assert dependencies is not None and len(dependencies) == 1 and isinstance(dependencies[0], Metropolis)
        self.metropolis: Metropolis = dependencies[0]
        if self.metropolis.rung_sigma is None:
            raise ValueError("TuneRungSigma: the Metropolis has no widths per rung to tune (Metropolis(..., rung_sigma=...))")
        self.target, self.gamma = float(target), float(gamma)
        self.sigma_min, self.sigma_max = float(sigma_min), float(sigma_max)
        if not 0.0 < self.target < 1.0:
            raise ValueError(f"TuneRungSigma: target = {target!r} must lie in (0, 1)")
        if not 0.0 < self.gamma <= 1.0:
            raise ValueError(f"TuneRungSigma: gamma = {gamma!r} must lie in (0, 1]")
        if int(min_calls) != min_calls or int(min_calls) < 1:
            raise ValueError(f"TuneRungSigma: min_calls = {min_calls!r} must be an integer >= 1")
        if not (1e-100 <= self.sigma_min <= self.sigma_max <= 1e100):
            raise ValueError(f"TuneRungSigma: sigma_min = {sigma_min!r}, sigma_max = {sigma_max!r} must satisfy "
                             "1e-100 <= sigma_min <= sigma_max <= 1e100")
        self.min_calls = int(min_calls)
        self.until = None if until is None else int(until)
        self.statuses = []         # (t, status array (K, R)) of every tuning asked for

    def initialise(self, simulation: Simulation) -> None:
        if self.metropolis.restored and self.metropolis._rung_window_used:
            return                 # (storage.restore brought the window back: the resumed run tunes as the uninterrupted one)
        self.metropolis.restart_rung_window()

    def make_step(self, simulation: Simulation) -> None:
        if self.until is not None and simulation.t > self.until:
            return
        status = self.metropolis.tune_rung_sigma(self.target, self.gamma, self.min_calls, self.sigma_min, self.sigma_max)
        self.statuses.append((simulation.t, status))

    def write_algorithm(self, io, scheduler) -> None:
        io.write("\tTuneRungSigma\n")
        io.write(f"\t\tCalls: {_calls(scheduler)}\n")
        io.write(f"\t\tTarget: {self.target}\n")
        io.write(f"\t\tGamma: {self.gamma}\n")
        io.write(f"\t\tMin calls: {self.min_calls}\n")
        io.write(f"\t\tSigma min: {self.sigma_min}\n")
        io.write(f"\t\tSigma max: {self.sigma_max}\n")
        io.write(f"\t\tUntil: {self.until}\n")


def _find_exchange(simulation: Simulation) -> ReplicaExchange:
    found = [a for a in simulation.algorithms if isinstance(a, ReplicaExchange)]
    if len(found) != 1:
        raise ValueError(f"this callback needs exactly one ReplicaExchange in the algorithm list, found {len(found)}")
    return found[0]


def callback_exchange_acceptance(simulation: Simulation) -> np.ndarray:
    """Per gap of the ladder, accepted / attempted swaps since the start: a vector of R - 1 ratios, NaN before the first attempt
    (callback_acceptance's convention, src/metropolis.jl:319-321).  Reads the gap counters: the host waits for the queued steps."""
    return _find_exchange(simulation).acceptance()


def callback_rung_acceptance(simulation: Simulation) -> np.ndarray:
    """accepted / total calls of every Metropolis move per rung over all shards, an array of shape (K, R), NaN where a move was
    never picked at a rung (Metropolis.rung_acceptance): the figure a width per rung (``Metropolis(..., rung_sigma=...)``) is tuned
    by.  Reads the per-chain counters: the host waits for the queued steps."""
    return _find_exchange(simulation).metropolis.rung_acceptance()


def callback_flow_fraction(simulation: Simulation) -> np.ndarray:
    """The flow fraction f(r) per rung, a vector of R values (ReplicaExchange.flow).  Needs ReplicaExchange(..., track=True)."""
    return _find_exchange(simulation).flow()


def callback_ladder(simulation: Simulation) -> np.ndarray:
    """beta per rung as the device holds it now, a vector of R values (ReplicaExchange.betas): with StoreCallbacks, the history of a
    ladder that RespaceLadder moves.  The host waits for the queued steps."""
    return _find_exchange(simulation).betas()


def callback_round_trips(simulation: Simulation) -> np.ndarray:
    """(round trips, up trips) over all ladders since the start, a vector of 2 values (ReplicaExchange.round_trips).  Needs
    ReplicaExchange(..., track=True)."""
    return _find_exchange(simulation).round_trips()


def callback_log_z(simulation: Simulation) -> np.ndarray:
    """log(Z_r / Z_0) per rung, a vector of R values (ReplicaExchange.log_z, the acceptance estimator) from the bridge sums accumulated
    so far; reading it does not reset the accumulator.  Needs ReplicaExchange(..., bridge=True)."""
    return _find_exchange(simulation).log_z()


def callback_log_z_error(simulation: Simulation) -> np.ndarray:
    """The jackknife standard error of callback_log_z's values (ReplicaExchange.log_z(error=True)[1]; needs blocks=B)."""
    return _find_exchange(simulation).log_z(error=True)[1]


def callback_heat_capacity_error(simulation: Simulation) -> np.ndarray:
    """The jackknife standard error of callback_heat_capacity's values (ReplicaExchange.heat_capacity(error=True)[1])."""
    return _find_exchange(simulation).heat_capacity(error=True)[1]


def callback_heat_capacity(simulation: Simulation) -> np.ndarray:
    """The heat capacity beta_r^2 (<e^2> - <e>^2) per rung, a vector of R values (ReplicaExchange.heat_capacity) from the bridge sums
    accumulated so far; reading it does not reset the accumulator.  Needs ReplicaExchange(..., bridge=True)."""
    return _find_exchange(simulation).heat_capacity()


def callback_rung_energy(simulation: Simulation) -> np.ndarray:
    """Mean energy per rung, a vector of R means over the ladders of all shards: reproducible sums formed on the device
    (ReplicaExchange.rung_sums), the same bits on any number of shards.  Any potential, Float64 or Float32 state."""
    return _find_exchange(simulation).rung_sums(AMC_REDUCE_E)[:, 0].copy()


def callback_rung_moments(simulation: Simulation) -> np.ndarray:
    """<x> and <x^2> per rung over the ladders of all shards, an array of shape (2, R): row 0 the means, row 1 the second moments
    (ReplicaExchange.rung_sums)."""
    return np.ascontiguousarray(_find_exchange(simulation).rung_sums(AMC_REDUCE_X | AMC_REDUCE_XX)[:, 1:].T)


def rung_energy(simulation: Simulation) -> np.ndarray:
    """Mean energy per rung, a vector of R means over the ladders of all shards.  A HOST pass: one strided download per rung
    (8 M bytes in all), potential(x) and a plain Float64 sum on the host -- not one of the engine's reproducible sums, so the last
    bits may depend on the split into shards.  Built-in potentials only.  (callback_rung_energy is the device-side, reproducible
    form.)"""
    rx = _find_exchange(simulation)
    met, R = rx.metropolis, rx.n_rungs
    start, stop = met.shard
    count = (stop - start) // R
    def energies(x):
        if getattr(met.chains, "dtype", "f64") != "f32":
            return _potential(met.chains.potential, x)
        x32 = x.astype(np.float32)                      # Particle{Float32}.e: potential(x) in Float32
        if met.chains.potential == "double_well":
            q = x32 * x32 - np.float32(1.0)
            return (q * q).astype(np.float64)
        _potential(met.chains.potential, x[:0])         # (raises for a CustomPotential)
        return (x32 * x32).astype(np.float64)
    sums = np.array([float(np.sum(energies(met.engine.download_strided(r, R, count)))) for r in range(R)])
    tot = sharding.allreduce_sum(np.concatenate([sums, [float(count)]]), met.engine)
    return tot[:R] / tot[R]


def callback_rung_sigma(simulation: Simulation) -> np.ndarray:
    """The widths per (move, rung) in force, shape (K, R) (``Metropolis.rung_sigma``, which follows every tuning): with StoreCallbacks,
    the history of a table that TuneRungSigma moves."""
    met = _find_exchange(simulation).metropolis
    if met.rung_sigma is None:
        raise ValueError("callback_rung_sigma: the Metropolis has no widths per rung (Metropolis(..., rung_sigma=...))")
    return np.array(met.rung_sigma, dtype=np.float64)


def callback_rung_window_acceptance(simulation: Simulation) -> np.ndarray:
    """accepted / total calls of every move per rung over the current window, shape (K, R) (Metropolis.rung_window_acceptance): the
    acceptance of the table in force, where callback_rung_acceptance mixes every table since the counters began."""
    return _find_exchange(simulation).metropolis.rung_window_acceptance()
