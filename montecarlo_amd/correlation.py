"""``Autocorrelation``: how fast an observable of the chains decorrelates, measured on the device.

An extension over the reference, like ``ReplicaExchange`` and ``PopulationAnnealing``.  A many-chain engine suits the cheapest
estimator there is: ONE time origin and the M chains as independent series,
    C(k) = <O_i(t0) O_i(t0 + k)>_i - <O_i(t0)>_i <O_i(t0 + k)>_i.
The engine keeps one word per chain -- the observable at the origin -- and forms the three sums a lag needs in one memory-bound
pass (include/amc.h amc_corr_mark / amc_corr_sample); this algorithm schedules the passes like any other.
The sums are reproducible: the same bits on any grid and any split into shards.  With a ladder there is one series per RUNG (group
r = the chains l R + r, whatever replicas pass through them): tau_int at the cold rung is the number a ladder is meant to shorten.

The first scheduled call marks the origin, the next ``n_lags`` calls sample.  With ``origins`` > 1 the call after that fetches the
records, merges them into a host accumulator slot by slot and marks again: the sums of the origins add, which averages C(k) over
them.  Nothing synchronises between a mark and its last sample.
"""
from __future__ import annotations

import numpy as np

from . import jackknife, sharding
from ._capi import AMC_CORR_AO, AMC_CORR_MAX_LAGS, AMC_CORR_O, AMC_CORR_OO, AMC_XSUM_WORDS, CORR_OBSERVABLES, xsum_merge, xsum_round
from .metropolis import Metropolis
from .simulation import AriannaAlgorithm, Simulation, _calls


def rho_from_records(records, n: float) -> np.ndarray:
    """rho[G][S] from records[S][G][3][AMC_XSUM_WORDS] of sums over ``n`` chains per group (per origin merged in: n counts them all).
    From the rounded means: rho_g(k) = (<a O_k> - <a><O_k>) / sqrt((<a^2> - <a>^2)(<O_k^2> - <O_k>^2)); <a>, <a^2> are slot 0's."""
    rec = np.asarray(records, dtype=np.float64)
    return rho_from_means(xsum_round(rec.reshape(-1, AMC_XSUM_WORDS)).reshape(rec.shape[:-1]) / float(n))


def rho_from_means(m) -> np.ndarray:
    """rho[G][S] from the means m[S][G][3] of O, OO, AO (rho_from_records)."""
    mo, moo, mao = m[:, :, AMC_CORR_O], m[:, :, AMC_CORR_OO], m[:, :, AMC_CORR_AO]
    with np.errstate(all="ignore"):
        cov = mao - mo[0] * mo
        var_a = moo[0] - mo[0] * mo[0]
        var_o = moo - mo * mo
        return (cov / np.sqrt(var_a * var_o)).T


def tau_from_rho(rho, spacing: float = 1.0, c: float = 5.0):
    """(tau[G], window[G], converged[G]) from rho[G][n_lags + 1] at equally spaced lags: tau = spacing (1/2 + sum_{k=1..W} rho(k)), W
    the first k with k >= c (1/2 + sum_{j<=k} rho(j)) (Sokal's automatic window); without such a k, W = n_lags and converged is
    False."""
    rho = np.atleast_2d(np.asarray(rho, dtype=np.float64))
    G, n_lags = rho.shape[0], rho.shape[1] - 1
    tau, window, converged = np.zeros(G), np.zeros(G, dtype=np.int64), np.zeros(G, dtype=bool)
    for g in range(G):
        acc, w, ok = 0.5, n_lags, False
        for k in range(1, n_lags + 1):
            acc += rho[g, k]
            if k >= c * acc:
                w, ok = k, True
                break
        tau[g], window[g], converged[g] = spacing * acc, w, ok
    return tau, window, converged


class Autocorrelation(AriannaAlgorithm):
    """Autocorrelation(chains; dependencies=(Metropolis,), scheduler=..., observable="energy" | "x", n_lags=..., origins=1): at its
    scheduled times [mark; n_lags samples] per origin, on the Metropolis' engine.  It observes only: listed behind its Metropolis, a
    time step at which both are due is [sweep; mark or sample].  ``rho()`` and ``tau_int()`` read the result.

    ``blocks=B`` (2..64) keeps the sums per block of ladders (of chains, without a ladder), block of ladder l = (l div block_chunk)
    mod B (``block_chunk`` None: max(1, 256 div G) ladders), and ``rho(error=True)`` /
    ``tau_int(c, error=True)`` add the standard error of the delete-one-block jackknife: every replicate runs the whole estimator,
    its own automatic window included."""

    def __init__(self, chains, dependencies=None, observable="energy", n_lags=None, origins=1, blocks=None, block_chunk=None, path=None,
                 **extras):
        assert dependencies is not None and len(dependencies) == 1 and isinstance(dependencies[0], Metropolis)
        self.metropolis: Metropolis = dependencies[0]
        if observable not in CORR_OBSERVABLES:
            raise ValueError(f"Autocorrelation: observable = {observable!r} must be one of {sorted(CORR_OBSERVABLES)}")
        if n_lags is None or int(n_lags) != n_lags or not 1 <= int(n_lags) < AMC_CORR_MAX_LAGS:
            raise ValueError(f"Autocorrelation: n_lags = {n_lags!r} must be an integer in [1, {AMC_CORR_MAX_LAGS - 1}] (slot 0 is the mark's)")
        if int(origins) != origins or int(origins) < 1:
            raise ValueError(f"Autocorrelation: origins = {origins!r} must be an integer >= 1")
        if not hasattr(self.metropolis.engine, "corr_mark"):
            raise ValueError("Autocorrelation: this engine has no time correlation (streams > 1 is not supported)")
        self.observable, self.n_lags, self.origins = observable, int(n_lags), int(origins)
        self.chains = chains
        self.phase = -1                        # samples taken of the origin at hand (0: marked); -1: nothing is marked
        self.origins_done = 0                  # origins merged into the accumulator
        self._acc = None                       # [n_lags + 1][G][3][AMC_XSUM_WORDS]: the merged records of those origins (this shard's)
        self._steps = None                     # their lag steps (differences from the mark): every origin's pattern
        self.metropolis.autocorrelation = self     # (storage.checkpoint: the mark, its samples and the accumulator are state)
        groups = int(getattr(chains, "n_rungs", None) or 1)
        if blocks is not None and block_chunk is None and self.metropolis.blocks and self.metropolis.blocks[0] == int(blocks):
            block_chunk = self.metropolis.blocks[1]      # (the ReplicaExchange of these chains set the chunk: one partition per engine)
        self._blocks_asked = jackknife.check_blocks("Autocorrelation", blocks, block_chunk, len(chains) // groups, groups)
        if self._blocks_asked:
            jackknife.ask_blocks("Autocorrelation", self.metropolis, self._blocks_asked)
        self._acc_blocks = None                # [B][n_lags + 1][G][3][AMC_XSUM_WORDS]: the same per jackknife block

    @property
    def blocks(self):
        """The partition (B, C) the sums are kept under, None without one: this algorithm's own, or the one the ReplicaExchange of the
        same Metropolis asked for -- the engine has one partition, and every mark of it goes into the blocked accumulator."""
        return self._blocks_asked or self.metropolis.blocks

    # -- scheduling -----------------------------------------------------------------------------------------------------------------
    def initialise(self, simulation: Simulation) -> None:
        """An annealing step between a mark and one of its samples would resample the chains under the origin: refused here, from the
        schedules, before anything runs."""
        from .annealing import PopulationAnnealing
        if self.blocks:
            jackknife.refuse_annealing("Autocorrelation", simulation)
        from .exchange import ReplicaExchange
        if self._blocks_asked and any(isinstance(a, ReplicaExchange) and a.bridge and not a.blocks for a in simulation.algorithms):
            raise ValueError("Autocorrelation: blocks beside a ReplicaExchange(bridge=...) without blocks: setting the partition at the first "
                             "mark would clear the bridge sums accumulated so far; give the ReplicaExchange the same blocks")
        algs = list(simulation.algorithms)
        me = algs.index(self)
        mine = [(t, me) for t in simulation.schedulers[me] if t > 0]
        anneals = sorted((t, j) for j, a in enumerate(algs) if isinstance(a, PopulationAnnealing) for t in simulation.schedulers[j] if t > 0)
        phase, done, mark = self.phase, self.origins_done, None      # (a restored mark: no time of this run, everything lies behind it)
        for call in mine:
            if done >= self.origins:
                break
            if phase < 0:
                phase, mark = 0, call
            elif phase < self.n_lags:
                phase += 1
                between = [a for a in anneals if (mark is None or mark < a) and a < call]
                if between:
                    raise ValueError(f"Autocorrelation: the annealing step at t = {between[0][0]} falls between the mark at t = "
                                     f"{'(restored)' if mark is None else mark[0]} and the sample at t = {call[0]}; resampling moves the chains "
                                     "between slots, a product across it has no meaning")
            elif done + 1 < self.origins:
                done, phase, mark = done + 1, 0, call
            else:
                break

    def make_step(self, simulation: Simulation) -> None:
        eng = self.metropolis.engine
        if self.origins_done >= self.origins:      # every origin is taken and merged: further scheduled calls launch nothing
            return
        if self.phase < 0:
            self._mark()
        elif self.phase < self.n_lags:
            eng.corr_sample()
            self.phase += 1
        elif self.origins_done + 1 < self.origins:
            self._fold()
            self._mark()
        # else: the last origin is complete; further scheduled calls launch nothing

    def _mark(self) -> None:
        if self.blocks:                         # (here and not in initialise: every algorithm's set_ladder lies behind us by now)
            jackknife.use_blocks(self.metropolis, self.blocks)
        self.metropolis.engine.corr_mark(self.observable)
        self.phase = 0

    def _fold(self) -> None:
        """The complete origin at hand merged into the accumulator (the host waits for its samples)."""
        rec, steps, _ = self.metropolis.engine.corr_fetch()
        lags = (steps - steps[0]).astype(np.int64)
        if self._acc is None:
            self._acc, self._steps = rec.copy(), lags
        else:
            if not np.array_equal(lags, self._steps):
                raise ValueError(f"Autocorrelation: origin {self.origins_done + 1} has lag steps {lags.tolist()}, the first origin had "
                                 f"{self._steps.tolist()}: origins add slot by slot, so every one needs the same pattern")
            self._acc = xsum_merge(self._acc.reshape(-1, AMC_XSUM_WORDS), rec.reshape(-1, AMC_XSUM_WORDS)).reshape(rec.shape)
        if self.blocks:                         # the same origin per block; a block without a local ladder stays all zero
            blk = self.metropolis.engine.corr_fetch_blocks()[0]
            self._acc_blocks = blk if self._acc_blocks is None else np.stack([jackknife._merge(a.reshape(-1, AMC_XSUM_WORDS), b.reshape(-1, AMC_XSUM_WORDS))
                                                                             .reshape(b.shape) for a, b in zip(self._acc_blocks, blk)])
        self.origins_done += 1
        self.phase = -1

    # -- results --------------------------------------------------------------------------------------------------------------------
    def _local(self):
        """(records, lag steps, origins in them) of this shard: the accumulator, with the origin at hand merged in once it is complete;
        before the first origin is complete, what it has so far."""
        if self.phase == self.n_lags:
            self._fold()
            self.metropolis.engine.corr_clear()
        if self._acc is not None:
            return self._acc, self._steps, self.origins_done
        if self.phase < 0:
            raise ValueError("Autocorrelation: nothing has been marked yet")
        rec, steps, _ = self.metropolis.engine.corr_fetch()
        return rec, (steps - steps[0]).astype(np.int64), 1

    def lags(self) -> np.ndarray:
        """Step differences from the mark, one per slot (slot 0: 0)."""
        return self._local()[1].copy()

    def records(self) -> np.ndarray:
        """records[S][G][3][AMC_XSUM_WORDS], columns O, OO, AO, of ALL ranks and the origins so far (merged as reduce_rungs' are: every
        rank ends with the same bits, those one rank holding all the chains would have)."""
        rec = self._local()[0]
        return sharding.allreduce_xsum(rec, self.metropolis.engine if self.metropolis.world_size > 1 else None)

    def n_per_group(self) -> float:
        """Summands of every record: the chains of a group times the origins merged."""
        return float(len(self.chains) // max(self.metropolis.n_rungs, 1) * self._local()[2])

    def block_records(self):
        """(records[B][S][G][3][AMC_XSUM_WORDS], ladders[B]) of ALL ranks and the origins so far, per jackknife block -- the ranks'
        records merged block by block -- and the ladders (chains, without a ladder) of every block.  Needs ``blocks``."""
        if not self.blocks:
            raise ValueError("Autocorrelation: error=True needs the sums per block: build the Autocorrelation with blocks=B")
        self._local()                           # (folds a complete origin)
        rec = self._acc_blocks if self._acc_blocks is not None else self.metropolis.engine.corr_fetch_blocks()[0]
        rec = sharding.allreduce_xsum(rec, self.metropolis.engine if self.metropolis.world_size > 1 else None).reshape(rec.shape)
        return rec, jackknife.block_counts(len(self.chains) // max(self.metropolis.n_rungs, 1), *self.blocks)

    def _jackknife(self, fn):
        rec, ladders = self.block_records()
        origins = self._local()[2]
        return jackknife.jackknife(rec, ladders, lambda values, n: fn(rho_from_means(values / float(n * origins))))

    def rho(self, error: bool = False):
        """rho[G][S]: the normalised autocorrelation of every group at every slot (rho_from_records).  ``error=True``: (rho, se), se
        from the delete-one-block jackknife (needs ``blocks``)."""
        if error:
            return self._jackknife(lambda rho: rho)
        return rho_from_records(self.records(), self.n_per_group())

    def tau_int(self, c: float = 5.0, error: bool = False):
        """(tau[G], window[G], converged[G]) in MH steps (tau_from_rho).  The lag steps must be equally spaced.  ``error=True``:
        (tau, se, window, converged); every leave-one-out replicate runs the whole estimator, its own automatic window included."""
        lags = self.lags()
        d = np.diff(lags)
        if d.size == 0 or d[0] <= 0 or np.any(d != d[0]):
            raise ValueError(f"Autocorrelation.tau_int: the lag steps {lags.tolist()} are not equally spaced")
        tau, window, converged = tau_from_rho(self.rho(), float(d[0]), c)
        if not error:
            return tau, window, converged
        return tau, self._jackknife(lambda rho: tau_from_rho(rho, float(d[0]), c)[0])[1], window, converged

    # -- checkpoints (storage.py's section) -------------------------------------------------------------------------------------------
    def state(self) -> dict:
        eng = self.metropolis.engine
        d = dict(corr_observable=np.int64(CORR_OBSERVABLES[self.observable]), corr_phase=np.int64(self.phase),
                 corr_origins_done=np.int64(self.origins_done))
        if self.phase >= 0:
            rec, steps, _ = eng.corr_fetch()
            d.update(corr_origin=eng.corr_origin(), corr_records=rec, corr_steps=steps)
        if self._acc is not None:
            d.update(corr_acc=self._acc, corr_acc_steps=self._steps)
        return d

    def state_blocks(self) -> dict:
        """The section of a run with ``blocks``: the partition, the mark's records per block, the accumulator per block."""
        if not self.blocks:
            return {}
        d = dict(corr_blocks=np.array(self.blocks, dtype=np.int64))
        if self.phase >= 0:
            d["corr_block_records"] = self.metropolis.engine.corr_fetch_blocks()[0]
        if self._acc_blocks is not None:
            d["corr_acc_blocks"] = self._acc_blocks
        return d

    def set_state_blocks(self, d) -> None:
        if not self.blocks:
            return                              # (a run without blocks reads a blocked checkpoint's merged records: set_state did)
        if "corr_blocks" not in d:
            if "corr_observable" in d and (int(d["corr_phase"]) >= 0 or "corr_acc" in d):
                raise ValueError("checkpoint holds a time correlation without sums per block, this Autocorrelation asks for blocks")
            return
        if tuple(int(v) for v in d["corr_blocks"]) != self.blocks:
            raise ValueError(f"checkpoint holds a time correlation under the partition {tuple(int(v) for v in d['corr_blocks'])}, this "
                             f"Autocorrelation asks for {self.blocks}")
        if "corr_block_records" in d:           # (set_state left the mark to us: merged records cannot fill the blocks)
            jackknife.use_blocks(self.metropolis, self.blocks)
            self.metropolis.engine.set_corr_blocks(self.observable, d["corr_origin"], d["corr_block_records"], d["corr_steps"])
        if "corr_acc_blocks" in d:
            self._acc_blocks = np.array(d["corr_acc_blocks"], dtype=np.float64)

    def set_state(self, d) -> None:
        if int(d["corr_observable"]) != CORR_OBSERVABLES[self.observable]:
            raise ValueError(f"checkpoint holds a time correlation of observable {int(d['corr_observable'])}, this Autocorrelation asks for "
                             f"{self.observable!r}")
        self.phase, self.origins_done = int(d["corr_phase"]), int(d["corr_origins_done"])
        if self.phase >= 0 and not self.blocks:     # (with blocks: set_state_blocks restores the mark per block)
            self.metropolis.engine.set_corr(self.observable, d["corr_origin"], d["corr_records"], d["corr_steps"])
        if "corr_acc" in d:
            self._acc, self._steps = np.array(d["corr_acc"], dtype=np.float64), np.array(d["corr_acc_steps"], dtype=np.int64)

    def write_algorithm(self, io, scheduler) -> None:
        io.write(f"\tAutocorrelation\n\t\tCalls: {_calls(scheduler)}\n\t\tObservable: {self.observable}\n\t\tLags: {self.n_lags}\n"
                 f"\t\tOrigins: {self.origins}\n")


def _find_autocorrelation(simulation: Simulation) -> Autocorrelation:
    found = [a for a in simulation.algorithms if isinstance(a, Autocorrelation)]
    if len(found) != 1:
        raise ValueError(f"this callback needs exactly one Autocorrelation in the algorithm list, found {len(found)}")
    return found[0]


def callback_tau_int(simulation: Simulation) -> np.ndarray:
    """tau_int per group in MH steps (Autocorrelation.tau_int()[0]).  The host waits for the queued samples."""
    return _find_autocorrelation(simulation).tau_int()[0]


def callback_tau_int_error(simulation: Simulation) -> np.ndarray:
    """The jackknife standard error of callback_tau_int's values (Autocorrelation.tau_int(error=True)[1]; needs blocks=B)."""
    return _find_autocorrelation(simulation).tau_int(error=True)[1]


def callback_rho(simulation: Simulation) -> np.ndarray:
    """rho per group at the last slot taken (Autocorrelation.rho()[:, -1])."""
    return _find_autocorrelation(simulation).rho()[:, -1]
