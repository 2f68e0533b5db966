"""``Convergence``: has the ensemble at a rung reached the stationary distribution?  The Gelman-Rubin potential scale reduction per
group, from running sums the device keeps per chain.

An extension over the reference, like ``Autocorrelation``.  Every other tool here -- the bridge sums, tau_int from one time origin, the
jackknife blocks, the energy histograms -- assumes the chains at a rung are stationary; this one checks it.  R-hat compares the
variance BETWEEN the chains' time means with the variance WITHIN the chains, for one observable.  The engine keeps two sums per chain
and half of the window -- S = sum o, Q = sum o^2 -- in one memory-bound pass per sample, and forms seven reproducible sums over the
chains of a group at fetch time (include/amc.h amc_chain_stats_accumulate / amc_chain_stats_fetch); the
formulas below are numpy Float64 on their rounded values.  The sums are the same bits on any grid and any split into shards.  With
a ladder "chain i" is the SLOT at rung r, whatever replicas pass through it: the series ``Autocorrelation`` uses.

Split R-hat (2N sequences of length n: both halves of every chain) also catches a drift within the window; the unsplit form (N
sequences of length 2n) is the classic one.  ``tau_int_batch`` is a batch-means ESTIMATE of the integrated autocorrelation time in
units of the sample spacing -- a check beside ``Autocorrelation.tau_int()``, not a second definition.
"""
from __future__ import annotations

import numpy as np

from . import sharding
from ._capi import (AMC_CHAIN_STATS_COLS, AMC_CHAIN_STATS_Q0, AMC_CHAIN_STATS_Q1, AMC_CHAIN_STATS_S0, AMC_CHAIN_STATS_S0S0,
                    AMC_CHAIN_STATS_S0S1, AMC_CHAIN_STATS_S1, AMC_CHAIN_STATS_S1S1, AMC_XSUM_WORDS, CORR_OBSERVABLES, xsum_round)
from .metropolis import Metropolis
from .simulation import AriannaAlgorithm, Simulation, _calls


def _equal_counts(n) -> int:
    """n of both halves; a ValueError naming the two counts unless n[0] = n[1] >= 2."""
    n0, n1 = (int(n), int(n)) if np.ndim(n) == 0 else (int(n[0]), int(n[1]))
    if n0 != n1 or n0 < 2:
        raise ValueError(f"R-hat needs the same number of samples, two at least, in both halves of the window: part 0 holds {n0}, part 1 holds {n1}")
    return n0


def variances_from_records(records, n, N, split: bool = True):
    """(W[G], Bn[G], var_plus[G]) from records[G][7][AMC_XSUM_WORDS] (columns S0, S0S0, Q0, S1, S1S1, Q1, S0S1) of sums over ``N``
    chains per group and ``n`` = (n0, n1) samples per half.  With m sequences of length L -- split: m = 2N, L = n, the halves;
    otherwise m = N, L = 2n, the whole chains --
        W = (sum Q - (sum S^2) / L) / (m (L - 1))                       the mean within-sequence variance
        Bn = ((sum S^2) / L^2 - (sum S / L)^2 / m) / (m - 1)            the variance of the sequence means (B / L)
        var_plus = (L - 1) / L W + Bn."""
    n = _equal_counts(n)
    rec = np.asarray(records, dtype=np.float64)
    v = xsum_round(rec.reshape(-1, AMC_XSUM_WORDS)).reshape(rec.shape[:-1])
    assert v.ndim == 2 and v.shape[1] == AMC_CHAIN_STATS_COLS, v.shape
    sum_s = v[:, AMC_CHAIN_STATS_S0] + v[:, AMC_CHAIN_STATS_S1]
    sum_q = v[:, AMC_CHAIN_STATS_Q0] + v[:, AMC_CHAIN_STATS_Q1]
    sum_ss = v[:, AMC_CHAIN_STATS_S0S0] + v[:, AMC_CHAIN_STATS_S1S1]
    m, length = 2.0 * float(N), float(n)
    if not split:
        sum_ss = v[:, AMC_CHAIN_STATS_S0S0] + 2.0 * v[:, AMC_CHAIN_STATS_S0S1] + v[:, AMC_CHAIN_STATS_S1S1]
        m, length = float(N), 2.0 * float(n)
    with np.errstate(all="ignore"):
        w = (sum_q - sum_ss / length) / (m * (length - 1.0))
        a = sum_s / length
        a2 = sum_ss / (length * length)
        bn = (a2 - a * a / m) / (m - 1.0)
        var_plus = (length - 1.0) / length * w + bn
    return w, bn, var_plus


def rhat_from_records(records, n, N, split: bool = True) -> np.ndarray:
    """R-hat[G] = sqrt(var_plus / W) (variances_from_records)."""
    w, _, var_plus = variances_from_records(records, n, N, split)
    with np.errstate(all="ignore"):
        return np.sqrt(var_plus / w)


def tau_batch_from_records(records, n, N) -> np.ndarray:
    """tau[G] = n Bn / (2 var_plus) from the split form, in units of the sample spacing: the variance of a batch mean of n samples
    is about 2 tau var / n.  An estimate (biased low while n is not >> tau), 1/2 for independent samples."""
    n_each = _equal_counts(n)
    _, bn, var_plus = variances_from_records(records, n, N, True)
    with np.errstate(all="ignore"):
        return n_each * bn / (2.0 * var_plus)


class Convergence(AriannaAlgorithm):
    """Convergence(chains; dependencies=(Metropolis,), scheduler=..., observable="energy" | "x", n_samples=2n): the first n scheduled
    calls add the observable of every chain to part 0 of its running sums, the next n to part 1; later calls launch nothing.  It
    observes only.  ``rhat()``, ``variances()``, ``tau_int_batch()`` and ``counts()`` read the result, one value per group (rung; one
    group without a ladder); ``restart()`` clears the sums and begins a new window with the next scheduled call."""

    def __init__(self, chains, dependencies=None, observable="energy", n_samples=None, path=None, **extras):
        assert dependencies is not None and len(dependencies) == 1 and isinstance(dependencies[0], Metropolis)
        self.metropolis: Metropolis = dependencies[0]
        if observable not in CORR_OBSERVABLES:
            raise ValueError(f"Convergence: observable = {observable!r} must be one of {sorted(CORR_OBSERVABLES)}")
        if n_samples is None or int(n_samples) != n_samples or int(n_samples) < 4 or int(n_samples) % 2:
            raise ValueError(f"Convergence: n_samples = {n_samples!r} must be an even integer >= 4 (two halves of two samples at least)")
        if not hasattr(self.metropolis.engine, "chain_stats_accumulate"):
            raise ValueError("Convergence: this engine keeps no sums per chain (streams > 1 is not supported)")
        self.observable, self.n_samples = observable, int(n_samples)
        self.chains = chains
        self.phase = 0                          # samples taken of the window at hand
        self.metropolis.convergence = self      # (storage.checkpoint: the sums per chain and the phase are state)

    # -- scheduling -----------------------------------------------------------------------------------------------------------------
    def initialise(self, simulation: Simulation) -> None:
        """Every sample of a window belongs to ONE beta and ONE table of widths per group: an annealing step, a respacing or a tuning
        between the first and the last sample is refused here, from the schedules, before anything runs."""
        from .annealing import PopulationAnnealing
        from .exchange import RespaceLadder, TuneRungSigma
        algs = list(simulation.algorithms)
        me = algs.index(self)
        mine = [(t, me) for t in simulation.schedulers[me] if t > 0][:self.n_samples - self.phase]
        if not mine:
            return
        first = mine[0] if self.phase == 0 else None      # (a restored window: no time of this run, everything lies behind its first sample)
        last = mine[-1]
        for kind, what in ((PopulationAnnealing, "annealing step"), (RespaceLadder, "respacing"), (TuneRungSigma, "tuning of the widths")):
            inside = sorted((t, j) for j, a in enumerate(algs) if isinstance(a, kind) for t in simulation.schedulers[j]
                            if t > 0 and (first is None or first < (t, j)) and (t, j) < last)
            if inside:
                raise ValueError(f"Convergence: the {what} at t = {inside[0][0]} falls between the first sample at t = "
                                 f"{'(restored)' if first is None else first[0]} and the last sample at t = {last[0]}; the sums per chain "
                                 "belong to one stationary distribution per group, clear them (restart()) when it moves")

    def make_step(self, simulation: Simulation) -> None:
        if self.phase >= self.n_samples:        # the window is full: further scheduled calls launch nothing
            return
        self.metropolis.engine.chain_stats_accumulate(self.observable, 0 if 2 * self.phase < self.n_samples else 1)
        self.phase += 1

    def restart(self) -> None:
        """Clear the sums per chain; the next scheduled call is the first sample of a new window."""
        self.metropolis.engine.chain_stats_clear()
        self.phase = 0

    # -- results --------------------------------------------------------------------------------------------------------------------
    def _groups(self) -> int:
        return max(int(self.metropolis.n_rungs), 1)

    def counts(self):
        """(n0, n1): the samples each half of the window holds.  Host state: nothing is queued, nothing waits."""
        return self.metropolis.engine.chain_stats_counts()[0]

    def _fetch(self, equal: bool = True):
        """(records of ALL ranks, (n0, n1)) from ONE fetch of the engine (the sums by group, the copy, the wait).  ``equal``: the
        halves must hold the same number of samples, two at least -- checked on the host's counts before anything is queued."""
        n, obs = self.metropolis.engine.chain_stats_counts()
        if not obs:
            raise ValueError("Convergence: nothing has been accumulated yet")
        if equal:
            _equal_counts(n)
        rec, n, obs = self.metropolis.engine.chain_stats_fetch()
        return sharding.allreduce_xsum(rec, self.metropolis.engine if self.metropolis.world_size > 1 else None).reshape(rec.shape), n

    def records(self) -> np.ndarray:
        """records[G][7][AMC_XSUM_WORDS] of ALL ranks (merged as ``Autocorrelation.records`` merges: every rank ends with the same
        bits, those one rank holding all the chains would have).  The host waits for the queued samples."""
        return self._fetch(equal=False)[0]

    def n_per_group(self) -> int:
        return len(self.chains) // self._groups()

    def variances(self, split: bool = True):
        """(W[G], Bn[G], var_plus[G]) (variances_from_records)."""
        rec, n = self._fetch()
        return variances_from_records(rec, n, self.n_per_group(), split)

    def rhat(self, split: bool = True) -> np.ndarray:
        """R-hat per group; ValueError while the halves do not hold the same number of samples (two at least)."""
        rec, n = self._fetch()
        return rhat_from_records(rec, n, self.n_per_group(), split)

    def tau_int_batch(self) -> np.ndarray:
        """The batch-means estimate of tau_int per group, in units of the sample spacing (tau_batch_from_records)."""
        rec, n = self._fetch()
        return tau_batch_from_records(rec, n, self.n_per_group())

    # -- checkpoints (storage.py's section) -------------------------------------------------------------------------------------------
    def state(self) -> dict:
        eng = self.metropolis.engine
        n, obs = eng.chain_stats_counts()
        d = dict(conv_observable=np.int64(CORR_OBSERVABLES[self.observable]), conv_phase=np.int64(self.phase),
                 conv_n=np.array(n, dtype=np.uint64))
        if obs:
            d["conv_sums"] = eng.chain_stats_sums()
        return d

    def set_state(self, d) -> None:
        if int(d["conv_observable"]) != CORR_OBSERVABLES[self.observable]:
            raise ValueError(f"checkpoint holds sums per chain of observable {int(d['conv_observable'])}, this Convergence asks for "
                             f"{self.observable!r}")
        self.phase = int(d["conv_phase"])
        if "conv_sums" in d:
            self.metropolis.engine.set_chain_stats(self.observable, d["conv_n"], d["conv_sums"])

    def write_algorithm(self, io, scheduler) -> None:
        io.write(f"\tConvergence\n\t\tCalls: {_calls(scheduler)}\n\t\tObservable: {self.observable}\n\t\tSamples: {self.n_samples}\n")


def _find_convergence(simulation: Simulation) -> Convergence:
    found = [a for a in simulation.algorithms if isinstance(a, Convergence)]
    if len(found) != 1:
        raise ValueError(f"this callback needs exactly one Convergence in the algorithm list, found {len(found)}")
    return found[0]


def callback_rhat(simulation: Simulation) -> np.ndarray:
    """The split R-hat per group (Convergence.rhat()): one fetch, for which the host waits.  Due while the halves are unequal it
    stores NaN and queues nothing."""
    conv = _find_convergence(simulation)
    n = conv.counts()
    if n[0] != n[1] or n[0] < 2:
        return np.full(conv._groups(), np.nan)
    return conv.rhat()
