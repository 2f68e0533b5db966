"""``PopulationAnnealing``: cool the whole ensemble step by step and resample it on the device.

An extension over the reference, like ``ReplicaExchange``: there a user would write an ``AriannaAlgorithm`` whose ``make_step!`` walks
``simulation.chains``; here the chains live in HBM behind the C ABI, so the engine provides the resampling step (DESIGN.md section
3.14, include/amc.h amc_anneal) and this algorithm schedules it like any other.

Population annealing runs ONE large population at one shared beta.  At each scheduled time the population is moved to the next beta of
a list: every chain is weighted by exp(-(beta' - beta) e), the chains are resampled in proportion to the weights (systematic
resampling, exact integers on the device), and the Metropolis sweeps that follow equilibrate the copies -- the Philox draws are keyed
by chain slot and step, so copies of one parent part ways at their first sweep.  The mean weight of a step estimates
Z(beta') / Z(beta): one run yields log Z along the whole schedule.  ``families=True`` carries the id of every chain's ancestor along;
rho_t = sum_f n_f^2 / M, the mean family size seen from a chain, tells whether the population is large enough (rho_t << M).
"""
from __future__ import annotations

import math
import struct

import numpy as np

from . import sharding
from ._capi import AMC_ANNEAL_MAX_RECORDS, AMC_ANNEAL_RECORD_WORDS, AMC_ANNEAL_WEIGHT_BITS
from .metropolis import Metropolis
from .simulation import AriannaAlgorithm, Simulation, _calls


def _f64(bits) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(bits)))[0]


class PopulationAnnealing(AriannaAlgorithm):
    """PopulationAnnealing(chains; dependencies=(Metropolis,), betas=[...], families=False): one annealing step of the Metropolis'
    engine per scheduled time, to the next beta of ``betas``.  Listed behind its Metropolis, a time step at which both are due is
    [sweep; anneal].  It is an error when the list runs out."""

    mutates_chains = True          # a callback due behind it at the same t observes the state AFTER the resampling

    def __init__(self, chains, dependencies=None, betas=None, families=False, path=None, **extras):
        assert dependencies is not None and len(dependencies) == 1 and isinstance(dependencies[0], Metropolis)
        self.metropolis: Metropolis = dependencies[0]
        if betas is None or len(betas) == 0:
            raise ValueError("PopulationAnnealing: betas is missing (the list of beta values to anneal to, one per scheduled call)")
        self.betas = [float(b) for b in betas]
        for i, b in enumerate(self.betas):
            if not math.isfinite(b):
                raise ValueError(f"PopulationAnnealing: betas[{i}] = {b!r} is not finite")
        if chains.beta_array is not None:
            raise ValueError("PopulationAnnealing: the chains carry a per-chain beta array (ParticleChains.ladder); population annealing "
                             "cools one shared beta")
        if self.metropolis.world_size != 1:
            raise ValueError(f"PopulationAnnealing: {self.metropolis.world_size} ranks; resampling needs the whole ensemble on one "
                             "device (populations that span GPUs are not supported)")
        if not hasattr(self.metropolis.engine, "anneal"):
            raise ValueError("PopulationAnnealing: this engine has no annealing step (streams > 1 is not supported)")
        self.families = bool(families)
        self.chains = chains
        self._records = []                     # records drained from the engine's log, oldest first
        self.metropolis.annealing = self       # (storage.checkpoint: beta, the step index, the records and the families are state)
        self.rank, _ = sharding.world()

    def initialise(self, simulation: Simulation) -> None:
        from .exchange import ReplicaExchange
        if any(isinstance(a, ReplicaExchange) for a in simulation.algorithms):
            raise ValueError("PopulationAnnealing: the algorithm list holds a ReplicaExchange; a ladder and an annealed population "
                             "exclude each other")
        if self.families and not self.metropolis.families_restored:     # (restored: storage.restore brought them back)
            self.metropolis.engine.set_anneal_families(True)

    def make_step(self, simulation: Simulation) -> None:
        eng = self.metropolis.engine
        i = eng.anneal_step
        if i >= len(self.betas):
            raise ValueError(f"PopulationAnnealing: annealing step {i + 1} is due and betas holds {len(self.betas)} values")
        if i - len(self._records) >= AMC_ANNEAL_MAX_RECORDS:
            self._drain()
        eng.anneal(self.betas[i])
        self.chains.beta = self.betas[i]
        self.metropolis.invalidate_reductions()

    def _drain(self) -> None:
        rec = np.asarray(self.metropolis.engine.anneal_records(reset=True), dtype=np.uint64).reshape(-1, AMC_ANNEAL_RECORD_WORDS)
        self._records.extend(rec.copy())

    @property
    def beta(self) -> float:
        """The shared beta in force."""
        return float(self.metropolis.engine.beta)

    def records(self) -> np.ndarray:
        """One row of 8 unsigned 64-bit words per annealing step so far: status, bits of beta before, bits of beta after, bits of
        a_max, T_w, U, n_parents, max_children.  The host waits for the queued steps."""
        self._drain()
        return np.array(self._records, dtype=np.uint64).reshape(-1, AMC_ANNEAL_RECORD_WORDS)

    def log_z_ratios(self) -> np.ndarray:
        """log(Z(beta_to) / Z(beta_from)) per annealing step: a_max + log T_w - log M - 30 log 2, the log of the mean reweighting
        factor, formed from the integer records (the same number on any grid); NaN for a step that did not resample."""
        M = float(len(self.chains))
        out = [(_f64(r[3]) + math.log(int(r[4])) - math.log(M) - AMC_ANNEAL_WEIGHT_BITS * math.log(2.0)) if int(r[0]) == 0 else math.nan
               for r in self.records()]
        return np.array(out, dtype=np.float64)

    def log_z(self) -> np.ndarray:
        """log(Z(beta_i) / Z(beta_start)) after every annealing step: the cumulative sum of log_z_ratios() from the first beta."""
        return np.cumsum(self.log_z_ratios())

    def betas_done(self) -> np.ndarray:
        """beta after every annealing step so far (the records' own)."""
        return np.array([_f64(r[2]) for r in self.records()], dtype=np.float64)

    def survival(self) -> np.ndarray:
        """n_parents / M per annealing step: the share of the population that left at least one child."""
        return self.records()[:, 6].astype(np.float64) / float(len(self.chains))

    def family_stats(self):
        """(families with a member, sum of n_f^2, largest n_f): exact integers.  Needs families=True."""
        if not self.families:
            raise ValueError("PopulationAnnealing.family_stats needs the families: build the PopulationAnnealing with families=True")
        return self.metropolis.engine.anneal_family_stats()

    def rho_t(self) -> float:
        """sum_f n_f^2 / M: the mean size of the family a chain belongs to (1 before the first step, M when one family is left)."""
        return self.family_stats()[1] / float(len(self.chains))

    def write_algorithm(self, io, scheduler) -> None:
        io.write(f"\tPopulationAnnealing\n\t\tCalls: {_calls(scheduler)}\n\t\tBetas: {len(self.betas)} from {self.betas[0]} to {self.betas[-1]}\n"
                 f"\t\tFamilies: {str(self.families).lower()}\n")


def _find_annealing(simulation: Simulation) -> PopulationAnnealing:
    found = [a for a in simulation.algorithms if isinstance(a, PopulationAnnealing)]
    if len(found) != 1:
        raise ValueError(f"this callback needs exactly one PopulationAnnealing in the algorithm list, found {len(found)}")
    return found[0]


def callback_anneal_beta(simulation: Simulation) -> float:
    """The shared beta in force (PopulationAnnealing.beta)."""
    return _find_annealing(simulation).beta


def callback_anneal_log_z(simulation: Simulation) -> float:
    """log(Z(beta) / Z(beta_start)) at the beta in force (the last entry of PopulationAnnealing.log_z; 0 before the first step).  The
    host waits for the queued steps."""
    lz = _find_annealing(simulation).log_z()
    return float(lz[-1]) if lz.size else 0.0


def callback_rho_t(simulation: Simulation) -> float:
    """rho_t = sum_f n_f^2 / M (PopulationAnnealing.rho_t).  Needs PopulationAnnealing(..., families=True)."""
    return _find_annealing(simulation).rho_t()
