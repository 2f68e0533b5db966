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
``blocks=B`` partitions the FAMILIES into B blocks -- descendants of different ancestors never share a parent, so these blocks stay
independent where blocks of slots do not -- and the engine keeps the weight sums of every step per block: ``log_z(error=True)`` is a
delete-one-block jackknife over them (DESIGN.md section 3.14 "Error bars").
"""
from __future__ import annotations

import math
import struct

import numpy as np

from . import sharding
from ._capi import (AMC_MAX_JK_BLOCKS, AMC_ANNEAL_MAX_RECORDS, AMC_ANNEAL_RECORD_WORDS, AMC_ANNEAL_SEARCH_MAX_ROUNDS, AMC_ANNEAL_SEARCH_STALLED,
                    AMC_ANNEAL_SEARCH_WORDS, AMC_ANNEAL_WEIGHT_BITS, AMC_EHIST_MAX_BINS)
from .metropolis import Metropolis
from .simulation import AriannaAlgorithm, Simulation, _calls


def _f64(bits) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(bits)))[0]


# the status word of a search (search_log()[:, 0]; include/amc.h AMC_ANNEAL_SEARCH_*), by value
ANNEAL_SEARCH_STATUS = ("OK", "LIMIT", "BELOW_RESOLUTION", "STALLED", "ALL_NAN", "INF", "NO_WEIGHT")


def _adaptive_plan(adaptive) -> dict:
    """adaptive=dict(beta_end=..., target=..., rounds=6), checked: what PopulationAnnealing hands to anneal_next_beta."""
    try:
        plan = dict(adaptive)
    except (TypeError, ValueError):
        raise ValueError(f"PopulationAnnealing: adaptive = {adaptive!r} is not a dict(beta_end=..., target=..., rounds=6)") from None
    unknown = sorted(set(plan) - {"beta_end", "target", "rounds"})
    if unknown:
        raise ValueError(f"PopulationAnnealing: adaptive has unknown keys {unknown} (beta_end, target, rounds)")
    for key in ("beta_end", "target"):
        if key not in plan:
            raise ValueError(f"PopulationAnnealing: adaptive[{key!r}] is missing (it has no default)")
    beta_end, target, rounds = float(plan["beta_end"]), float(plan["target"]), plan.get("rounds", 6)
    if not math.isfinite(beta_end):
        raise ValueError(f"PopulationAnnealing: adaptive['beta_end'] = {beta_end!r} is not finite")
    if not 0.0 < target < 1.0:
        raise ValueError(f"PopulationAnnealing: adaptive['target'] = {target!r} must lie strictly between 0 and 1 (the effective-sample "
                         "fraction a step keeps)")
    if int(rounds) != rounds or not 1 <= int(rounds) <= AMC_ANNEAL_SEARCH_MAX_ROUNDS:
        raise ValueError(f"PopulationAnnealing: adaptive['rounds'] = {rounds!r} must be an integer in [1, {AMC_ANNEAL_SEARCH_MAX_ROUNDS}]")
    return dict(beta_end=beta_end, target=target, rounds=int(rounds))


def _histogram_plan(energy_histogram) -> dict:
    """energy_histogram=dict(lo=..., hi=..., n_bins=..., max_outside=0.0), checked."""
    try:
        plan = dict(energy_histogram)
    except (TypeError, ValueError):
        raise ValueError(f"PopulationAnnealing: energy_histogram = {energy_histogram!r} is not a dict(lo=..., hi=..., n_bins=...)") from None
    unknown = sorted(set(plan) - {"lo", "hi", "n_bins", "max_outside"})
    if unknown:
        raise ValueError(f"PopulationAnnealing: energy_histogram has unknown keys {unknown} (lo, hi, n_bins, max_outside)")
    for key in ("lo", "hi", "n_bins"):
        if key not in plan:
            raise ValueError(f"PopulationAnnealing: energy_histogram[{key!r}] is missing (it has no default)")
    lo, hi, n_bins, max_outside = float(plan["lo"]), float(plan["hi"]), plan["n_bins"], float(plan.get("max_outside", 0.0))
    if int(n_bins) != n_bins or not 1 <= int(n_bins) <= AMC_EHIST_MAX_BINS or not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"PopulationAnnealing: energy_histogram needs an integer 1 <= n_bins <= {AMC_EHIST_MAX_BINS} and finite lo < hi, got {plan!r}")
    if not 0.0 <= max_outside <= 1.0:
        raise ValueError(f"PopulationAnnealing: energy_histogram['max_outside'] = {max_outside!r} must lie in [0, 1]")
    return dict(lo=lo, hi=hi, n_bins=int(n_bins), max_outside=max_outside)


class PopulationAnnealing(AriannaAlgorithm):
    """PopulationAnnealing(chains; dependencies=(Metropolis,), betas=[...], families=False): one annealing step of the Metropolis'
    engine per scheduled time, to the next beta of ``betas``.  Listed behind its Metropolis, a time step at which both are due is
    [sweep; anneal].  It is an error when the list runs out.

    PopulationAnnealing(..., adaptive=dict(beta_end=..., target=..., rounds=6)) instead of ``betas``: each scheduled call is
    [next_beta; anneal] -- the engine finds the largest step towards ``beta_end`` whose reweighting keeps the effective-sample fraction
    ESS / M at or above ``target`` (DESIGN.md section 3.14 "Choosing the next beta") and anneals to it.  The number of steps is not
    known in advance: once beta == beta_end, scheduled calls launch nothing and append no record (``finished``).

    PopulationAnnealing(..., energy_histogram=dict(lo=..., hi=..., n_bins=..., max_outside=0.0)): before each annealing step, and once
    at ``finalise``, the energy histogram of the population at the beta in force is taken on the device (DESIGN.md section 3.17:
    [accumulate; fetch with reset]) and kept with its beta; ``histograms()`` returns them, ``reweight(betas)`` applies
    multiple-histogram reweighting over the temperatures of the schedule.  Without the option nothing new is launched.

    PopulationAnnealing(..., blocks=B, block_chunk=None) implies ``families=True`` and sets the engine's partition into blocks of
    families, block of a chain = (family id div chunk) mod B (chunk None: ceil(M / B), every block one contiguous range of ancestors).
    Every annealing step then appends a block record beside its record (one more launch per step); ``block_records()`` returns them,
    ``log_z_ratios(error=True)`` / ``log_z(error=True)`` return (value, se) by the delete-one-block jackknife of
    ``jackknife.anneal_log_z``.  Together with ``energy_histogram=...`` the histogram of every temperature is kept per block of families
    (``histograms_blocks()``) and ``reweight(betas, error=True)`` returns the curve with its standard errors.  Without the option
    nothing new is launched or allocated."""

    mutates_chains = True          # a callback due behind it at the same t observes the state AFTER the resampling

    def __init__(self, chains, dependencies=None, betas=None, adaptive=None, families=False, energy_histogram=None, blocks=None,
                 block_chunk=None, path=None, **extras):
        assert dependencies is not None and len(dependencies) == 1 and isinstance(dependencies[0], Metropolis)
        self.metropolis: Metropolis = dependencies[0]
        if adaptive is not None and betas is not None:
            raise ValueError("PopulationAnnealing: both betas and adaptive are given; a run walks a list or chooses its steps, not both")
        self.adaptive = None if adaptive is None else _adaptive_plan(adaptive)
        if self.adaptive is None and (betas is None or len(betas) == 0):
            raise ValueError("PopulationAnnealing: betas is missing (the list of beta values to anneal to, one per scheduled call)")
        self.betas = [] if betas is None else [float(b) for b in betas]
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
        if self.adaptive is not None and not hasattr(self.metropolis.engine, "anneal_next_beta"):
            raise ValueError("PopulationAnnealing: this engine cannot choose the next beta (adaptive needs amc_anneal_next_beta)")
        self.blocks = None                     # blocks=B: the partition (B, chunk) over the families
        if blocks is None or blocks is False:
            if block_chunk is not None:
                raise ValueError(f"PopulationAnnealing: block_chunk = {block_chunk!r} without blocks")
        else:
            if int(blocks) != blocks or not 2 <= int(blocks) <= AMC_MAX_JK_BLOCKS:
                raise ValueError(f"PopulationAnnealing: blocks = {blocks!r} must be an integer in [2, {AMC_MAX_JK_BLOCKS}]")
            B, M = int(blocks), len(chains)
            chunk = -(-M // B) if block_chunk is None else block_chunk
            if int(chunk) != chunk or int(chunk) < 1:
                raise ValueError(f"PopulationAnnealing: block_chunk = {block_chunk!r} must be an integer >= 1")
            if -(-M // int(chunk)) < B:
                raise ValueError(f"PopulationAnnealing: {M} families in chunks of {int(chunk)} make fewer chunks than blocks = {B} (a block "
                                 "would hold no family)")
            if not hasattr(self.metropolis.engine, "set_anneal_blocks"):
                raise ValueError("PopulationAnnealing: this engine keeps no weight sums per block of families (blocks needs amc_set_anneal_blocks)")
            self.blocks = (B, int(chunk))
            families = True                    # the partition is a function of the family ids
        self.families = bool(families)
        self.hist_plan = None if energy_histogram is None else _histogram_plan(energy_histogram)
        if self.hist_plan is not None and not hasattr(self.metropolis.engine, "energy_histogram_accumulate"):
            raise ValueError("PopulationAnnealing: this engine has no energy histograms (energy_histogram needs amc_energy_histogram_accumulate)")
        self._hist = []                        # energy_histogram: (beta, row[n_bins + 3]) per temperature, oldest first
        self._hist_blocks = []                 # ... with blocks=B: rows[B, n_bins + 3] per temperature beside them, one per block of families
        self._hist_final = False               # ... the last one was taken by finalise (a checkpoint leaves it out: the resumed run takes
                                               # the histogram of that beta itself, in front of its next step or at its own finalise)
        self.chains = chains
        self._records = []                     # records drained from the engine's log, oldest first
        self._block_records = []               # blocks=B: the block records drained beside them, [2, B] each
        self._search_log = []                  # adaptive: the diag of every search of this process, oldest first
        self.metropolis.annealing = self       # (storage.checkpoint: beta, the step index, the records and the families are state)
        self.rank, _ = sharding.world()

    def initialise(self, simulation: Simulation) -> None:
        from .exchange import ReplicaExchange
        if any(isinstance(a, ReplicaExchange) for a in simulation.algorithms):
            raise ValueError("PopulationAnnealing: the algorithm list holds a ReplicaExchange; a ladder and an annealed population "
                             "exclude each other")
        if self.families and not self.metropolis.families_restored:     # (restored: storage.restore brought them back)
            self.metropolis.engine.set_anneal_families(True)
        if self.blocks is not None and not self.metropolis.anneal_blocks_restored:      # (behind the families: it needs them)
            self.metropolis.engine.set_anneal_blocks(*self.blocks)

    def make_step(self, simulation: Simulation) -> None:
        eng = self.metropolis.engine
        i = eng.anneal_step
        if self.adaptive is None:
            if i >= len(self.betas):
                raise ValueError(f"PopulationAnnealing: annealing step {i + 1} is due and betas holds {len(self.betas)} values")
            beta_new = self.betas[i]
        else:
            if self.finished:                   # at beta_end: nothing is launched, no record is appended
                return
            plan = self.adaptive
            beta_new, diag, _ = eng.anneal_next_beta(plan["beta_end"], plan["target"], plan["rounds"])
            if int(diag[0]) == AMC_ANNEAL_SEARCH_STALLED:
                raise ValueError(f"PopulationAnnealing: the search stalled at beta = {eng.beta!r}: the smallest step it resolves towards "
                                 f"beta_end = {plan['beta_end']!r} does not change beta in the state's type (more rounds, or a beta_end "
                                 "closer by)")
            self._search_log.append(np.array(diag, dtype=np.uint64))
        if i - len(self._records) >= AMC_ANNEAL_MAX_RECORDS:
            self._drain()
        if self.hist_plan is not None:
            self._take_histogram(final=False)
        eng.anneal(beta_new)
        self.chains.beta = beta_new
        self.metropolis.invalidate_reductions()

    def finalise(self, simulation: Simulation) -> None:
        if self.hist_plan is not None and not self._hist_final:
            self._take_histogram(final=True)

    def _take_histogram(self, final: bool) -> None:
        """[accumulate; fetch with reset] at the beta in force: one row, kept with its beta.  The histogram finalise took is replaced
        when the run goes on (the population has been swept since)."""
        eng, plan = self.metropolis.engine, self.hist_plan
        if self._hist_final:
            self._hist.pop()
            if self.blocks is not None:
                self._hist_blocks.pop()
        if self.blocks is not None:            # a row per block of families; their sum is the plain histogram cell for cell
            eng.energy_histogram_accumulate_blocks(plan["lo"], plan["hi"], plan["n_bins"])
            per_block = np.array(eng.energy_histogram_fetch_blocks(reset=True)[0], dtype=np.uint64).reshape(self.blocks[0], plan["n_bins"] + 3)
            self._hist_blocks.append(per_block)
            self._hist.append((float(eng.beta), per_block.sum(axis=0, dtype=np.uint64)))
        else:
            eng.energy_histogram_accumulate(plan["lo"], plan["hi"], plan["n_bins"])
            counts, _, _ = eng.energy_histogram_fetch(reset=True)
            self._hist.append((float(eng.beta), np.array(counts[0], dtype=np.uint64)))
        self._hist_final = bool(final)

    def histograms(self):
        """(betas[S], counts[S, n_bins + 3]): the energy histogram taken at every temperature so far, the bins, then below lo, at or
        above hi, NaN.  Needs energy_histogram=..."""
        if self.hist_plan is None:
            raise ValueError("PopulationAnnealing.histograms needs the histograms: build the PopulationAnnealing with energy_histogram=dict(...)")
        n = self.hist_plan["n_bins"] + 3
        return (np.array([b for b, _ in self._hist], dtype=np.float64),
                np.array([c for _, c in self._hist], dtype=np.uint64).reshape(-1, n))

    def histograms_blocks(self):
        """(betas[S], counts[S, B, n_bins + 3]): the histograms() per block of families -- chain c counted in the row of block
        (family id div chunk) mod B; the sum over the blocks is histograms() cell for cell.  Needs energy_histogram=... and blocks=B."""
        if self.hist_plan is None or self.blocks is None:
            raise ValueError("PopulationAnnealing.histograms_blocks needs the histograms per block: build the PopulationAnnealing with "
                             "energy_histogram=dict(...) and blocks=B")
        n = self.hist_plan["n_bins"] + 3
        return (np.array([b for b, _ in self._hist], dtype=np.float64),
                np.array(self._hist_blocks, dtype=np.uint64).reshape(-1, self.blocks[0], n))

    def reweight(self, betas, error: bool = False, **kw):
        """(log Z, <e>, <e^2>, C) at every beta of ``betas`` by multiple-histogram reweighting over the temperatures of the schedule
        (reweighting.wham / reweight); log Z is 0 at the first temperature.  Raises, naming the temperature and the cell, when a
        histogram's share outside the bins exceeds ``max_outside``.
        error=True (needs blocks=B): ((log Z, <e>, <e^2>, C), (their standard errors)) by the delete-one-block jackknife over the
        blocks of families (jackknife.jackknife_counts): every replicate is the whole of WHAM and the reweighting on the counts of ALL
        temperatures without block b -- the same families appear at every temperature, so the block is deleted everywhere at once."""
        from . import reweighting
        b, counts = self.histograms()
        if not len(b):
            raise ValueError("PopulationAnnealing.reweight: no histogram has been taken yet")
        plan = self.hist_plan
        share = reweighting.outside_share(counts)
        bad = np.argwhere(share > plan["max_outside"])
        if bad.size:
            s, c = int(bad[0][0]), int(bad[0][1])
            raise ValueError(f"PopulationAnnealing: the histogram at beta = {b[s]!r} (temperature {s}) has a share of {share[s, c]:.3e} of its "
                             f"samples in the cell '{('below lo', 'at or above hi', 'NaN')[c]}' (max_outside = {plan['max_outside']:g}): "
                             f"widen [lo, hi) = [{plan['lo']:g}, {plan['hi']:g})")
        energies = reweighting.bin_centres(plan["lo"], plan["hi"], plan["n_bins"])
        if not error:
            log_g = reweighting.wham(counts[:, :plan["n_bins"]], b, energies, **kw)[0]
            return reweighting.reweight(log_g, energies, betas)
        from . import jackknife
        per_block = self.histograms_blocks()[1]                       # [S, B, n_bins + 3]
        start = {}

        def curve(c):                                                  # c[S, n_bins]: the full counts first, then every replicate's
            log_g, f, _ = reweighting.wham(c, b, energies, **dict(kw, f0=start.get("f", kw.get("f0"))))
            start.setdefault("f", f)                                   # the replicates start from the full solution
            return np.array(reweighting.reweight(log_g, energies, np.atleast_1d(np.asarray(betas, dtype=np.float64))))

        theta, se = jackknife.jackknife_counts(np.ascontiguousarray(per_block.transpose(1, 0, 2)[:, :, :plan["n_bins"]]), curve)
        return tuple(theta), tuple(se)

    def histogram_state(self) -> dict:
        """The section of a checkpoint: the bins and the list, without the histogram finalise took."""
        if self.hist_plan is None:
            return {}
        b, counts = self.histograms()
        keep = len(b) - (1 if self._hist_final else 0)
        plan = self.hist_plan
        out = dict(anneal_hist_bins=np.array([plan["lo"], plan["hi"], float(plan["n_bins"])]), anneal_hist_betas=b[:keep],
                   anneal_hist_counts=counts[:keep])
        if self.blocks is not None:            # blocks=B: the rows per block of families (no field otherwise)
            out["anneal_hist_block_counts"] = self.histograms_blocks()[1][:keep]
        return out

    def set_histogram_state(self, d) -> None:
        if self.hist_plan is None or "anneal_hist_bins" not in d:
            return
        lo, hi, n_bins = (float(v) for v in d["anneal_hist_bins"])
        plan = self.hist_plan
        if (lo, hi, int(n_bins)) != (plan["lo"], plan["hi"], plan["n_bins"]):
            raise ValueError(f"checkpoint holds annealing histograms with the bins {(lo, hi, int(n_bins))}, this PopulationAnnealing asks "
                             f"for {(plan['lo'], plan['hi'], plan['n_bins'])}")
        counts = np.asarray(d["anneal_hist_counts"], dtype=np.uint64).reshape(-1, plan["n_bins"] + 3)
        self._hist = [(float(b), c.copy()) for b, c in zip(d["anneal_hist_betas"], counts)]
        self._hist_final = False
        if self.blocks is not None:
            if "anneal_hist_block_counts" not in d:
                if len(counts):
                    raise ValueError("checkpoint holds annealing histograms without histograms per block, this PopulationAnnealing asks for blocks")
                self._hist_blocks = []
            else:
                per_block = np.asarray(d["anneal_hist_block_counts"], dtype=np.uint64).reshape(-1, self.blocks[0], plan["n_bins"] + 3)
                self._hist_blocks = [c.copy() for c in per_block]

    @property
    def finished(self) -> bool:
        """No annealing step is left: beta has reached beta_end (adaptive), or the list has been walked."""
        if self.adaptive is not None:
            return float(self.metropolis.engine.beta) == self.adaptive["beta_end"]
        return self.metropolis.engine.anneal_step >= len(self.betas)

    def search_log(self) -> np.ndarray:
        """adaptive: one row of 8 unsigned 64-bit words per search of this process (a resumed run starts an empty log): status, rounds
        decided, bits of the step chosen, rho at the bracket's low end, bits of its high end, rho there, bits of the largest and of the
        smallest -e."""
        return np.array(self._search_log, dtype=np.uint64).reshape(-1, AMC_ANNEAL_SEARCH_WORDS)

    def _drain(self) -> None:
        eng = self.metropolis.engine
        rec = np.asarray(eng.anneal_records(reset=True), dtype=np.uint64).reshape(-1, AMC_ANNEAL_RECORD_WORDS)
        self._records.extend(rec.copy())
        if self.blocks is not None:            # both logs in this one place: they stay aligned
            blk = np.asarray(eng.anneal_block_records(reset=True), dtype=np.uint64).reshape(-1, 2, self.blocks[0])
            if len(blk) != len(rec):
                raise ValueError(f"PopulationAnnealing: the engine's log holds {len(rec)} records and {len(blk)} block records (steps were "
                                 "taken without the partition, or one log was drained alone)")
            self._block_records.extend(blk.copy())

    @property
    def beta(self) -> float:
        """The shared beta in force."""
        return float(self.metropolis.engine.beta)

    def records(self) -> np.ndarray:
        """One row of 8 unsigned 64-bit words per annealing step so far: status, bits of beta before, bits of beta after, bits of
        a_max, T_w, U, n_parents, max_children.  The host waits for the queued steps."""
        self._drain()
        return np.array(self._records, dtype=np.uint64).reshape(-1, AMC_ANNEAL_RECORD_WORDS)

    def block_records(self) -> np.ndarray:
        """[steps, 2, B] unsigned 64-bit words, one block record per annealing step so far: n_b, the chains of block b before the
        resampling, then T_b, the sum of their integer weights (sum_b T_b = T_w, sum_b n_b = M).  Needs blocks=B; the host waits."""
        if self.blocks is None:
            raise ValueError("PopulationAnnealing.block_records needs the partition: build the PopulationAnnealing with blocks=B")
        self._drain()
        return np.array(self._block_records, dtype=np.uint64).reshape(-1, 2, self.blocks[0])

    def _log_z_error(self, cumulative: bool):
        from . import jackknife
        if self.blocks is None:
            raise ValueError("PopulationAnnealing: error=True needs the partition: build the PopulationAnnealing with blocks=B")
        value, se, _ = jackknife.anneal_log_z(self.records(), self.block_records(), len(self.chains), cumulative=cumulative)
        return value, se

    def log_z_ratios(self, error: bool = False):
        """log(Z(beta_to) / Z(beta_from)) per annealing step: a_max + log T_w - log M - 30 log 2, the log of the mean reweighting
        factor, formed from the integer records (the same number on any grid); NaN for a step that did not resample.
        error=True (needs blocks=B): (value, se), se by the delete-one-block jackknife over the blocks of families, per step."""
        if error:
            return self._log_z_error(cumulative=False)
        M = float(len(self.chains))
        out = [(_f64(r[3]) + math.log(int(r[4])) - math.log(M) - AMC_ANNEAL_WEIGHT_BITS * math.log(2.0)) if int(r[0]) == 0 else math.nan
               for r in self.records()]
        return np.array(out, dtype=np.float64)

    def log_z(self, error: bool = False):
        """log(Z(beta_i) / Z(beta_start)) after every annealing step: the cumulative sum of log_z_ratios() from the first beta.
        error=True (needs blocks=B): (value, se).  Replicate b of log Z after step t is the sum over s <= t of
        a_max^s + log(T_w^s - T_b^s) - log(M - n_b^s) - 30 log 2 -- the replicate of the cumulative sum, not a sum of per-step errors
        --, se^2 = (B' - 1) / B' sum_b (theta_b - mean)^2 over the B' blocks that held a family at the first step.  A replicate whose
        argument is 0 (one block holds every chain, or all the weight) is NaN from that step on, and so is the se."""
        if error:
            return self._log_z_error(cumulative=True)
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
        if self.adaptive is None:
            betas = f"\t\tBetas: {len(self.betas)} from {self.betas[0]} to {self.betas[-1]}\n"
        else:
            betas = (f"\t\tBetas: adaptive, ESS / M >= {self.adaptive['target']} per step, to {self.adaptive['beta_end']} "
                     f"({self.adaptive['rounds']} rounds)\n")
        blocks = "" if self.blocks is None else f"\t\tBlocks: {self.blocks[0]} of families, chunk {self.blocks[1]}\n"
        io.write(f"\tPopulationAnnealing\n\t\tCalls: {_calls(scheduler)}\n{betas}\t\tFamilies: {str(self.families).lower()}\n{blocks}")


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


def callback_anneal_log_z_error(simulation: Simulation) -> float:
    """The jackknife standard error of callback_anneal_log_z (the last se of PopulationAnnealing.log_z(error=True); 0 before the first
    step).  Needs PopulationAnnealing(..., blocks=B).  The host waits for the queued steps."""
    se = _find_annealing(simulation).log_z(error=True)[1]
    return float(se[-1]) if se.size else 0.0


def callback_rho_t(simulation: Simulation) -> float:
    """rho_t = sum_f n_f^2 / M (PopulationAnnealing.rho_t).  Needs PopulationAnnealing(..., families=True)."""
    return _find_annealing(simulation).rho_t()
