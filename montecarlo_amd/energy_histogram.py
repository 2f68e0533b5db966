"""``EnergyHistogram``: per rung a histogram of the chains' energies, accumulated on the device, and the curve between the
simulated temperatures from it.

An extension over the reference, like ``ReplicaExchange`` and ``Autocorrelation``.  The engine bins e = potential(x) of every chain
into the row of its group -- the rungs of the ladder, ONE group without a ladder -- in one memory-bound pass per scheduled call
(include/amc.h amc_energy_histogram_accumulate); the counts are integers, the same on any grid, in any
snapshot order and on any split into shards.  Multiple-histogram reweighting (``reweighting.wham``) turns the rows into the density
of states log g(E), the free energy per rung and <e>(beta), C(beta), log Z(beta) at any beta between the rungs; with one group it
is single-histogram reweighting around the shared beta.

With ``blocks=B`` the engine keeps the counts per jackknife block of ladders (DESIGN.md section 3.17 "Per block"), and every result
comes with a delete-one-block standard error (``error=True``): each replicate is the whole of WHAM and the reweighting on its
leave-one-out counts.

With ``moments=("x", "x2", "pos")`` and ``x_bound=...`` the pass also adds x, x^2 and [x > 0] of the chains of every bin into integer
sums on the device (DESIGN.md section 3.17 "Moments per bin"; include/amc.h amc_energy_moments_accumulate), and
``reweight_moments(betas)`` gives <x>, <x^2> and the occupancy of the right-hand well at any beta: functions of the position, which
the counts alone cannot give.  Together with ``blocks=B`` the sums are kept per jackknife block too (DESIGN.md section 3.17 "Moments
per block"), and ``reweight_moments(betas, error=True)`` returns every value with its standard error.
"""
from __future__ import annotations

import numpy as np

from . import jackknife, reweighting, sharding
from ._capi import AMC_EHIST_MAX_BINS, AMC_EMOM_POS, AMC_EMOM_X, AMC_EMOM_XX
from .metropolis import Metropolis
from .simulation import AriannaAlgorithm, Simulation, _calls

_CELLS = ("below lo", "at or above hi", "NaN", "x beyond x_bound")
MOMENTS = {"x": AMC_EMOM_X, "x2": AMC_EMOM_XX, "pos": AMC_EMOM_POS}      # name -> column bit; the columns stand in bit order


def emom_quanta(x_bound: float):
    """(2^E_X, 2^E_XX, 1): the quantum of every column under ``x_bound`` -- eb = ilogb(x_bound) + 1, E_X = eb - 32, E_XX = 2 eb - 32."""
    eb = int(np.floor(np.log2(float(x_bound)))) + 1
    if not 2.0 ** (eb - 1) <= float(x_bound) < 2.0 ** eb:      # (log2 rounded across a power of two)
        eb += 1 if float(x_bound) >= 2.0 ** eb else -1
    return {AMC_EMOM_X: 2.0 ** (eb - 32), AMC_EMOM_XX: 2.0 ** (2 * eb - 32), AMC_EMOM_POS: 1.0}


class EnergyHistogram(AriannaAlgorithm):
    """EnergyHistogram(chains; dependencies=(Metropolis,), scheduler=..., lo=..., hi=..., n_bins=..., max_outside=0.0): one snapshot of
    the energy histograms per scheduled time, on the Metropolis' engine.  It observes only: listed behind its Metropolis (and its
    ReplicaExchange), a time step at which all are due is [sweep; exchange; snapshot].

    ``counts()`` are the counts of ALL ranks, ``reweight(betas)`` the curve.  ``max_outside``: the largest share of a row that may lie
    in one of the three cells outside the bins (below lo, at or above hi, NaN) before ``reweight`` / ``density_of_states`` /
    ``free_energies`` refuse: what lies outside is missing from the reweighted sums, so the default tolerates nothing.

    ``blocks=B`` (``block_chunk=C``, default ``jackknife.default_chunk``): the counts are kept per block of the jackknife partition
    (B, C) -- one partition per Metropolis, shared with a ReplicaExchange / Autocorrelation that asks for blocks --;
    ``counts_blocks()`` returns them, ``counts()`` their sum, and ``reweight`` / ``free_energies`` / ``density_of_states`` take
    ``error=True``.

    ``moments=("x", "x2", "pos")`` (any of the three) with ``x_bound=...``: the pass keeps, per bin, the sums of x, x^2 and [x > 0]
    beside the counts, in an accumulator of their own; ``moment_sums()``, ``microcanonical()``, ``reweight_moments(betas)`` return
    them.  A chain of a bin with |x| > x_bound (or NaN) is counted in a fourth cell outside the bins, "x beyond x_bound", which
    ``max_outside`` covers too.  Together with ``blocks=B`` counts and sums are kept per jackknife block (``counts_blocks()``,
    ``moment_sums_blocks()``), and ``reweight_moments(betas, error=True)`` gives {name: (value, se)}."""

    def __init__(self, chains, dependencies=None, lo=None, hi=None, n_bins=None, max_outside=0.0, blocks=None, block_chunk=None, path=None,
                 moments=None, x_bound=None, **extras):
        assert dependencies is not None and len(dependencies) == 1 and isinstance(dependencies[0], Metropolis)
        self.metropolis: Metropolis = dependencies[0]
        if lo is None or hi is None or n_bins is None:
            raise ValueError("EnergyHistogram: lo, hi and n_bins are required")
        if int(n_bins) != n_bins or not 1 <= int(n_bins) <= AMC_EHIST_MAX_BINS or not (np.isfinite(lo) and np.isfinite(hi) and float(lo) < float(hi)):
            raise ValueError(f"EnergyHistogram: need an integer 1 <= n_bins <= {AMC_EHIST_MAX_BINS} and finite lo < hi, got lo = {lo!r}, hi = {hi!r}, n_bins = {n_bins!r}")
        if not 0.0 <= float(max_outside) <= 1.0:
            raise ValueError(f"EnergyHistogram: max_outside = {max_outside!r} must lie in [0, 1]")
        if not hasattr(self.metropolis.engine, "energy_histogram_accumulate"):
            raise ValueError("EnergyHistogram: this engine has no energy histograms (streams > 1 is not supported)")
        self.mask, self.moments, self.x_bound = 0, (), None
        if moments is not None:
            names = (moments,) if isinstance(moments, str) else tuple(moments)
            if not names or any(n not in MOMENTS for n in names) or len(set(names)) != len(names):
                raise ValueError(f"EnergyHistogram: moments = {moments!r}: need one or more of {tuple(MOMENTS)}, each once")
            if x_bound is None:
                raise ValueError("EnergyHistogram: moments need x_bound, the largest |x| a binned chain may have (it fixes the sums' quanta)")
            if not (np.isfinite(x_bound) and 2.0 ** -500 <= float(x_bound) < 2.0 ** 500):
                raise ValueError(f"EnergyHistogram: x_bound = {x_bound!r} must be finite, positive and within [2^-500, 2^500)")
            if not hasattr(self.metropolis.engine, "energy_moments_accumulate"):
                raise ValueError("EnergyHistogram: this engine keeps no moments per energy bin (streams > 1 is not supported)")
            self.moments = tuple(n for n in MOMENTS if n in names)      # (in column order)
            self.mask = sum(MOMENTS[n] for n in self.moments)
            self.x_bound = float(x_bound)
        elif x_bound is not None:
            raise ValueError("EnergyHistogram: x_bound without moments")
        self.chains = chains
        self.lo, self.hi, self.n_bins, self.max_outside = float(lo), float(hi), int(n_bins), float(max_outside)
        self.metropolis.energy_histogram = self     # (storage.checkpoint: the accumulator is state)
        groups = int(getattr(chains, "n_rungs", None) or 1)
        if blocks is not None and block_chunk is None and self.metropolis.blocks and self.metropolis.blocks[0] == int(blocks):
            block_chunk = self.metropolis.blocks[1]      # (another algorithm of these chains set the chunk: one partition per engine)
        self.blocks = jackknife.check_blocks("EnergyHistogram", blocks, block_chunk, len(chains) // groups, groups)
        if self.blocks:
            if not hasattr(self.metropolis.engine, "energy_moments_accumulate_blocks" if self.mask else "energy_histogram_accumulate_blocks"):
                raise ValueError("EnergyHistogram: this engine keeps no energy histograms per block (streams > 1 is not supported)")
            jackknife.ask_blocks("EnergyHistogram", self.metropolis, self.blocks)

    # -- scheduling -----------------------------------------------------------------------------------------------------------------
    def initialise(self, simulation: Simulation) -> None:
        from .annealing import PopulationAnnealing
        if any(isinstance(a, PopulationAnnealing) for a in simulation.algorithms):
            raise ValueError("EnergyHistogram beside a PopulationAnnealing: a histogram belongs to one beta, and annealing moves it; "
                             "PopulationAnnealing(..., energy_histogram=dict(lo=..., hi=..., n_bins=...)) keeps one histogram per temperature")
        if self.blocks:
            jackknife.refuse_annealing("EnergyHistogram", simulation)
            from .exchange import ReplicaExchange
            if any(isinstance(a, ReplicaExchange) and a.bridge and not a.blocks for a in simulation.algorithms):
                raise ValueError("EnergyHistogram: blocks beside a ReplicaExchange(bridge=...) without blocks: setting the partition at the "
                                 "first snapshot would clear the bridge sums accumulated so far; give the ReplicaExchange the same blocks")

    def make_step(self, simulation: Simulation) -> None:
        if self.blocks:                         # (here and not in initialise: every algorithm's set_ladder lies behind us by now)
            jackknife.use_blocks(self.metropolis, self.blocks)
            if self.mask:
                self.metropolis.engine.energy_moments_accumulate_blocks(self.lo, self.hi, self.n_bins, self.mask, self.x_bound)
            else:
                self.metropolis.engine.energy_histogram_accumulate_blocks(self.lo, self.hi, self.n_bins)
        elif self.mask:
            self.metropolis.engine.energy_moments_accumulate(self.lo, self.hi, self.n_bins, self.mask, self.x_bound)
        else:
            self.metropolis.engine.energy_histogram_accumulate(self.lo, self.hi, self.n_bins)

    def restart(self) -> None:
        """Drop what has been accumulated (fetch with reset); the next scheduled call begins anew."""
        if self.mask:
            self.metropolis.engine.energy_moments_fetch(reset=True)
        else:
            self.metropolis.engine.energy_histogram_fetch(reset=True)

    # -- results --------------------------------------------------------------------------------------------------------------------
    def _groups(self) -> int:
        return max(int(self.metropolis.n_rungs), 1)

    def _local(self):
        """(counts[G, n_bins + 3], n_snapshots) of this shard; zeros while nothing has been accumulated."""
        if self.mask:                           # (the moments' pass counts too: its first n_bins + 3 cells)
            counts, _, n_snap = self._local_moments()
            return np.ascontiguousarray(counts[:, :self.n_bins + 3]), n_snap
        counts, n_snap, (lo, hi, n_bins) = self.metropolis.engine.energy_histogram_fetch(reset=False)
        if n_bins == 0:
            return np.zeros((self._groups(), self.n_bins + 3), dtype=np.uint64), 0
        if (lo, hi, n_bins) != (self.lo, self.hi, self.n_bins):
            raise ValueError(f"EnergyHistogram: the engine's accumulator has the bins {(lo, hi, n_bins)}, this algorithm asks for "
                             f"{(self.lo, self.hi, self.n_bins)}")
        return counts, n_snap

    def _local_moments(self):
        """(counts[G, n_bins + 4], sums[G, C, n_bins] int64, n_snapshots) of this shard; zeros while nothing has been accumulated."""
        if not self.mask:
            raise ValueError("EnergyHistogram: the moments per bin need moments=(...) and x_bound")
        counts, sums, n_snap, form = self.metropolis.engine.energy_moments_fetch(reset=False)
        if form[2] == 0:
            G = self._groups()
            return np.zeros((G, self.n_bins + 4), dtype=np.uint64), np.zeros((G, len(self.moments), self.n_bins), dtype=np.int64), 0
        mine = (self.lo, self.hi, self.n_bins, self.mask, self.x_bound)
        if form != mine:
            raise ValueError(f"EnergyHistogram: the engine's accumulator has the form (lo, hi, n_bins, mask, x_bound) = {form}, this algorithm "
                             f"asks for {mine}")
        return counts, sums, n_snap

    def counts(self) -> np.ndarray:
        """counts[G, n_bins + 3] (uint64) of ALL ranks: the bins, then below lo, at or above hi, NaN.  Summed exactly: a 64-bit count
        travels as two halves below 2^32, so the Float64 sum over the ranks rounds nothing.  The host waits for the queued
        snapshots."""
        return self._all_ranks(self._local()[0])

    def _all_ranks(self, local: np.ndarray) -> np.ndarray:
        if self.metropolis.world_size <= 1:
            return local
        halves = np.concatenate([(local & np.uint64(0xFFFFFFFF)).ravel(), (local >> np.uint64(32)).ravel()]).astype(np.float64)
        total = sharding.allreduce_sum(halves, self.metropolis.engine)
        lo_half, hi_half = total[:local.size].astype(np.uint64), total[local.size:].astype(np.uint64)
        return (lo_half + (hi_half << np.uint64(32))).reshape(local.shape)

    def _local_blocks(self):
        """(counts[B, G, n_bins + 3], n_snapshots) of this shard; zeros while nothing has been accumulated."""
        if not self.blocks:
            raise ValueError("EnergyHistogram: counts per block need blocks=B")
        if self.mask:                           # (the moments' pass counts too: the first n_bins + 3 cells of every row)
            counts, _, n_snap = self._local_moments_blocks()
            return np.ascontiguousarray(counts[:, :, :self.n_bins + 3]), n_snap
        if self._local()[1] == 0:               # (nothing stands, or other bins: _local has said so)
            return np.zeros((self.blocks[0], self._groups(), self.n_bins + 3), dtype=np.uint64), 0
        counts, n_snap, _ = self.metropolis.engine.energy_histogram_fetch_blocks(reset=False)
        return counts, n_snap

    def _local_moments_blocks(self):
        """(counts[B, G, n_bins + 4], sums[B, G, C, n_bins] int64, n_snapshots) of this shard; zeros while nothing has been accumulated."""
        if not self.blocks:
            raise ValueError("EnergyHistogram: moments per block need blocks=B")
        if self._local_moments()[2] == 0:       # (nothing stands, or another form: _local_moments has said so)
            B, G = self.blocks[0], self._groups()
            return np.zeros((B, G, self.n_bins + 4), dtype=np.uint64), np.zeros((B, G, len(self.moments), self.n_bins), dtype=np.int64), 0
        counts, sums, n_snap, _ = self.metropolis.engine.energy_moments_fetch_blocks(reset=False)
        return counts, sums, n_snap

    def counts_blocks(self) -> np.ndarray:
        """counts[B, G, n_bins + 3] (uint64) of ALL ranks per jackknife block: blocks are functions of the global ladder index, so the
        shards add cell by cell (the two halves of ``counts()``).  Needs ``blocks=B``; their sum over B is ``counts()``."""
        return self._all_ranks(self._local_blocks()[0])

    @property
    def n_snapshots(self) -> int:
        """Snapshots in the accumulator (every rank takes the same number)."""
        return self._local()[1]

    def betas(self) -> np.ndarray:
        """beta per group as it stands now: the ladder on the device (``ReplicaExchange.betas()``), the shared beta without one."""
        eng = self.metropolis.engine
        if self.metropolis.n_rungs:
            return np.asarray(eng.ladder(), dtype=np.float64)
        return np.array([float(eng.beta)], dtype=np.float64)

    def energies(self) -> np.ndarray:
        return reweighting.bin_centres(self.lo, self.hi, self.n_bins)

    def _checked_counts(self) -> np.ndarray:
        counts = self.counts()
        if not counts[:, :self.n_bins].sum():
            raise ValueError("EnergyHistogram: nothing has been accumulated yet")
        share = reweighting.outside_share(counts)
        if self.mask:                           # the fourth cell, "x beyond x_bound", belongs to the same total
            beyond = self.beyond_bound().astype(np.float64)
            total = counts.sum(axis=1).astype(np.float64) + beyond
            with np.errstate(invalid="ignore", divide="ignore"):
                share = np.where(total[:, None] > 0, np.concatenate([counts[:, -3:], beyond[:, None]], axis=1) / total[:, None], 0.0)
        bad = np.argwhere(share > self.max_outside)
        if bad.size:
            g, c = int(bad[0][0]), int(bad[0][1])
            raise ValueError(f"EnergyHistogram: rung {g} has a share of {share[g, c]:.3e} of its samples in the cell '{_CELLS[c]}' "
                             f"(max_outside = {self.max_outside:g}): " +
                             (f"raise x_bound = {self.x_bound:g}" if c == 3 else f"widen [lo, hi) = [{self.lo:g}, {self.hi:g})"))
        return counts

    def _wham(self, tol=1e-12, max_iter=100000):
        counts = self._checked_counts()
        return reweighting.wham(counts[:, :self.n_bins], self.betas(), self.energies(), tol=tol, max_iter=max_iter)

    def _jackknife(self, pick, tol=1e-12, max_iter=100000, with_sums=False):
        """(theta, se) of ``pick(log_g, f)`` (a flat Float64 array): theta from the counts of all blocks -- the bits the call without
        ``error`` gives --, se from the B leave-one-out replicates, each the whole of WHAM on its own counts, started from the full
        solution.  ``with_sums``: ``pick(log_g, f, counts[G, n_bins], sums[G, C, n_bins])`` with the replicate's own counts and moment
        sums (Float64, in the columns' quanta), exact leave-one-out integers both.  The ``max_outside`` check is the total's; a
        replicate that WHAM cannot solve raises, naming the block."""
        if not self.blocks:
            raise ValueError("EnergyHistogram: error=True needs blocks=B (the counts per jackknife block)")
        self._checked_counts()                                          # (the total: the same refusals as without error)
        blocks = self.counts_blocks()
        betas, energies, n = self.betas(), self.energies(), self.n_bins
        total = blocks.sum(axis=0, dtype=np.uint64)
        log_g, f, _ = reweighting.wham(total[:, :n], betas, energies, tol=tol, max_iter=max_iter)
        for b in range(blocks.shape[0]):
            if not blocks[b].any():
                raise ValueError(f"EnergyHistogram: block {b} is empty (fewer chunks of ladders than blocks?)")
            rest = (total - blocks[b])[:, :n]
            if np.any(rest.sum(axis=1) == 0) or not reweighting._connected(rest > 0):
                raise ValueError(f"EnergyHistogram: without block {b} the rungs' histograms no longer connect (a row is empty or shares no "
                                 "bin with the others): the replicate's free energies are undetermined; more snapshots or fewer blocks")
        arrays = [blocks]
        if with_sums:
            arrays.append(self._moment_integers_blocks())
            q = self._quanta()
        first = [True]

        def fn(counts, sums=None):
            more = () if sums is None else (counts[:, :n], sums.astype(np.float64) * q[None, :, None])
            if first[0]:                        # (jackknife_integers gives the total first: the full solution, solved above)
                first[0] = False
                return pick(log_g, f, *more)
            lg, fr, _ = reweighting.wham(counts[:, :n], betas, energies, tol=tol, max_iter=max_iter, f0=f)
            return pick(lg, fr, *more)

        return jackknife.jackknife_integers(arrays, fn)

    def density_of_states(self, error=False, **kw):
        """(energies[n_bins], log_g[n_bins]): the bin centres and the WHAM density of states (-inf where no rung has a count), on the
        normalisation log Z(beta_0) = 0.  ``error=True``: (energies, (log_g, se)), se NaN where a replicate has -inf."""
        if error:
            return self.energies(), self._jackknife(lambda lg, f: lg, **kw)
        return self.energies(), self._wham(**kw)[0]

    def free_energies(self, error=False, **kw):
        """f_r = -log Z(beta_r) + log Z(beta_0) per rung (f_0 = 0).  ``error=True``: (f, se)."""
        if error:
            return self._jackknife(lambda lg, f: f, **kw)
        return self._wham(**kw)[1]

    def reweight(self, betas, error=False, **kw):
        """(log Z, <e>, <e^2>, C) at every beta of ``betas`` (reweighting.reweight), from the ladder as it stands at fetch time.
        ``error=True``: the four as (value, se) pairs, ((log Z, se), (<e>, se), (<e^2>, se), (C, se))."""
        if not error:
            return reweighting.reweight(self._wham(**kw)[0], self.energies(), betas)
        b = np.asarray(betas, dtype=np.float64)
        energies = self.energies()
        theta, se = self._jackknife(lambda lg, f: np.concatenate([np.ravel(v) for v in reweighting.reweight(lg, energies, b)]), **kw)
        return tuple((t.reshape(b.shape), s.reshape(b.shape)) for t, s in zip(np.split(theta, 4), np.split(se, 4)))

    # -- moments per bin ---------------------------------------------------------------------------------------------------------------
    def beyond_bound(self) -> np.ndarray:
        """Per group the chains of ALL ranks that fell into a bin with |x| > x_bound or NaN (uint64[G]): the fourth tail cell."""
        return self._all_ranks(np.ascontiguousarray(self._local_moments()[0][:, self.n_bins + 3]))

    def moment_sums(self) -> np.ndarray:
        """S[G, C, n_bins] (Float64) of ALL ranks: per group, column (``self.moments``, in that order) and bin the sum of the observable
        over the samples of the bin -- the device's integer times the column's quantum.  The signed 64-bit integers travel as the
        two halves of their two's complement, like the counts, and are put together modulo 2^64: exact.  The host waits for the
        queued snapshots."""
        k = self._all_ranks(self._local_moments()[1].view(np.uint64)).view(np.int64)
        return k.astype(np.float64) * self._quanta()[None, :, None]

    def _quanta(self) -> np.ndarray:
        """The quantum of every kept column, in column order."""
        quanta = emom_quanta(self.x_bound)
        return np.array([quanta[MOMENTS[n]] for n in self.moments], dtype=np.float64)

    def _moment_integers_blocks(self) -> np.ndarray:
        """k[B, G, C, n_bins] (int64) of ALL ranks: the device's integer sums per jackknife block, the halves of ``moment_sums``."""
        return self._all_ranks(np.ascontiguousarray(self._local_moments_blocks()[1]).view(np.uint64)).view(np.int64)

    def moment_sums_blocks(self) -> np.ndarray:
        """S[B, G, C, n_bins] (Float64) of ALL ranks per jackknife block: ``moment_sums()`` of the ladders of every block (blocks are
        functions of the global ladder index, so the shards add cell by cell).  Needs ``blocks=B``; the integers behind it sum over B
        to those behind ``moment_sums()``."""
        return self._moment_integers_blocks().astype(np.float64) * self._quanta()[None, None, :, None]

    def microcanonical(self):
        """(energies[n_bins], o[C, n_bins]): the mean of every observable over all samples of a bin, sum_g S_gb / sum_g n_gb; NaN where
        no group has a count."""
        n = self.counts()[:, :self.n_bins].sum(axis=0).astype(np.float64)
        s = self.moment_sums().sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.energies(), np.where(n[None, :] > 0, s / n[None, :], np.nan)

    def reweight_moments(self, betas, error=False, **kw) -> dict:
        """{name: <o>(beta)} for every kept moment ("x", "x2", "pos") at every beta of ``betas`` (reweighting.reweight_observable with
        WHAM's density of states), from the ladder as it stands at fetch time.  ``error=True`` (needs ``blocks=B``): {name: (value,
        se)}, the values those of ``error=False``, se the delete-one-block jackknife: every replicate is the whole of WHAM on its
        leave-one-out counts, followed by reweight_observable with its leave-one-out sums and counts."""
        if not self.mask:
            raise ValueError("EnergyHistogram: the moments per bin need moments=(...) and x_bound")
        if error:
            b = np.asarray(betas, dtype=np.float64)
            energies, C = self.energies(), len(self.moments)

            def pick(lg, f, counts, sums):
                return np.concatenate([np.ravel(reweighting.reweight_observable(lg, energies, b, sums[:, c, :], counts)) for c in range(C)])

            theta, se = self._jackknife(pick, with_sums=True, **kw)
            return {name: (t.reshape(b.shape), e.reshape(b.shape)) for name, t, e in zip(self.moments, np.split(theta, C), np.split(se, C))}
        counts = self._checked_counts()[:, :self.n_bins]
        log_g = reweighting.wham(counts, self.betas(), self.energies(), **kw)[0]
        sums = self.moment_sums()
        return {name: reweighting.reweight_observable(log_g, self.energies(), betas, sums[:, c, :], counts) for c, name in enumerate(self.moments)}

    # -- checkpoints (storage.py's section) -------------------------------------------------------------------------------------------
    def state(self) -> dict:
        if self.mask:                           # (the moments' accumulator holds the counts: state_moments)
            return {}
        counts, n_snap = self._local()
        return dict(ehist_bins=np.array([self.lo, self.hi, float(self.n_bins)], dtype=np.float64), ehist_counts=counts,
                    ehist_snapshots=np.uint64(n_snap))

    def set_state(self, d) -> None:
        lo, hi, n_bins = (float(v) for v in d["ehist_bins"])
        if (lo, hi, int(n_bins)) != (self.lo, self.hi, self.n_bins):
            raise ValueError(f"checkpoint holds energy histograms with the bins {(lo, hi, int(n_bins))}, this EnergyHistogram asks for "
                             f"{(self.lo, self.hi, self.n_bins)}")
        self.metropolis.engine.set_energy_histogram(self.lo, self.hi, self.n_bins, np.asarray(d["ehist_counts"], dtype=np.uint64),
                                                    int(d["ehist_snapshots"]))

    def state_moments(self) -> dict:
        """The moments' accumulator (storage.py's section): the form, the cells and the snapshot count; nothing without moments."""
        if not self.mask:
            return {}
        counts, sums, n_snap = self._local_moments()
        return dict(emom_form=np.array([self.lo, self.hi, float(self.n_bins), float(self.mask), self.x_bound], dtype=np.float64),
                    emom_counts=counts, emom_sums=sums, emom_snapshots=np.uint64(n_snap))

    def set_state_moments(self, d) -> None:
        if "emom_counts" not in d or not self.mask:
            return
        lo, hi, n_bins, mask, x_bound = (float(v) for v in d["emom_form"])
        form, mine = (lo, hi, int(n_bins), int(mask), x_bound), (self.lo, self.hi, self.n_bins, self.mask, self.x_bound)
        if form != mine:
            raise ValueError(f"checkpoint holds moments per bin of the form (lo, hi, n_bins, mask, x_bound) = {form}, this EnergyHistogram "
                             f"asks for {mine}")
        self.metropolis.engine.set_energy_moments(*mine, np.asarray(d["emom_counts"], dtype=np.uint64), np.asarray(d["emom_sums"], dtype=np.int64),
                                                  int(d["emom_snapshots"]))

    def state_blocks(self) -> dict:
        """The counts per block (storage.py's section behind the ladder and the partition); nothing without blocks or snapshots."""
        if self.mask or not self.blocks or self.metropolis.blocks_on != self.blocks:      # (with moments: state_moments_blocks)
            return {}
        counts, n_snap = self._local_blocks()
        if not n_snap:
            return {}
        return dict(ehist_blocks=np.array(self.blocks, dtype=np.int64), ehist_block_counts=counts, ehist_block_snapshots=np.uint64(n_snap))

    def set_state_blocks(self, d) -> None:
        if self.mask:                           # (the moments' accumulator holds the counts: set_state_moments_blocks)
            return
        if "ehist_block_counts" not in d:
            if self.blocks and "ehist_counts" in d and int(d["ehist_snapshots"]):
                raise ValueError("checkpoint holds energy histograms without counts per block, this EnergyHistogram asks for blocks")
            return
        if not self.blocks:                     # (set_state has restored their sum: the run goes on with a plain accumulator)
            return
        if tuple(int(v) for v in d["ehist_blocks"]) != tuple(self.blocks):
            raise ValueError(f"checkpoint holds energy histograms under the partition {tuple(int(v) for v in d['ehist_blocks'])}, this run asks "
                             f"for {tuple(self.blocks)}")
        jackknife.use_blocks(self.metropolis, self.blocks)
        self.metropolis.engine.set_energy_histogram_blocks(self.lo, self.hi, self.n_bins, np.asarray(d["ehist_block_counts"], dtype=np.uint64),
                                                           int(d["ehist_block_snapshots"]))

    def state_moments_blocks(self) -> dict:
        """The moments per block (storage.py's section behind the ladder and the partition): the partition, counts and sums per block
        and the snapshot count; nothing without moments, blocks or snapshots."""
        if not self.mask or not self.blocks or self.metropolis.blocks_on != self.blocks:
            return {}
        counts, sums, n_snap = self._local_moments_blocks()
        if not n_snap:
            return {}
        return dict(emom_blocks=np.array(self.blocks, dtype=np.int64), emom_block_counts=counts, emom_block_sums=sums,
                    emom_block_snapshots=np.uint64(n_snap))

    def set_state_moments_blocks(self, d) -> None:
        if not self.mask:
            return
        if "emom_block_counts" not in d:
            if self.blocks and "emom_counts" in d and int(d["emom_snapshots"]):
                raise ValueError("checkpoint holds moments per bin without cells per block, this EnergyHistogram asks for blocks")
            return
        if not self.blocks:                     # (set_state_moments has restored their sum: the run goes on with a plain accumulator)
            return
        if tuple(int(v) for v in d["emom_blocks"]) != tuple(self.blocks):
            raise ValueError(f"checkpoint holds moments per bin under the partition {tuple(int(v) for v in d['emom_blocks'])}, this run asks "
                             f"for {tuple(self.blocks)}")
        jackknife.use_blocks(self.metropolis, self.blocks)
        self.metropolis.engine.set_energy_moments_blocks(self.lo, self.hi, self.n_bins, self.mask, self.x_bound,
                                                         np.asarray(d["emom_block_counts"], dtype=np.uint64),
                                                         np.asarray(d["emom_block_sums"], dtype=np.int64), int(d["emom_block_snapshots"]))

    def write_algorithm(self, io, scheduler) -> None:
        io.write(f"\tEnergyHistogram\n\t\tCalls: {_calls(scheduler)}\n\t\tBins: {self.n_bins} in [{self.lo}, {self.hi})\n")
        if self.blocks:
            io.write(f"\t\tBlocks: {self.blocks[0]} of chunk {self.blocks[1]}\n")
        if self.mask:
            io.write(f"\t\tMoments: {', '.join(self.moments)} within |x| <= {self.x_bound}\n")


def _find_energy_histogram(simulation: Simulation) -> EnergyHistogram:
    found = [a for a in simulation.algorithms if isinstance(a, EnergyHistogram)]
    if len(found) != 1:
        raise ValueError(f"this callback needs exactly one EnergyHistogram in the algorithm list, found {len(found)}")
    return found[0]


def callback_reweight_error(simulation: Simulation) -> np.ndarray:
    """The jackknife standard errors [4, G] of (log Z, <e>, <e^2>, C) reweighted to the ladder's own betas
    (EnergyHistogram.reweight(betas(), error=True); needs blocks=B).  The host waits for the queued snapshots."""
    eh = _find_energy_histogram(simulation)
    return np.stack([se for _, se in eh.reweight(eh.betas(), error=True)])


def callback_reweight_moments(simulation: Simulation) -> np.ndarray:
    """The kept moments [C, G] (rows in the order of ``EnergyHistogram.moments``) reweighted to the ladder's own betas
    (EnergyHistogram.reweight_moments(betas())).  The host waits for the queued snapshots."""
    eh = _find_energy_histogram(simulation)
    out = eh.reweight_moments(eh.betas())
    return np.stack([out[name] for name in eh.moments])


def callback_reweight_moments_error(simulation: Simulation) -> np.ndarray:
    """The jackknife standard errors [C, G] of the kept moments (rows in the order of ``EnergyHistogram.moments``) reweighted to the
    ladder's own betas (EnergyHistogram.reweight_moments(betas(), error=True); needs blocks=B).  The host waits for the queued
    snapshots."""
    eh = _find_energy_histogram(simulation)
    out = eh.reweight_moments(eh.betas(), error=True)
    return np.stack([out[name][1] for name in eh.moments])
