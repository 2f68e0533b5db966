"""Device-side stand-ins for the reference's per-chain text I/O, usable at 10^7 chains.

The reference writes one text file per chain (StoreTrajectories src/algorithms.jl:154-210, StoreBackups
:264-303, StoreLastFrames :221-251; row format "$t $(x)", example/particle_1d/particle_1d.jl:63-66) and can
not resume (no loader; RNG state and move counters are not saved).  What those files are consumed for is
served here without 10^7 open files:

  StoreHistogram   pooled-position histogram over the schedule (the density plot of
                   MC_harmonic_oscillator.jl:40-51 and the mean/std check of test/distribution_test.jl:33-37)
  StoreSnapshots   strided binary snapshots x[first::stride] at the scheduled times (a trajectory subset)
  checkpoint / restore   complete, exact resume: positions, per-chain counters, sigma and the two Philox
                   step indices -- the generator is counter-based, so (seed, step) IS the RNG state.
"""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np

from . import sharding
from ._capi import AMC_ANNEAL_MAX_RECORDS
from .metropolis import Metropolis, _check_rung_sigma
from .simulation import AriannaAlgorithm, Simulation, _calls


class StoreHistogram(AriannaAlgorithm):
    """StoreHistogram(chains; dependencies=(Metropolis,), lo, hi, bins, scheduler): accumulates the histogram
    of all chain positions at every scheduled time; `finalise` all-reduces it and rank 0 writes
    `histogram.dat` (bin_lo bin_hi count) plus the pooled mean / std estimated from the bin-free moments."""

    wants_reductions = True

    def __init__(self, chains, dependencies=None, path=None, lo: float = -2.0, hi: float = 2.0, bins: int = 200,
                 **extras):
        assert dependencies is not None and len(dependencies) == 1 and isinstance(dependencies[0], Metropolis)
        self.metropolis: Metropolis = dependencies[0]
        self.lo, self.hi, self.bins = float(lo), float(hi), int(bins)
        self.counts = np.zeros(self.bins + 3, dtype=np.uint64)
        self.moments = np.zeros(3)                 # n, sum x, sum x^2 over all samples (global)
        self.path = os.path.join(path, "histogram.dat")
        self.rank, _ = sharding.world()

    def reduction_needs(self):
        return ("mean_x", "mean_x2")          # the bin-free moments (run() tells the sampler: simulation._declare_reduction_needs)

    def _settle(self) -> None:
        """The moments of the previous sample (a reduction ticket claimed then) are fetched when the next one is due."""
        ticket, self._ticket = getattr(self, "_ticket", None), None
        if ticket is not None:
            r = ticket.result()
            n = r["n_chains"]
            self.moments += np.array([n, r["mean_x"] * n, r["mean_x2"] * n])

    def make_step(self, simulation: Simulation) -> None:
        eng = self.metropolis.engine
        self._settle()
        # The engine keeps ONE running histogram.  The first StoreHistogram of a Metropolis to sample owns it (its counts stay
        # on the device until finalise and its moments are read one sample late: nothing makes the host wait for the queued
        # sweeps); any other instance -- same bins or not -- fetches its counts at each sample time.
        owner = self.metropolis._histogram_owner
        if owner is None and hasattr(eng, "histogram_accumulate"):
            owner = self.metropolis._histogram_owner = self
        on_device = owner is self
        if on_device:
            eng.histogram_accumulate(self.lo, self.hi, self.bins)
            self._on_device = True
        if on_device:
            self._ticket = self.metropolis.reductions_async()
        else:
            self.counts += eng.histogram(self.lo, self.hi, self.bins)
            self._ticket = self.metropolis.reductions_async()
            self._settle()

    def finalise(self, simulation: Simulation) -> None:
        self._settle()
        if getattr(self, "_on_device", False):
            self.counts += self.metropolis.engine.histogram_fetch(self.bins, reset=True)
            self._on_device = False
            self.metropolis._histogram_owner = None
        total = sharding.allreduce_sum(self.counts.astype(np.float64))
        self.global_counts = np.rint(total).astype(np.uint64)
        n, sx, sxx = self.moments
        self.mean = sx / n if n else float("nan")
        self.std = float(np.sqrt(max(sxx / n - self.mean ** 2, 0.0))) if n else float("nan")
        if self.rank == 0:
            os.makedirs(os.path.dirname(self.path), exist_ok=True)
            edges = self.lo + (self.hi - self.lo) * np.arange(self.bins + 1) / self.bins
            with open(self.path, "w") as f:
                f.write(f"# samples {int(n)} mean {self.mean!r} std {self.std!r} below {int(self.global_counts[self.bins])} "
                        f"above {int(self.global_counts[self.bins + 1])} nan {int(self.global_counts[self.bins + 2])}\n")
                for i in range(self.bins):
                    f.write(f"{edges[i]!r} {edges[i + 1]!r} {int(self.global_counts[i])}\n")

    def write_algorithm(self, io, scheduler) -> None:
        io.write(f"\tStoreHistogram\n\t\tCalls: {_calls(scheduler)}\n\t\tRange: [{self.lo}, {self.hi}) in {self.bins} bins\n")


class StoreSnapshots(AriannaAlgorithm):
    """StoreSnapshots(chains; dependencies=(Metropolis,), stride, scheduler): rows (t, x[first::stride]) of this
    rank's shard, kept in memory and written as `snapshots_rank<r>.npy` at finalise (binary trajectory subset)."""

    def __init__(self, chains, dependencies=None, path=None, stride: int = 1000, max_chains: int = 4096,
                 store_first: bool = True, **extras):
        assert dependencies is not None and len(dependencies) == 1 and isinstance(dependencies[0], Metropolis)
        self.metropolis: Metropolis = dependencies[0]
        start, stop = self.metropolis.shard
        self.stride = int(stride)
        first_global = -(-start // self.stride) * self.stride          # first multiple of stride inside the shard
        self.first = first_global - start
        self.count = 0 if self.first >= stop - start else min(int(max_chains), (stop - start - 1 - self.first) // self.stride + 1)
        self.chain_ids = start + self.first + self.stride * np.arange(self.count)
        self.times: List[int] = []
        self.rows: List[np.ndarray] = []
        self.store_first = store_first
        self.rank, _ = sharding.world()
        self.path = os.path.join(path, f"snapshots_rank{self.rank}.npy")

    def initialise(self, simulation: Simulation) -> None:
        if self.store_first:
            self.make_step(simulation)

    def make_step(self, simulation: Simulation) -> None:
        self.times.append(simulation.t)
        self.rows.append(self.metropolis.engine.download_strided(self.first, self.stride, self.count))

    def finalise(self, simulation: Simulation) -> None:
        os.makedirs(os.path.dirname(self.path), exist_ok=True)
        data = np.column_stack([np.array(self.times, dtype=np.float64), np.array(self.rows).reshape(len(self.times), self.count)])
        np.save(self.path, data)
        np.save(self.path.replace(".npy", "_chain_ids.npy"), self.chain_ids)

    def write_algorithm(self, io, scheduler) -> None:
        io.write(f"\tStoreSnapshots\n\t\tCalls: {_calls(scheduler)}\n\t\tChains: every {self.stride}th ({self.count} on rank {self.rank})\n")


# ---- checkpoint / restore: one pair of functions per group of state ------------------------------------------------------
# _write_<group>(met, eng, d, est) puts the group's fields into the dict that becomes the file, _read_<group>(met, eng, d, est) puts
# them back into the Metropolis and its engine.  A group has fields in the file only while its condition holds ("no field without
# one"); its reader's condition is the presence of the field.  _SECTIONS lists the pairs in the order both walk them.
def _write_core(met, eng, d, est) -> None:
    x, _ = eng.download_state(want_e=False)
    start, stop = met.shard
    d.update(x=x, shard=np.array([start, stop]), n_chains_global=len(met.chains), seed=met.seed, sweepstep=met.sweepstep,
             step=eng.step, estimator_step=eng.estimator_step, sigma=np.array([m.sigma for m in met.pool]),
             weight=np.array([m.weight for m in met.pool]), param_dtype=met.param_dtype)
    if met.chains.beta_array is not None:
        d["beta"] = met.chains.beta_array[start:stop]

def _read_core(met, eng, d, est) -> None:
    if list(d["shard"]) != list(met.shard) or int(d["seed"]) != met.seed or int(d["n_chains_global"]) != len(met.chains):
        raise ValueError("checkpoint does not match this Metropolis (shard / seed / ensemble size)")
    saved_pd = str(d["param_dtype"]) if "param_dtype" in d else "f64"
    if saved_pd != met.param_dtype:
        raise ValueError(f"checkpoint was written with param_dtype {saved_pd!r}, this Metropolis has {met.param_dtype!r}: the two run "
                         "different arithmetic (pass the moves' parameters in the checkpoint's type)")
    eng.upload_state(d["x"], d["beta"] if "beta" in d else None)
    for k, s in enumerate(d["sigma"]):
        met.set_parameters(k, [float(s)])
    eng.step = int(d["step"])
    eng.estimator_step = int(d["estimator_step"])


def _write_counters(met, eng, d, est) -> None:
    acc_tot, tot_tot = eng.counter_totals()
    d.update(accepted_total=acc_tot, total_total=tot_tot)
    try:
        acc, tot = eng.download_counters()
        d.update(accepted=acc, total=tot)
    except Exception:
        pass                                        # pool-wide counter mode: the totals are the state

def _read_counters(met, eng, d, est) -> None:
    if "accepted" in d:
        eng.upload_counters(d["accepted"], d["total"])
    else:
        eng.set_counter_totals(int(d["accepted_total"][0]), int(d["total_total"][0]) // (met.shard[1] - met.shard[0]))


def _write_rung_sigma(met, eng, d, est) -> None:
    if met.n_rungs and met.rung_sigma is not None:  # widths per rung: the table is state (no field without one)
        if hasattr(eng, "rung_sigma"):              # ... as the device holds it: a tuned table is the tuned one
            met.rung_sigma = np.array(eng.rung_sigma(), dtype=np.float64)
        d["rung_sigma"] = np.asarray(met.rung_sigma, dtype=np.float64)

def _read_rung_sigma(met, eng, d, est) -> None:
    if "n_rungs" in d:                              # (a ladder without the field: no table)
        tab = None
        if "rung_sigma" in d:                       # widths per rung: checked like the constructor's against this pool and ladder
            tab = _check_rung_sigma(d["rung_sigma"], met.pool, 1)
            if tab.shape[1] != int(d["n_rungs"]):
                raise ValueError(f"checkpoint holds rung_sigma of {tab.shape[1]} rungs per move for a ladder of R = {int(d['n_rungs'])}")
        met.rung_sigma = tab                        # the checkpoint's table, or none, replaces the constructor's; _read_ladder hands it on


def _write_ladder(met, eng, d, est) -> None:
    if met.n_rungs:                                 # a temperature ladder: the exchange step index and the gap counters are state
        acc_x, att_x = eng.exchange_counters()
        d.update(n_rungs=met.n_rungs, exchange_step=eng.exchange_step, exchange_accepted=acc_x, exchange_attempted=att_x)

def _read_ladder(met, eng, d, est) -> None:
    if "n_rungs" in d:
        met.set_ladder(int(d["n_rungs"]))
        # set_ladder does nothing where the ladder is set already, so the table goes to the engine here: what the engine sweeps
        # with is what the next checkpoint writes
        if met.rung_sigma is not None or hasattr(eng, "set_rung_sigma"):
            eng.set_rung_sigma(met.rung_sigma)
        eng.exchange_step = int(d["exchange_step"])
        eng.set_exchange_counters(d["exchange_accepted"], d["exchange_attempted"])


def _write_tracking(met, eng, d, est) -> None:
    if met.n_rungs and met.tracking:                # walker tracking is on: the labels and the trip counters are state too
        walker, direction = eng.labels()
        d.update(walker=walker, direction=direction, trips=np.array(eng.tracking_counters(), dtype=np.int64))

def _read_tracking(met, eng, d, est) -> None:
    if "walker" in d:
        eng.set_tracking(True)                      # (labels start as the identity; the checkpoint's replace them)
        eng.set_labels(d["walker"], d["direction"])
        eng.set_tracking_counters(int(d["trips"][0]), int(d["trips"][1]))
        met.tracking = True


def _write_window(met, eng, d, est) -> None:
    if met.n_rungs and met._rung_window_used:       # a tuning or a window restart has happened: the window's base and the count
        base_acc, base_tot = eng.rung_window_base()     # of tunings are state (no field otherwise)
        d.update(rung_window_accepted=base_acc, rung_window_total=base_tot)
        if met.rung_sigma is not None:
            d["n_tuned"] = eng.tune_status()[1]

def _read_window(met, eng, d, est) -> None:
    if "rung_window_accepted" in d:                 # the window of the acceptance per rung, and the count of tunings
        eng.set_rung_window_base(d["rung_window_accepted"], d["rung_window_total"])
        if "n_tuned" in d and met.rung_sigma is not None:
            eng.set_tuned(int(d["n_tuned"]))
        met._rung_window_used = True


def _write_bridge(met, eng, d, est) -> None:
    if met.n_rungs and met.bridge:                  # the bridge sums are on: the accumulator is state (no field otherwise)
        rec, n_snap = eng.bridge_fetch(reset=False)
        d.update(bridge_records=rec, bridge_columns=int(met.bridge), bridge_snapshots=n_snap)

def _read_bridge(met, eng, d, est) -> None:
    if "bridge_records" in d:                       # (read whenever it is there: the resumed run accumulates on to the same bits)
        if met.bridge and int(d["bridge_columns"]) != int(met.bridge):
            raise ValueError(f"checkpoint holds bridge sums of columns {int(d['bridge_columns'])}, this ReplicaExchange asks for "
                             f"{int(met.bridge)}")
        eng.set_bridge(d["bridge_records"], int(d["bridge_snapshots"]))


def _write_bridge_blocks(met, eng, d, est) -> None:
    if met.n_rungs and met.bridge and met.blocks_on:    # a jackknife partition: the records per block are the state the run goes on from
        rec, n_snap = eng.bridge_fetch_blocks(reset=False)
        d.update(bridge_blocks=np.array(met.blocks_on, dtype=np.int64), bridge_block_records=rec, bridge_block_snapshots=n_snap)

def _read_bridge_blocks(met, eng, d, est) -> None:
    # behind _read_bridge: setting the partition clears the plain accumulator that section filled, and this one fills the blocks
    if "bridge_block_records" in d and met.blocks:
        from . import jackknife
        if tuple(int(v) for v in d["bridge_blocks"]) != tuple(met.blocks):
            raise ValueError(f"checkpoint holds bridge sums under the partition {tuple(int(v) for v in d['bridge_blocks'])}, this run asks "
                             f"for {tuple(met.blocks)}")
        jackknife.use_blocks(met, met.blocks)
        eng.set_bridge_blocks(d["bridge_block_records"], int(d["bridge_block_snapshots"]))
    elif "bridge_records" in d and met.bridge and met.blocks and int(d["bridge_snapshots"]):
        raise ValueError("checkpoint holds bridge sums without sums per block, this ReplicaExchange asks for blocks")


def _write_respacing(met, eng, d, est) -> None:
    n_respaced = eng.respace_status()[1] if met.n_rungs and hasattr(eng, "respace_status") else 0
    if n_respaced:                                  # the ladder was respaced (ReplicaExchange.respace keeps beta_array current): no field otherwise
        d["n_respaced"] = n_respaced

def _read_respacing(met, eng, d, est) -> None:
    if "n_respaced" in d:                           # a respaced ladder: the host copy follows the checkpoint's beta, as the engine did
        eng.set_respaced(int(d["n_respaced"]))
        met.chains.beta_array[met.shard[0]:met.shard[1]] = d["beta"]


def _write_annealing(met, eng, d, est) -> None:
    pa = met.annealing
    if pa is not None:                              # population annealing: beta, the step index, the records and the families are state
        d.update(anneal_beta=float(eng.beta), anneal_step=int(eng.anneal_step), anneal_records=pa.records())
        blk = pa.block_records() if pa.blocks is not None else None      # (drained with the records, while both logs are aligned)
        eng.set_anneal_records(d["anneal_records"][-AMC_ANNEAL_MAX_RECORDS:])      # (records() drained the engine's log: the run goes on with it)
        pa._records = list(d["anneal_records"][:-AMC_ANNEAL_MAX_RECORDS])
        if pa.families:
            d["families"] = eng.download_families()
        if pa.blocks is not None:                   # blocks=B: the partition and the block records beside the records (no field otherwise)
            d.update(anneal_blocks=np.array(pa.blocks, dtype=np.int64), anneal_block_records=blk)
            eng.set_anneal_block_records(blk[-AMC_ANNEAL_MAX_RECORDS:])
            pa._block_records = list(blk[:-AMC_ANNEAL_MAX_RECORDS])
        d.update(pa.histogram_state())              # energy_histogram=...: a histogram per temperature so far (no field otherwise)

def _read_annealing(met, eng, d, est) -> None:
    if "anneal_beta" in d:                          # population annealing: the resumed run anneals on to the same bits
        rec = np.asarray(d["anneal_records"], dtype=np.uint64).reshape(-1, 8)
        eng.beta = met.chains.beta = float(d["anneal_beta"])
        eng.anneal_step = int(d["anneal_step"])
        eng.set_anneal_records(rec[-AMC_ANNEAL_MAX_RECORDS:])
        if met.annealing is not None:
            met.annealing._records = list(rec[:-AMC_ANNEAL_MAX_RECORDS])
            met.annealing.set_histogram_state(d)
        if "families" in d:
            eng.set_anneal_families(True)
            eng.upload_families(d["families"])
            met.families_restored = True
        pa = met.annealing
        if pa is not None and pa.blocks is None and "anneal_blocks" in d:
            raise ValueError(f"checkpoint holds block records under the partition {tuple(int(v) for v in d['anneal_blocks'])}, this "
                             "PopulationAnnealing asks for no blocks: they would be dropped")
        if pa is not None and pa.blocks is not None:      # behind the families: the partition needs them
            if "anneal_blocks" not in d:
                if len(rec):
                    raise ValueError("checkpoint holds annealing records without block records, this PopulationAnnealing asks for blocks")
            else:
                if tuple(int(v) for v in d["anneal_blocks"]) != tuple(pa.blocks):
                    raise ValueError(f"checkpoint holds block records under the partition {tuple(int(v) for v in d['anneal_blocks'])}, this "
                                     f"PopulationAnnealing asks for {tuple(pa.blocks)}")
                blk = np.asarray(d["anneal_block_records"], dtype=np.uint64).reshape(-1, 2, pa.blocks[0])
                eng.set_anneal_blocks(*pa.blocks)
                eng.set_anneal_block_records(blk[-AMC_ANNEAL_MAX_RECORDS:])
                pa._block_records = list(blk[:-AMC_ANNEAL_MAX_RECORDS])
                met.anneal_blocks_restored = True


def _write_correlation(met, eng, d, est) -> None:
    ac = met.autocorrelation
    if ac is not None:                              # a time correlation: the observable, the mark with its origin values, records and steps,
        d.update(ac.state())                        # and the host accumulator with its origin count are state (no field otherwise)

def _read_correlation(met, eng, d, est) -> None:
    if "corr_observable" in d and met.autocorrelation is not None:      # behind the core: upload_state has cleared the engine's mark
        met.autocorrelation.set_state(d)


def _write_correlation_blocks(met, eng, d, est) -> None:
    if met.autocorrelation is not None:
        d.update(met.autocorrelation.state_blocks())

def _read_correlation_blocks(met, eng, d, est) -> None:
    if met.autocorrelation is not None:
        met.autocorrelation.set_state_blocks(d)


def _write_convergence(met, eng, d, est) -> None:
    cv = met.convergence
    if cv is not None:                              # convergence per group: the observable, the counts, the sums per chain and the
        d.update(cv.state())                        # algorithm's phase are state (no field otherwise)

def _read_convergence(met, eng, d, est) -> None:
    if "conv_observable" in d and met.convergence is not None:      # behind the core and the ladder: both clear the engine's sums
        met.convergence.set_state(d)


def _write_energy_histogram(met, eng, d, est) -> None:
    eh = met.energy_histogram
    if eh is not None:                              # energy histograms: the bins, the counts and the snapshot count are state (no field otherwise)
        d.update(eh.state())

def _read_energy_histogram(met, eng, d, est) -> None:
    if "ehist_counts" in d and met.energy_histogram is not None:      # behind the ladder: set_ladder clears the engine's accumulator
        met.energy_histogram.set_state(d)


def _write_energy_moments(met, eng, d, est) -> None:
    if met.energy_histogram is not None:            # moments=...: the form, the counts, the sums per bin and the snapshot count (no field otherwise)
        d.update(met.energy_histogram.state_moments())

def _read_energy_moments(met, eng, d, est) -> None:
    if "emom_counts" in d and met.energy_histogram is not None:      # behind the ladder: set_ladder clears the engine's accumulator
        met.energy_histogram.set_state_moments(d)


def _write_energy_histogram_blocks(met, eng, d, est) -> None:
    if met.energy_histogram is not None:            # blocks=B: the counts per jackknife block are the state the run goes on from
        d.update(met.energy_histogram.state_blocks())

def _read_energy_histogram_blocks(met, eng, d, est) -> None:
    # behind _read_energy_histogram (which restored the sum over the blocks), the ladder and the sections that set the partition
    if met.energy_histogram is not None:
        met.energy_histogram.set_state_blocks(d)


def _write_energy_moments_blocks(met, eng, d, est) -> None:
    if met.energy_histogram is not None:            # moments=... with blocks=B: the cells per jackknife block (no field otherwise)
        d.update(met.energy_histogram.state_moments_blocks())

def _read_energy_moments_blocks(met, eng, d, est) -> None:
    # behind _read_energy_moments (which restored the sum over the blocks), the ladder and the sections that set the partition
    if met.energy_histogram is not None:
        met.energy_histogram.set_state_moments_blocks(d)


def _write_estimator(met, eng, d, est) -> None:
    if est is not None:
        d["gd"] = np.array([[g.j, g.grad_j[0], g.grad_logq_forward[0], g.g[0, 0], g.n] for g in est.gradients_data])

def _read_estimator(met, eng, d, est) -> None:
    if est is not None and "gd" in d:
        from .policy_guided import GradientData
        est.gradients_data = [GradientData(float(r[0]), np.array([r[1]]), np.array([r[2]]), np.array([[r[3]]]), int(r[4])) for r in d["gd"]]
        if est.device_resident and est.learn_ids:
            # the running sums live in the engine (amc_pg_accumulate adds to them there): without this the first update
            # after the resume would average the post-resume samples only
            if hasattr(eng, "pg_set_accumulated"):
                eng.pg_set_accumulated(est.learn_ids, np.asarray(d["gd"], dtype=np.float64))
            elif any(int(r[4]) != 0 for r in d["gd"]):
                raise ValueError("restore: this engine cannot take over non-empty device-resident gradients_data")


# The order is restore's, the engine calls depend on it: the table is checked before the ladder is set and goes to the engine behind it;
# the ladder comes before everything kept per rung (labels, window, bridge records, the time correlation's groups); the window's base
# before the count of tunings.
_SECTIONS = ((_write_core, _read_core), (_write_counters, _read_counters), (_write_rung_sigma, _read_rung_sigma),
             (_write_ladder, _read_ladder), (_write_tracking, _read_tracking), (_write_window, _read_window),
             (_write_bridge, _read_bridge), (_write_bridge_blocks, _read_bridge_blocks), (_write_respacing, _read_respacing),
             (_write_annealing, _read_annealing), (_write_correlation, _read_correlation),
             (_write_correlation_blocks, _read_correlation_blocks), (_write_convergence, _read_convergence),
             (_write_energy_histogram, _read_energy_histogram), (_write_energy_moments, _read_energy_moments),
             (_write_energy_histogram_blocks, _read_energy_histogram_blocks), (_write_energy_moments_blocks, _read_energy_moments_blocks),
             (_write_estimator, _read_estimator))


def checkpoint(metropolis: Metropolis, path: str, estimator=None) -> str:
    """Write this rank's shard so that `restore` continues the run bit for bit."""
    if metropolis.device_params_dirty:
        metropolis.pull_parameters()
    if estimator is not None:
        estimator.refresh()
    data = {}
    for write, _ in _SECTIONS:
        write(metropolis, metropolis.engine, data, estimator)
    os.makedirs(path, exist_ok=True)
    fn = os.path.join(path, f"checkpoint_rank{metropolis.rank}.npz")
    np.savez(fn, **data)
    return fn


def restore(metropolis: Metropolis, path: str, estimator=None) -> None:
    """Load `checkpoint`'s file into a freshly constructed Metropolis with the same pool/seed/sharding."""
    d = np.load(os.path.join(path, f"checkpoint_rank{metropolis.rank}.npz"))
    for _, read in _SECTIONS:
        read(metropolis, metropolis.engine, d, estimator)
    metropolis.chains.x = None                      # initialise() must not overwrite the restored state
    metropolis.restored = True
    metropolis.invalidate_reductions()
