"""Delete-one-block jackknife over the blocks of a partition (HipEngine.set_blocks).

The ladders of an ensemble -- the chains, where there is no ladder -- are independent systems, so the B blocks of a partition are
independent too, whatever the correlation in time or between the rungs of one ladder.  For any function theta = fn(sums) of the
reproducible sums the engine keeps per block, the jackknife gives a standard error from the B leave-one-out replicates

    theta_(b) = fn(total without block b),     se^2 = (B - 1) / B * sum_b (theta_(b) - mean_b theta_(b))^2.

The leave-one-out totals are exact: records are merged as integers (xsum_merge), never subtracted as Float64s.
"""
import numpy as np

from ._capi import AMC_MAX_JK_BLOCKS, AMC_XSUM_WORDS, xsum_merge, xsum_round

__all__ = ["anneal_log_z", "block_counts", "check_blocks", "default_chunk", "jackknife", "jackknife_counts", "jackknife_integers", "leave_one_out",
           "leave_one_out_integers", "use_blocks"]


def default_chunk(n_groups: int) -> int:
    """The chunk amc_set_blocks takes for chunk = 0: one block-width of contiguous chains."""
    return max(1, 256 // max(int(n_groups), 1))


def block_counts(n_ladders: int, n_blocks: int, chunk: int, first: int = 0) -> np.ndarray:
    """Ladders per block of the ``n_ladders`` ladders that begin at global ladder ``first``, block of ladder l = (l div chunk) mod
    n_blocks, in closed form: a whole period of n_blocks * chunk ladders gives every block ``chunk``, the cut periods the rest."""
    B, C = int(n_blocks), int(chunk)
    if B < 1 or C < 1 or n_ladders < 0 or first < 0:
        raise ValueError(f"block_counts: n_ladders = {n_ladders}, n_blocks = {n_blocks}, chunk = {chunk}, first = {first}")

    def below(g):                                    # ladders of each block among the global ladders [0, g)
        whole, rest = divmod(int(g), B * C)
        return whole * C + np.clip(rest - np.arange(B, dtype=np.int64) * C, 0, C)

    return below(int(first) + int(n_ladders)) - below(first)


def check_blocks(who: str, blocks, chunk, n_ladders: int, n_groups: int):
    """``blocks=`` / ``block_chunk=`` of an algorithm as the partition (B, C), None without one.  A ValueError where B lies outside
    [2, AMC_MAX_JK_BLOCKS], C < 1, or the ``n_ladders`` ladders make fewer chunks than blocks (a block would be empty)."""
    if blocks is None or blocks is False:
        if chunk is not None:
            raise ValueError(f"{who}: block_chunk = {chunk!r} without blocks")
        return None
    if int(blocks) != blocks or not 2 <= int(blocks) <= AMC_MAX_JK_BLOCKS:
        raise ValueError(f"{who}: blocks = {blocks!r} must be an integer in [2, {AMC_MAX_JK_BLOCKS}]")
    C = default_chunk(n_groups) if chunk is None else chunk
    if int(C) != C or int(C) < 1:
        raise ValueError(f"{who}: block_chunk = {chunk!r} must be an integer >= 1")
    B, C = int(blocks), int(C)
    n_chunks = -(-int(n_ladders) // C)
    if B > n_chunks:
        raise ValueError(f"{who}: blocks = {B} is larger than the {n_chunks} chunks that {n_ladders} ladders make in chunks of {C}: "
                         "a jackknife block would be empty (fewer blocks, or a smaller block_chunk)")
    return B, C


def ask_blocks(who: str, metropolis, partition) -> None:
    """``metropolis.blocks`` = the partition an algorithm asks for; the engine keeps one, so a second algorithm asks for the same."""
    if metropolis.blocks is not None and tuple(metropolis.blocks) != tuple(partition):
        raise ValueError(f"{who}: blocks and chunk {tuple(partition)}, another algorithm of this Metropolis asks for {tuple(metropolis.blocks)}: "
                         "the engine keeps its sums under one partition")
    metropolis.blocks = tuple(partition)


def refuse_annealing(who: str, simulation) -> None:
    """Blocks of ladders stop being independent once a resampling lets copies of one parent share them."""
    from .annealing import PopulationAnnealing
    if any(isinstance(a, PopulationAnnealing) for a in simulation.algorithms):
        raise ValueError(f"{who}: blocks together with a PopulationAnnealing in the algorithm list: resampling makes copies of one parent "
                         "share blocks, so a jackknife over them has no meaning")


def use_blocks(metropolis, partition) -> None:
    """The partition (B, C) on the Metropolis' engine, once: setting it again would clear the sums (storage.restore sets it first, two
    algorithms may share it).  Behind set_ladder, which turns a partition off."""
    if metropolis.blocks_on == tuple(partition):
        return
    if metropolis.blocks_on is not None:
        raise ValueError(f"blocks: the engine keeps its sums under the partition {metropolis.blocks_on}, {tuple(partition)} is asked for "
                         "(one partition per Metropolis: give every algorithm and the checkpoint the same blocks and chunk)")
    if not hasattr(metropolis.engine, "set_blocks"):
        raise ValueError("blocks: this engine keeps no sums per block (streams > 1 is not supported)")
    metropolis.engine.set_blocks(*partition)
    metropolis.blocks_on = tuple(partition)


def _merge(a, b):
    """Records merged record by record; an all-zero record (a slot without a summand) merges as nothing."""
    if a is None:
        return b.copy()
    out = a.copy()
    za, zb = ~a.any(axis=1), ~b.any(axis=1)
    both = ~za & ~zb
    if both.any():
        out[both] = xsum_merge(a[both], b[both])
    out[za] = b[za]
    return out


def leave_one_out(block_records):
    """(total, [total without block b for every b]) of ``block_records[B][...][AMC_XSUM_WORDS]``, every one an exact merge (prefix and
    suffix merges: 3 B of them)."""
    rec = np.ascontiguousarray(block_records, dtype=np.float64)
    B, shape = rec.shape[0], rec.shape[1:]
    flat = rec.reshape(B, -1, AMC_XSUM_WORDS)
    prefix, suffix = [None] * (B + 1), [None] * (B + 1)       # prefix[b]: blocks < b; suffix[b]: blocks >= b
    for b in range(B):
        prefix[b + 1] = _merge(prefix[b], flat[b])
    for b in range(B - 1, -1, -1):
        suffix[b] = _merge(suffix[b + 1], flat[b])
    loo = []
    for b in range(B):
        if prefix[b] is None:
            loo.append(suffix[b + 1].copy())
        elif suffix[b + 1] is None:
            loo.append(prefix[b].copy())
        else:
            loo.append(_merge(prefix[b], suffix[b + 1]))
    return prefix[B].reshape(shape), [r.reshape(shape) for r in loo]


def jackknife(block_records, counts, fn):
    """(theta, se) of ``theta = fn(values, n)``: ``values`` the Float64s of merged records, shaped as one block's records without
    the last axis, ``n`` the ladders merged.  ``block_records[B][...][AMC_XSUM_WORDS]``: the records per block (bridge_fetch_blocks,
    one sample or all of corr_fetch_blocks); ``counts[B]``: the ladders of each block (block_counts) -- they may differ.  theta comes
    from the full merge, se from the B leave-one-out replicates, each the whole of ``fn``.  An empty block is a ValueError."""
    rec = np.ascontiguousarray(block_records, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.int64)
    if rec.ndim < 2 or rec.shape[-1] != AMC_XSUM_WORDS or rec.shape[0] != counts.size:
        raise ValueError(f"jackknife: records of shape {rec.shape} for {counts.size} blocks")
    B = counts.size
    if B < 2:
        raise ValueError(f"jackknife: {B} block(s); a jackknife needs at least 2")
    for b in range(B):
        if counts[b] <= 0:
            raise ValueError(f"jackknife: block {b} is empty (fewer chunks of ladders than blocks?)")
    total, loo = leave_one_out(rec)
    n = int(counts.sum())
    shape = rec.shape[1:-1]
    theta = np.asarray(fn(xsum_round(total).reshape(shape), n), dtype=np.float64)
    reps = np.stack([np.asarray(fn(xsum_round(loo[b]).reshape(shape), n - int(counts[b])), dtype=np.float64) for b in range(B)])
    dev = reps - reps.mean(axis=0)
    se = np.sqrt((B - 1) / B * (dev * dev).sum(axis=0))
    return theta, se


def jackknife_counts(block_counts, fn):
    """(theta, se) of ``theta = fn(counts)`` for integer counts kept per block: ``block_counts[B, ...]`` uint64 (the energy histograms
    of energy_histogram_fetch_blocks).  theta comes from the exact uint64 total, the B replicates from total - block b -- exact too: a
    block's counts are part of the total, so the difference neither wraps nor rounds --, each the whole of ``fn``; se by the formula
    of ``jackknife``.  A ValueError for B < 2 and for a block whose counts are all zero."""
    c = np.ascontiguousarray(block_counts)
    if c.dtype != np.uint64:
        raise ValueError(f"jackknife_counts: counts of dtype {c.dtype}; the exact leave-one-out totals need uint64")
    if c.ndim < 1:
        raise ValueError(f"jackknife_counts: counts of shape {c.shape}; need [B, ...]")
    B = c.shape[0]
    if B < 2:
        raise ValueError(f"jackknife_counts: {B} block(s); a jackknife needs at least 2")
    for b in range(B):
        if not c[b].any():
            raise ValueError(f"jackknife_counts: block {b} is empty (fewer chunks of ladders than blocks?)")
    total = c.sum(axis=0, dtype=np.uint64)
    theta = np.asarray(fn(total), dtype=np.float64)
    reps = np.stack([np.asarray(fn(total - c[b]), dtype=np.float64) for b in range(B)])
    # (an entry that is not finite in some replicate -- log g of a bin only one block filled -- has the se NaN, and no other entry)
    with np.errstate(invalid="ignore"):
        dev = reps - reps.mean(axis=0)
        se = np.sqrt((B - 1) / B * (dev * dev).sum(axis=0))
    return theta, se


def leave_one_out_integers(block_arrays):
    """(totals, [totals without block b for every b]) of several integer arrays kept per block at once: ``block_arrays`` is a sequence
    of arrays [B, ...], each uint64 (counts) or int64 (signed sums), all with the same B.  Every total and every difference is an
    exact integer: a uint64 block is part of its total, so the difference neither wraps nor rounds; int64 sums are added and
    subtracted modulo 2^64, which is exact wherever the true results fit 64 bits, as the engine's cells do.  A ValueError for another
    dtype, for B < 2 and for a block in which every array is zero."""
    arrays = [np.ascontiguousarray(a) for a in block_arrays]
    if not arrays:
        raise ValueError("leave_one_out_integers: no arrays")
    for a in arrays:
        if a.dtype not in (np.uint64, np.int64):
            raise ValueError(f"leave_one_out_integers: an array of dtype {a.dtype}; the exact leave-one-out totals need uint64 or int64")
        if a.ndim < 1 or a.shape[0] != arrays[0].shape[0]:
            raise ValueError(f"leave_one_out_integers: arrays of shapes {[x.shape for x in arrays]}; need [B, ...] with one B")
    B = arrays[0].shape[0]
    if B < 2:
        raise ValueError(f"leave_one_out_integers: {B} block(s); a jackknife needs at least 2")
    for b in range(B):
        if not any(a[b].any() for a in arrays):
            raise ValueError(f"leave_one_out_integers: block {b} is empty (fewer chunks of ladders than blocks?)")
    with np.errstate(over="ignore"):
        totals = tuple(a.sum(axis=0, dtype=a.dtype) for a in arrays)
        loo = [tuple(t - a[b] for t, a in zip(totals, arrays)) for b in range(B)]
    return totals, loo


def jackknife_integers(block_arrays, fn):
    """(theta, se) of ``theta = fn(*totals)`` for several integer arrays kept per block that belong together -- the counts (uint64) and
    the sums per bin (int64) of energy_moments_fetch_blocks: ``jackknife_counts`` for more than one array.  theta comes from the exact
    totals (``fn`` sees them first), the B replicates from ``leave_one_out_integers``, each the whole of ``fn``; se by the formula of
    ``jackknife``, NaN where a replicate is not finite."""
    totals, loo = leave_one_out_integers(block_arrays)
    B = len(loo)
    theta = np.asarray(fn(*totals), dtype=np.float64)
    reps = np.stack([np.asarray(fn(*loo[b]), dtype=np.float64) for b in range(B)])
    with np.errstate(invalid="ignore"):
        dev = reps - reps.mean(axis=0)
        se = np.sqrt((B - 1) / B * (dev * dev).sum(axis=0))
    return theta, se


def anneal_log_z(records, block_records, n_chains: int, cumulative: bool = True):
    """(value[S], se[S], replicates[S, B]) of population annealing's log Z over blocks of FAMILIES (DESIGN.md section 3.14 "Error
    bars"; HipEngine.set_anneal_blocks).  ``records[S, 8]`` are the steps' records, ``block_records[S, 2, B]`` the block records beside
    them: n_b, the chains of block b before the resampling, and T_b, the sum of their integer weights.  The term of step s is
    a_max + log T_w - log M - 30 log 2; replicate b, the same without block b, is a_max + log(T_w - T_b) - log(M - n_b) - 30 log 2 --
    exact integer differences.  cumulative: value and replicates are the running sums over the steps (log Z(beta_s) / Z(beta_0): the
    replicate of the SUM, not a sum of per-step errors); otherwise per step.  se^2 = (B' - 1) / B' sum (theta_b - mean theta_b)^2 over
    the B' blocks that held a family at the first step (n_b > 0 there: a block that was empty from the start is no replicate, one that
    dies out later stays one).  A replicate whose argument is 0 -- block b holds every chain, or all the weight -- is NaN, in the
    cumulative form from that step on, and so is the se there; a step that did not resample (status != 0) is NaN as in log_z_ratios.
    Fewer than two blocks with a family: se is NaN."""
    import math
    rec = np.asarray(records, dtype=np.uint64).reshape(-1, 8)
    blk = np.asarray(block_records, dtype=np.uint64)
    if blk.ndim != 3 or blk.shape[1] != 2 or blk.shape[0] != rec.shape[0]:
        raise ValueError(f"anneal_log_z: {rec.shape[0]} records beside block records of shape {blk.shape} (one [2, B] per record)")
    S, B, M = rec.shape[0], blk.shape[2], int(n_chains)
    shift = 30 * math.log(2.0)
    value, rep = np.full(S, math.nan), np.full((S, B), math.nan)
    for s in range(S):
        status, t_w = int(rec[s, 0]), int(rec[s, 4])
        if sum(int(v) for v in blk[s, 0]) != M or (status == 0 and sum(int(v) for v in blk[s, 1]) != t_w):
            raise ValueError(f"anneal_log_z: the block record of step {s} does not add up to its record (sum n_b = M, sum T_b = T_w)")
        if status != 0:
            continue
        a_max = float(np.array(rec[s, 3], dtype=np.uint64).view(np.float64))
        value[s] = a_max + math.log(t_w) - math.log(M) - shift
        for b in range(B):
            t, n = t_w - int(blk[s, 1, b]), M - int(blk[s, 0, b])
            if t > 0 and n > 0:
                rep[s, b] = a_max + math.log(t) - math.log(n) - shift
    if cumulative:
        value, rep = np.cumsum(value), np.cumsum(rep, axis=0)
    se = np.full(S, math.nan)
    if S:
        alive = blk[0, 0] > 0
        k = int(alive.sum())
        if k >= 2:
            th = rep[:, alive]
            se = np.sqrt((k - 1) / k * ((th - th.mean(axis=1, keepdims=True)) ** 2).sum(axis=1))
    return value, se, rep
