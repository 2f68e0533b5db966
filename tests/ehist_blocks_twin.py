"""Host twin of the energy histograms per jackknife block (DESIGN.md section 3.17 "Per block"; include/amc.h
amc_energy_histogram_accumulate_blocks), written from that text: ehist_twin's cells (the oracle's energies, the bin rule in numpy
Float64) composed with the block of a ladder,

    b(l) = ((first + l) div C) mod B,     first = chain_offset / G,

chain i being rung i mod G of local ladder i div G.  counts[(b, g, cell)] counts the chains of group g in the ladders of block b.  It
shares no code with the product.
"""
import numpy as np

import ehist_twin as T


def block_of(n_ladders: int, n_blocks: int, chunk: int, first: int = 0) -> np.ndarray:
    """b(l) for the local ladders l < n_ladders of a shard whose ladder 0 is global ladder ``first``."""
    return ((int(first) + np.arange(int(n_ladders), dtype=np.int64)) // int(chunk)) % int(n_blocks)


def ladders(n_ladders: int, n_blocks: int, chunk: int, first: int = 0) -> np.ndarray:
    """Local ladders per block, by counting."""
    return np.bincount(block_of(n_ladders, n_blocks, chunk, first), minlength=int(n_blocks)).astype(np.int64)


def histogram(e, lo, hi, n_bins, n_groups, n_blocks, chunk, first=0) -> np.ndarray:
    """counts[B, G, n_bins + 3] (uint64) of one snapshot of the energies ``e`` (Float64, one per local chain)."""
    G, n, B = int(n_groups), int(n_bins), int(n_blocks)
    c = T.cells(e, lo, hi, n).reshape(-1, G)
    b = block_of(c.shape[0], B, chunk, first)
    out = np.zeros((B, G, n + 3), dtype=np.uint64)
    np.add.at(out, (b[:, None], np.arange(G)[None, :], c), np.uint64(1))
    return out


def snapshot(potential, x, lo, hi, n_bins, n_groups, n_blocks, chunk, first=0, f32=False) -> np.ndarray:
    """counts[B, G, n_bins + 3] of the positions ``x``."""
    return histogram(T.energies(potential, x, f32), lo, hi, n_bins, n_groups, n_blocks, chunk, first)
