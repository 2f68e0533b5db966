"""Host twin of the moments per energy bin per jackknife block (DESIGN.md section 3.17 "Moments per block"; include/amc.h
amc_energy_moments_accumulate_blocks), written from that text: emom_twin's rule per chain (the oracle's energies, the cells and the
deposits in numpy Float64) composed with the block of a ladder (ehist_blocks_twin.block_of),

    b(l) = ((first + l) div C) mod B,     first = chain_offset / G,

chain i being rung i mod G of local ladder i div G.  Block b holds what emom_twin.moments gives for the ladders of block b alone.  It
shares no code with the product.
"""
import numpy as np

import ehist_blocks_twin as KB
import ehist_twin as T
import emom_twin as E


def moments(e, xd, lo, hi, n_bins, mask, x_bound, n_groups, n_blocks, chunk, first=0):
    """(counts[B, G, n_bins + 4] uint64, sums[B, G, C, n_bins] int64) of one snapshot: energies ``e``, positions ``xd``."""
    G, n, B = int(n_groups), int(n_bins), int(n_blocks)
    e = np.asarray(e, dtype=np.float64).reshape(-1, G)
    xd = np.asarray(xd, dtype=np.float64).reshape(-1, G)
    block = KB.block_of(e.shape[0], B, chunk, first)
    cols = bin(int(mask)).count("1")
    counts = np.zeros((B, G, n + 4), dtype=np.uint64)
    sums = np.zeros((B, G, cols, n), dtype=np.int64)
    for b in range(B):
        mine = block == b
        if mine.any():                          # (whole ladders: chain i of the selection is still in group i mod G)
            counts[b], sums[b] = E.moments(e[mine].reshape(-1), xd[mine].reshape(-1), lo, hi, n, mask, x_bound, G)
    return counts, sums


def snapshot(potential, x, lo, hi, n_bins, mask, x_bound, n_groups, n_blocks, chunk, first=0, f32=False):
    """(counts, sums) per block of the positions ``x`` as download_state returns them."""
    return moments(T.energies(potential, x, f32), x, lo, hi, n_bins, mask, x_bound, n_groups, n_blocks, chunk, first)
