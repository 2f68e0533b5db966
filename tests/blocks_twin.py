"""Host twin of the jackknife blocks (include/amc.h amc_set_blocks .. amc_corr_fetch_blocks): the partition as
a numpy mask over the twins of the bridge sums and the time correlation (bridge_twin.py, corr_twin.py), written from the text and
sharing no code with the product.

The block of local ladder l is ((first + l) div C) mod B, first = chain_offset / G the global index of local ladder 0; a ladder is one
chain where there is no ladder (G = 1).  A block's record is oracle_lib.xsum_r over the summands of ITS ladders alone; a block without
a local ladder has all-zero records.
"""
import numpy as np

import oracle_lib as O

import bridge_twin as BT
import corr_twin as CT

WORDS = O.XS_WORDS


def block_of(n_ladders: int, n_blocks: int, chunk: int, first: int = 0) -> np.ndarray:
    """The block of every local ladder (Python integers underneath: no 64-bit wrap to think about)."""
    return np.array([((int(first) + l) // int(chunk)) % int(n_blocks) for l in range(int(n_ladders))], dtype=np.int64)


def counts(n_ladders: int, n_blocks: int, chunk: int, first: int = 0) -> np.ndarray:
    return np.bincount(block_of(n_ladders, n_blocks, chunk, first), minlength=int(n_blocks))


def bridge_records(e, beta, n_rungs: int, n_blocks: int, chunk: int, columns: int = BT.ALL, f32: bool = False, first: int = 0) -> np.ndarray:
    """records[B][R][6][12] of one snapshot of whole ladders."""
    R = int(n_rungs)
    cols = BT.summands(e, beta, R, f32)
    blk = block_of(cols[0].shape[0], n_blocks, chunk, first)
    out = np.zeros((int(n_blocks), R, BT.COLS, WORDS))
    for b in range(int(n_blocks)):
        m = blk == b
        if not m.any():
            continue
        for r in range(R):
            for c in range(BT.COLS):
                if (columns >> c) & 1 and BT.has_summand(c, r, R):
                    out[b, r, c] = O.xsum_r(np.ascontiguousarray(cols[c][m, r]))
    return out


def corr_records(series, n_groups: int, n_blocks: int, chunk: int, first: int = 0) -> np.ndarray:
    """records[B][S][G][3][12] of a mark (series[0]) and its samples."""
    G = int(n_groups)
    a = np.asarray(series[0], dtype=np.float64).reshape(-1, G)
    blk = block_of(a.shape[0], n_blocks, chunk, first)
    out = np.zeros((int(n_blocks), len(series), G, CT.COLS, WORDS))
    for b in range(int(n_blocks)):
        m = blk == b
        if not m.any():
            continue
        for s, o in enumerate(series):
            o = np.asarray(o, dtype=np.float64).reshape(-1, G)
            out[b, s] = CT.sample_records(a[m].reshape(-1), o[m].reshape(-1), G)
    return out


def merge_blocks(block_records) -> np.ndarray:
    """The merge over the blocks, record by record; an all-zero record merges as nothing (bridge_twin.merge)."""
    return BT.merge(list(np.asarray(block_records, dtype=np.float64)))
