"""Host twin of the per-rung reproducible sums (DESIGN.md section 3.13 "Per-rung sums"; include/amc.h amc_reduce_rungs_exact), written
from that text with the oracle's own kind-R sum (oracle_lib.xsum_r) and sharing no code with the product.

For a ladder of R rungs, rung r and column c the record is the kind-R sum over the ladders l of ONE chain's summand, chain l R + r:
    c = 0  double(potential_T(x))      the energies as the caller holds them (the oracle simulation's e, or download_state's)
    c = 1  double(x)
    c = 2  fl(double(x) * double(x))   one Float64 product (numpy's * on float64 is a single IEEE operation)
-- that is, xsum_r over the strided slices e[r::R], x[r::R] and x[r::R] * x[r::R].  A column nobody asked for is an all-zero record.
"""
import numpy as np

import oracle_lib as O

WORDS = O.XS_WORDS
E, X, XX, ALL = 1, 2, 4, 7


def records(x, e, n_rungs: int, columns: int = ALL) -> np.ndarray:
    """records[R][3][12] of the chains whose positions are x and energies e (Float64 arrays of whole ladders)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    R = int(n_rungs)
    assert x.size == e.size and x.size % R == 0
    out = np.zeros((R, 3, WORDS))
    for r in range(R):
        xr = np.ascontiguousarray(x[r::R])
        with np.errstate(all="ignore"):
            xx = xr * xr
        if columns & E:
            out[r, 0] = O.xsum_r(np.ascontiguousarray(e[r::R]))
        if columns & X:
            out[r, 1] = O.xsum_r(xr)
        if columns & XX:
            out[r, 2] = O.xsum_r(xx)
    return out


def merge(parts) -> np.ndarray:
    """The shards' records merged (integers: any order)."""
    parts = list(parts)
    tot = np.array(parts[0], dtype=np.float64).reshape(-1, WORDS)
    for p in parts[1:]:
        tot = O.xsum_merge(tot, np.asarray(p, dtype=np.float64).reshape(-1, WORDS))
    return tot.reshape(np.asarray(parts[0]).shape)


def values(rec) -> np.ndarray:
    """The Float64 of every record, shape (R, 3)."""
    rec = np.asarray(rec, dtype=np.float64)
    return O.xsum_round(rec.reshape(-1, WORDS)).reshape(rec.shape[:-1])


def means(rec, n_ladders_global: int) -> np.ndarray:
    return values(rec) / float(n_ladders_global)
