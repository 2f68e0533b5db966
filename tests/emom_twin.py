"""Host twin of the moments per energy bin (DESIGN.md section 3.17 "Moments per bin"; include/amc.h amc_energy_moments_accumulate),
written from that text: the energies and the cells from ehist_twin (the oracle's potential, the bin rule in numpy Float64), the
deposits in numpy Float64 with rint.  It shares no code with the product.

For chain i of group i mod G with e_i = double(potential_T(x_i)), xd_i = double(x_i):
    cell = ehist_twin.cells(e_i); if cell < n_bins and not (|xd_i| <= x_bound): cell = n_bins + 3, and the chain reaches no sum
    a chain of bin b adds to the kept columns of (group, b), with eb = ilogb(x_bound) + 1:
        X    rint(lsb1(xd) * 2^-(eb - 32))
        XX   rint(lsb1(fl(xd * xd)) * 2^-(2 eb - 32))
        POS  1 if xd > 0
lsb1(v): the bit pattern of v with its last bit set.  Scaling by a power of two is exact here (the scaled value is far from the
subnormals unless it rounds to 0 anyway), and no scaled value lies half way between two integers, so rint's tie rule never decides.
"""
import math

import numpy as np

import ehist_twin as T

X, XX, POS = 1, 2, 4
COLUMNS = (X, XX, POS)                   # mask-bit order


def exponents(x_bound: float):
    """(E_X, E_XX) of the bound."""
    eb = math.frexp(float(x_bound))[1]          # x_bound = m 2^eb with 0.5 <= m < 1: eb = ilogb(x_bound) + 1
    return eb - 32, 2 * eb - 32


def lsb1(v) -> np.ndarray:
    return (np.asarray(v, dtype=np.float64).view(np.uint64) | np.uint64(1)).view(np.float64)


def quanta(v, e: int) -> np.ndarray:
    """rint(lsb1(v) 2^-e) as int64."""
    with np.errstate(all="ignore"):
        return np.rint(np.ldexp(lsb1(v), -int(e))).astype(np.int64)


def deposits(xd, x_bound: float):
    """{column: int64[n]} of the positions ``xd`` (Float64 images of the state type's values), every one taken as inside the bound."""
    xd = np.asarray(xd, dtype=np.float64).reshape(-1)
    e_x, e_xx = exponents(x_bound)
    return {X: quanta(xd, e_x), XX: quanta(xd * xd, e_xx), POS: (xd > 0).astype(np.int64)}


def moments(e, xd, lo, hi, n_bins, mask, x_bound, n_groups=1):
    """(counts[G, n_bins + 4] uint64, sums[G, C, n_bins] int64) of one snapshot: energies ``e``, positions ``xd``, chain i in group i mod G."""
    G, n = int(n_groups), int(n_bins)
    xd = np.asarray(xd, dtype=np.float64).reshape(-1)
    cell = T.cells(e, lo, hi, n)
    with np.errstate(invalid="ignore"):
        inside = np.abs(xd) <= float(x_bound)            # False for NaN
    cell = np.where((cell < n) & ~inside, n + 3, cell)
    cols = [c for c in COLUMNS if mask & c]
    dep = deposits(np.where(inside, xd, 0.0), x_bound)
    counts = np.zeros((G, n + 4), dtype=np.uint64)
    sums = np.zeros((G, len(cols), n), dtype=np.int64)
    group = np.arange(xd.size) % G
    for g in range(G):
        mine = group == g
        counts[g] = np.bincount(cell[mine], minlength=n + 4).astype(np.uint64)
        binned = mine & (cell < n)
        for j, c in enumerate(cols):
            np.add.at(sums[g, j], cell[binned], dep[c][binned])
    return counts, sums


def snapshot(potential, x, lo, hi, n_bins, mask, x_bound, n_groups=1, f32=False):
    """(counts, sums) of the positions ``x`` as download_state returns them."""
    return moments(T.energies(potential, x, f32), x, lo, hi, n_bins, mask, x_bound, n_groups)
