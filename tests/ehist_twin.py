"""Host twin of the energy histograms (include/amc.h amc_energy_histogram_accumulate), written from that text:
the energies from the oracle (amo_potential / amo_potential_f32 through oracle_lib), the bin rule in numpy Float64, a row per group.
It shares no code with the product.

For chain i of group i mod G, v = double(potential_T(x_i)); with inv_w = n_bins / (hi - lo) in Float64 the cell of v is
    n_bins + 2  if v is NaN
    n_bins      if v < lo
    n_bins + 1  if v >= hi
    min(trunc((v - lo) * inv_w), n_bins - 1)  otherwise
-- one Float64 subtraction, one Float64 product (numpy's elementwise operations: nothing is contracted), truncation toward zero.
"""
import numpy as np

import oracle_lib as O


def energies(potential, x, f32: bool = False) -> np.ndarray:
    """double(potential_T(x)) per chain; ``x``: the positions as download_state returns them (exact images of the state type's values).
    ``potential``: a built-in name, or whatever oracle_lib.install_custom_potential installed."""
    lib, pot = O.load(), O._potential_id(potential)
    xs = np.asarray(x, dtype=np.float64).reshape(-1)
    if f32:
        return np.array([lib.amo_potential_f32(pot, float(np.float32(v))) for v in xs], dtype=np.float64)
    return np.array([lib.amo_potential(pot, float(v)) for v in xs], dtype=np.float64)


def cells(v, lo: float, hi: float, n_bins: int) -> np.ndarray:
    """The cell of every value of ``v`` (Float64), by the rule above."""
    v = np.asarray(v, dtype=np.float64)
    lo, hi, n = np.float64(lo), np.float64(hi), int(n_bins)
    inv_w = np.float64(n) / (hi - lo)
    out = np.empty(v.shape, dtype=np.int64)
    nan = np.isnan(v)
    below = ~nan & (v < lo)
    above = ~nan & (v >= hi)
    inside = ~(nan | below | above)
    out[nan], out[below], out[above] = n + 2, n, n + 1
    with np.errstate(all="ignore"):
        b = np.trunc((v[inside] - lo) * inv_w).astype(np.int64)
    out[inside] = np.minimum(b, n - 1)
    return out


def histogram(e, lo: float, hi: float, n_bins: int, n_groups: int = 1) -> np.ndarray:
    """counts[G, n_bins + 3] (uint64) of one snapshot of the energies ``e``, chain i in group i mod G."""
    G, n = int(n_groups), int(n_bins)
    c = cells(e, lo, hi, n).reshape(-1, G)
    out = np.zeros((G, n + 3), dtype=np.uint64)
    for g in range(G):
        out[g] = np.bincount(c[:, g], minlength=n + 3).astype(np.uint64)
    return out


def snapshot(potential, x, lo, hi, n_bins, n_groups=1, f32=False) -> np.ndarray:
    """counts[G, n_bins + 3] of the positions ``x``."""
    return histogram(energies(potential, x, f32), lo, hi, n_bins, n_groups)
