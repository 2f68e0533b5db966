"""Multiple-histogram reweighting (Ferrenberg-Swendsen / WHAM) of energy histograms, on the host: numpy Float64, deterministic, no
device.  The histograms come from the engine's integer accumulator (HipEngine.energy_histogram_fetch);
everything here works on a few thousand cells.

With n_kb the count of row k (taken at beta_k) in bin b, E_b the bin centre and N_k the in-range total of row k, the density of
states g_b and the free energies f_k = -log Z_k solve

    log g_b = log sum_k n_kb  -  logsumexp_k(log N_k + f_k - beta_k E_b)
    f_k     = -logsumexp_b(log g_b - beta_k E_b)

which `wham` iterates in log space from f = 0, normalised to f_0 = 0, until max |delta f| < tol."""
import numpy as np

__all__ = ["bin_centres", "wham", "reweight", "reweight_observable", "outside_share"]


def bin_centres(lo, hi, n_bins):
    """E_b = lo + (b + 1/2) (hi - lo) / n_bins: the centres of the engine's half-open bins."""
    n = int(n_bins)
    return float(lo) + (np.arange(n, dtype=np.float64) + 0.5) * ((float(hi) - float(lo)) / n)


def _logsumexp(a, axis):
    """log sum exp along `axis`; a slice of -inf alone gives -inf (no NaN, no warning)."""
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.log(np.sum(np.exp(a - m), axis=axis)) + np.squeeze(m, axis=axis)


def _connected(support):
    """Do the rows form ONE connected set under "share a non-empty bin"?  support: bool[K, n_bins]."""
    k = support.shape[0]
    seen = np.zeros(k, dtype=bool)
    seen[0] = True
    frontier = [0]
    while frontier:
        i = frontier.pop()
        touch = np.any(support & support[i], axis=1) & ~seen
        seen |= touch
        frontier.extend(np.nonzero(touch)[0].tolist())
    return bool(np.all(seen))


def wham(counts, betas, energies, tol=1e-12, max_iter=100000, f0=None):
    """(log_g[n_bins], f[K], n_iter) from counts[K, n_bins] (integers or reals: expected counts are accepted), betas[K] and the
    bin energies.  f_0 = 0.  Bins empty in every row have log g = -inf and take no part.  ValueError: a row without an in-range
    count, rows whose supports are not connected, no convergence within `max_iter`.  ``f0``: the f[K] the iteration starts from
    instead of zeros (a jackknife's replicates start from the full solution); the fixed point is the same."""
    n = np.asarray(counts, dtype=np.float64)
    b = np.asarray(betas, dtype=np.float64).reshape(-1)
    e = np.asarray(energies, dtype=np.float64).reshape(-1)
    if n.ndim != 2 or n.shape != (b.size, e.size):
        raise ValueError(f"wham: counts of shape {n.shape} for {b.size} betas and {e.size} energies")
    if not np.all(np.isfinite(n)) or np.any(n < 0):
        raise ValueError("wham: counts must be finite and non-negative")
    totals = n.sum(axis=1)
    if np.any(totals <= 0):
        raise ValueError(f"wham: row {int(np.argmin(totals > 0))} has no count inside the bins")
    if not _connected(n > 0):
        raise ValueError("wham: the rows' supports are not connected (no chain of rows sharing a non-empty bin links them all): "
                         "their relative free energies are undetermined")
    live = n.sum(axis=0) > 0
    with np.errstate(divide="ignore"):
        log_num = np.log(n[:, live].sum(axis=0))
    log_n = np.log(totals)
    be = np.outer(b, e[live])                                   # beta_k E_b
    f = np.zeros(b.size)
    if f0 is not None:
        f = np.array(f0, dtype=np.float64).reshape(-1)
        if f.shape != b.shape or not np.all(np.isfinite(f)):
            raise ValueError(f"wham: f0 of shape {f.shape} for {b.size} betas, or not finite")
        f = f - f[0]
    for it in range(1, int(max_iter) + 1):
        log_g = log_num - _logsumexp((log_n + f)[:, None] - be, axis=0)
        f_new = -_logsumexp(log_g[None, :] - be, axis=1)
        f_new = f_new - f_new[0]
        delta = float(np.max(np.abs(f_new - f)))
        f = f_new
        if delta < tol:
            # the density of states on the normalisation of the f returned: one more half step
            log_g = log_num - _logsumexp((log_n + f)[:, None] - be, axis=0)
            out = np.full(e.size, -np.inf)
            out[live] = log_g
            return out, f, it
    raise ValueError(f"wham: no convergence within {int(max_iter)} iterations (last max |delta f| = {delta:.3e}, tol = {tol:.3e})")


def reweight(log_g, energies, betas):
    """(log Z, <e>, <e^2>, C = beta^2 (<e^2> - <e>^2)) at every beta of `betas` (a scalar or an array) from a density of states on the
    normalisation `wham` leaves it in: log Z(beta_0) = -f_0 = 0 there."""
    lg = np.asarray(log_g, dtype=np.float64).reshape(-1)
    e = np.asarray(energies, dtype=np.float64).reshape(-1)
    b = np.asarray(betas, dtype=np.float64)
    live = lg > -np.inf
    a = lg[live][None, :] - np.outer(b.reshape(-1), e[live])
    log_z = _logsumexp(a, axis=1)
    p = np.exp(a - log_z[:, None])
    m1 = p @ e[live]
    # the variance about the mean: no cancellation of two large moments
    var = np.sum(p * (e[live][None, :] - m1[:, None]) ** 2, axis=1)
    m2 = var + m1 * m1
    c = b.reshape(-1) ** 2 * var
    return tuple(v.reshape(b.shape) for v in (log_z, m1, m2, c))


def reweight_observable(log_g, energies, betas, sums, counts):
    """<o>(beta) at every beta of `betas` (a scalar or an array) of an observable that is no function of the energy, from its sums per
    bin: sums[K, n_bins] = S_kb, the sum of o over the samples of row k that fell into bin b, and counts[K, n_bins] = n_kb.  The
    microcanonical mean o_b = sum_k S_kb / sum_k n_kb is weighted with the density of states `wham` returns,

        <o>(beta) = sum_b g_b exp(-beta E_b) o_b / sum_b g_b exp(-beta E_b),

    the weights formed in log space.  Bins with sum_k n_kb = 0 (log g = -inf) take no part, in the numerator or the denominator; NaN
    where no bin is left."""
    lg = np.asarray(log_g, dtype=np.float64).reshape(-1)
    e = np.asarray(energies, dtype=np.float64).reshape(-1)
    b = np.asarray(betas, dtype=np.float64)
    s = np.asarray(sums, dtype=np.float64)
    n = np.asarray(counts, dtype=np.float64)
    if s.ndim == 1:
        s, n = s[None, :], n.reshape(1, -1)
    if s.shape != n.shape or s.ndim != 2 or s.shape[1] != e.size or lg.size != e.size:
        raise ValueError(f"reweight_observable: sums of shape {s.shape}, counts of shape {n.shape} for {e.size} energies and {lg.size} log g")
    total = n.sum(axis=0)
    live = (total > 0) & (lg > -np.inf)
    if not np.any(live):
        return np.full(b.shape, np.nan)
    mean = s[:, live].sum(axis=0) / total[live]
    a = lg[live][None, :] - np.outer(b.reshape(-1), e[live])
    p = np.exp(a - _logsumexp(a, axis=1)[:, None])
    return (p @ mean).reshape(b.shape)


def outside_share(counts_with_tail_cells):
    """Per row of counts[..., n_bins + 3] the share of its total in the three tail cells: [..., 3] = below lo, at or above hi, NaN."""
    c = np.asarray(counts_with_tail_cells, dtype=np.float64)
    total = c.sum(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(total > 0, c[..., -3:] / total, 0.0)
    return share
