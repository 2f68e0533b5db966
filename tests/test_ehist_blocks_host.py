"""The host side of the energy histograms per jackknife block (DESIGN.md section 3.17 "Per block"), no GPU: the twin of the blocked
counts (tests/ehist_blocks_twin.py) against explicit loops, ``jackknife.jackknife_counts`` against brute force and the textbook
formula, its refusals, ``wham``'s start vector, and the calibration of the error bar on synthetic multinomial blocks.

The calibration: harmonic e = x^2 at beta has P(e < t) = erf(sqrt(beta t)) exactly; K = 3 rungs beta = 1, 1.5, 2.25, 60 bins on
[0, 6), B = 16 blocks of 1500 samples per rung.  N = 200 independent replications give the empirical SD of theta (its own relative
error 1 / sqrt(2 N) = 5 %) and the mean jackknife se (about 1 %), so mean se / SD must lie in [0.85, 1.15] (3 sigma).  Measured with
the committed seed, per quantity (f_1 - f_0, f_2 - f_0, C at beta 1.2247, C at beta 1.8371): 0.930, 0.924, 0.981, 0.907 (the test prints them)."""
import math

import numpy as np
import pytest

from montecarlo_amd import reweighting as W
from montecarlo_amd.jackknife import block_counts, jackknife_counts

import ehist_blocks_twin as KB
import ehist_twin as T


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,L,B,chunk,first", [(1, 65, 2, 1, 0), (3, 22, 4, 3, 0), (7, 37, 5, 1, 11), (2, 3, 3, 1, 0), (3, 6, 4, 4, 8)])
def test_twin_is_the_cells_composed_with_the_block_rule(G, L, B, chunk, first):
    rng = np.random.default_rng(5)
    e = rng.uniform(-0.5, 3.0, G * L)
    e[::17] = np.nan
    lo, hi, n = 0.125, 2.5, 23
    got = KB.histogram(e, lo, hi, n, G, B, chunk, first)
    want = np.zeros((B, G, n + 3), dtype=np.uint64)
    cell = T.cells(e, lo, hi, n)
    for i in range(G * L):                                  # chain i: rung i mod G of local ladder i div G
        ladder = i // G
        want[((first + ladder) // chunk) % B, i % G, cell[i]] += np.uint64(1)
    assert np.array_equal(got, want)
    assert np.array_equal(got.sum(axis=0, dtype=np.uint64), T.histogram(e, lo, hi, n, G))
    per_block = block_counts(L, B, chunk, first)
    assert np.array_equal(KB.ladders(L, B, chunk, first), per_block)
    assert np.array_equal(got.sum(axis=2), np.repeat(per_block.astype(np.uint64)[:, None], G, axis=1))


# ---- jackknife_counts ---------------------------------------------------------------------------------------------------------------------
def _blocks(rng, B=7, shape=(3, 11), scale=40):
    return rng.integers(1, scale, size=(B,) + shape).astype(np.uint64)


def test_jackknife_counts_against_brute_force():
    rng = np.random.default_rng(11)
    blocks = _blocks(rng)
    blocks[3] += np.uint64(1) << np.uint64(60)              # counts beyond 2^53: the totals stay exact in uint64
    energies = np.linspace(0.1, 2.0, 11)

    def fn(c):
        assert c.dtype == np.uint64
        low = (c & np.uint64(0xFFFFFFFF)).astype(np.float64)  # (a function that sees every bit)
        p = low / low.sum(axis=1, keepdims=True)
        return np.concatenate([p @ energies, np.log(low[:, 0] + 1.0)])

    theta, se = jackknife_counts(blocks, fn)
    B = blocks.shape[0]
    total = np.zeros(blocks.shape[1:], dtype=np.uint64)
    for b in range(B):
        total = total + blocks[b]
    assert np.array_equal(theta, fn(total))
    reps = []
    for b in range(B):                                      # the leave-one-out arrays rebuilt from the blocks that stay
        rest = np.zeros(blocks.shape[1:], dtype=np.uint64)
        for k in range(B):
            if k != b:
                rest = rest + blocks[k]
        reps.append(fn(rest))
    reps = np.stack(reps)
    want = np.sqrt((B - 1) / B * ((reps - reps.mean(axis=0)) ** 2).sum(axis=0))
    assert np.array_equal(se, want)


def test_linear_function_gives_the_textbook_standard_error():
    """Equal blocks, theta = the mean energy: the jackknife se is the standard error of the block means, sd / sqrt(B)."""
    rng = np.random.default_rng(12)
    B, n_b, n_bins = 12, 500, 9
    energies = np.arange(n_bins) + 0.5
    blocks = np.stack([rng.multinomial(n_b, np.full(n_bins, 1.0 / n_bins)) for _ in range(B)]).astype(np.uint64)
    theta, se = jackknife_counts(blocks, lambda c: np.array([c.astype(np.float64) @ energies / c.sum()]))
    means = blocks.astype(np.float64) @ energies / n_b
    assert theta[0] == pytest.approx(means.mean(), rel=1e-13)
    assert se[0] == pytest.approx(means.std(ddof=1) / math.sqrt(B), rel=1e-10)


def test_refusals():
    rng = np.random.default_rng(13)
    blocks = _blocks(rng)
    fn = lambda c: c.sum(dtype=np.float64)
    with pytest.raises(ValueError, match="at least 2"):
        jackknife_counts(blocks[:1], fn)
    empty = blocks.copy()
    empty[4] = 0
    with pytest.raises(ValueError, match="block 4 is empty"):
        jackknife_counts(empty, fn)
    with pytest.raises(ValueError, match="uint64"):
        jackknife_counts(blocks.astype(np.int64), fn)
    # an entry that is -inf in one replicate alone: its se is NaN, the others stand
    def log_counts(c):
        with np.errstate(divide="ignore"):
            return np.log(c.astype(np.float64))

    theta, se = jackknife_counts(np.array([[3, 1], [2, 0], [4, 0]], dtype=np.uint64), log_counts)      # without block 0 the second cell is empty
    assert np.array_equal(theta, np.log([9.0, 1.0])) and np.isfinite(se[0]) and se[0] > 0 and np.isnan(se[1])


# ---- wham's start vector --------------------------------------------------------------------------------------------------------------------
def _harmonic_probabilities(betas, lo, hi, n_bins):
    edges = lo + (hi - lo) / n_bins * np.arange(n_bins + 1)
    cdf = np.array([[math.erf(math.sqrt(b * t)) for t in edges] for b in betas])
    return np.diff(cdf, axis=1)


def test_wham_start_vector():
    betas = np.array([1.0, 1.5, 2.25])
    energies = W.bin_centres(0.0, 6.0, 60)
    rng = np.random.default_rng(14)
    p = _harmonic_probabilities(betas, 0.0, 6.0, 60)
    counts = np.stack([rng.multinomial(20000, np.append(p[k], 1.0 - p[k].sum()))[:-1] for k in range(3)])
    log_g, f, n_iter = W.wham(counts, betas, energies)
    same = W.wham(counts, betas, energies, f0=None)
    assert np.array_equal(same[0], log_g) and np.array_equal(same[1], f) and same[2] == n_iter
    lg1, f1, it1 = W.wham(counts, betas, energies, f0=f + 3.0)      # (normalised to f_0 = 0: the same start)
    assert it1 <= 2 and np.allclose(f1, f, rtol=0, atol=1e-11) and np.allclose(lg1, log_g, rtol=0, atol=1e-11)
    with pytest.raises(ValueError, match="f0"):
        W.wham(counts, betas, energies, f0=np.zeros(2))


# ---- calibration ----------------------------------------------------------------------------------------------------------------------------
def test_the_error_bar_is_calibrated_on_synthetic_blocks():
    betas = np.array([1.0, 1.5, 2.25])
    targets = np.sqrt(betas[:-1] * betas[1:])
    lo, hi, n_bins, B, n_b, N = 0.0, 6.0, 60, 16, 1500, 200
    energies = W.bin_centres(lo, hi, n_bins)
    p = _harmonic_probabilities(betas, lo, hi, n_bins)
    p = np.concatenate([p, 1.0 - p.sum(axis=1, keepdims=True)], axis=1)      # the cell at or above hi
    rng = np.random.default_rng(20250321)

    def theta_of(counts, f0=None):
        log_g, f, _ = W.wham(counts[:, :n_bins], betas, energies, tol=1e-10, f0=f0)
        return np.concatenate([f[1:] - f[0], W.reweight(log_g, energies, targets)[3]]), f

    thetas, ses = [], []
    for _ in range(N):
        blocks = np.stack([np.stack([rng.multinomial(n_b, p[k]) for k in range(3)]) for _ in range(B)]).astype(np.uint64)
        full = {}

        def fn(c):
            if not full:
                full["theta"], full["f"] = theta_of(c)
                return full["theta"]
            return theta_of(c, full["f"])[0]

        theta, se = jackknife_counts(blocks, fn)
        thetas.append(theta)
        ses.append(se)
    ratio = np.mean(ses, axis=0) / np.std(thetas, axis=0, ddof=1)
    print("mean jackknife se / empirical SD:", ratio.tolist())
    assert np.all(ratio >= 0.85) and np.all(ratio <= 1.15), ratio
