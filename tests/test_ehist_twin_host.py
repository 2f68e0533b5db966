"""The host twin of the energy histograms (tests/ehist_twin.py) held to the text of DESIGN.md section 3.17: the row-sum identity and
the edges of the bin rule.  No GPU; the GPU tests compare the engine with this twin bit for bit."""
import numpy as np

import ehist_twin as T


def test_every_row_sums_to_its_chains(oracle):
    rng = np.random.default_rng(1)
    x = rng.normal(0.0, 1.2, size=7 * 33)
    x[[5, 17, 60]] = [np.nan, np.inf, 1e200]
    for G in (1, 3, 7):
        for pot in ("harmonic", "double_well"):
            h = T.snapshot(pot, x, 0.25, 2.0, 13, G)
            assert h.shape == (G, 16) and h.dtype == np.uint64
            assert np.array_equal(h.sum(axis=1), np.full(G, x.size // G, dtype=np.uint64))


def test_float32_state_takes_the_float32_energy(oracle):
    x = np.float64(np.float32(0.3))
    e32, e64 = T.energies("harmonic", [x], f32=True)[0], T.energies("harmonic", [x])[0]
    assert e32 == np.float64(np.float32(x) * np.float32(x)) and e64 == x * x and e32 != e64


def test_edges_of_the_bin_rule():
    lo, hi, n = 0.5, 2.0, 6
    assert T.cells([lo], lo, hi, n)[0] == 0                                  # e == lo: bin 0
    assert T.cells([np.nextafter(lo, -np.inf)], lo, hi, n)[0] == n           # just below: the "below" cell
    assert T.cells([hi], lo, hi, n)[0] == n + 1                              # e == hi: the ">= hi" cell (half-open bins)
    assert T.cells([np.nextafter(hi, lo)], lo, hi, n)[0] == n - 1            # the last value inside: the last bin
    assert list(T.cells([np.nan, np.inf, -np.inf, 1e300], lo, hi, n)) == [n + 2, n + 1, n, n + 1]


def test_the_clamp_of_the_last_bin():
    """There are bins for which fl(fl(hi - ulp - lo) * inv_w) == n_bins: the rule clamps to the last bin, it does not spill into a tail cell."""
    found = 0
    for n in range(1, 400):
        for lo, hi in ((0.0, 0.1), (0.0, 0.7), (0.3, 1.9), (-1.0, 2.3)):
            v = np.nextafter(np.float64(hi), np.float64(lo))
            raw = np.trunc((v - np.float64(lo)) * (np.float64(n) / (np.float64(hi) - np.float64(lo))))
            found += raw == n
            assert T.cells([v], lo, hi, n)[0] == n - 1
    assert found > 0, "no example of the rounding the clamp exists for: widen the search"


def test_negative_zero_is_not_below_zero():
    assert T.cells([-0.0], 0.0, 1.0, 4)[0] == 0
    assert T.histogram([-0.0, 0.0], 0.0, 1.0, 4)[0, 0] == 2
