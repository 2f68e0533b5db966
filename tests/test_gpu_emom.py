"""Moments per energy bin on the device (DESIGN.md section 3.17 "Moments per bin"; include/amc.h amc_energy_moments_accumulate ..
amc_set_energy_moments) against their host twin (tests/emom_twin.py: the oracle's energies, the bin rule and the deposits in numpy
Float64), integer for integer -- counts AND sums, no tolerance anywhere.  The twin is applied to download_state() taken right behind
each snapshot.  Shapes are the smallest at which the kernel takes another path: fewer chains than threads and the one-by-one tail
behind the four-fold loop; a ladder with an odd R and one bin; R = 64 with the word count G (n_bins + 4) + 2 C G n_bins on both sides of
the static LDS array (12288 words) for one column and for three; Float32 state; a potential compiled at run time."""
import ctypes as C

import numpy as np
import pytest

from montecarlo_amd.system import CustomPotential

import emom_twin as E

pytestmark = pytest.mark.gpu
CUSTOM = CustomPotential("x*x*x*x - 2.0*x*x + 0.25*x")
LADDER = lambda R: 0.5 * 1.5 ** np.arange(R)
ERR_BAD_ARG, ERR_STATE = -1, -5
LDS_WORDS = 12288                       # EHIST_LDS_CELLS of amc_ehist.h
ALL = E.X | E.XX | E.POS
FORM = (0.125, 2.5, 200, ALL, 1.5)      # lo, hi, n_bins, mask, x_bound of most tests: energies below, inside and above the bins, and
                                        # binned chains beyond the bound (the double well at 1.5 < |x| < 1.6 has e < 2.5)


def start_state(M, R=0, offset=0):
    ids = np.arange(offset, offset + M)
    x = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)
    return x, (LADDER(R)[ids % R] if R else None)


def make(gpu, M, R=0, *, potential="double_well", dtype="f64", offset=0, n_global=None, seed=23, env=None, x=None, **kw):
    mp = pytest.MonkeyPatch()
    for k, v in (env or {}).items():
        mp.setenv(k, v)
    try:
        eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=n_global or offset + M, potential=potential, beta=1.0,
                            sigma=[0.5], weight=[1.0], seed=seed, dtype=dtype, **kw)
    finally:
        mp.undo()
    x0, beta = start_state(M, R, offset)
    eng.upload_state(x0 if x is None else x, beta)
    if R:
        eng.set_ladder(R)
    return eng


def twin_now(eng, potential, form, R, dtype="f64"):
    return E.snapshot(potential, eng.download_state(want_e=False)[0], *form, max(R, 1), dtype == "f32")


def same(got, want, what=""):
    """(counts, sums) against the twin's, as integers."""
    for name, g, w, dt in (("counts", got[0], want[0], np.uint64), ("sums", got[1], want[1], np.int64)):
        assert g.shape == w.shape and g.dtype == dt, (what, name, g.shape, w.shape, g.dtype)
        if not np.array_equal(g, w):
            at = tuple(int(v) for v in np.argwhere(g != w)[0])
            raise AssertionError(f"{what}: {name} differ from the twin, first at {at}: {int(g[at])} != {int(w[at])}")


def check_sequence(eng, potential, form, R, what, dtype="f64"):
    """Three snapshots queued with sweeps (and an exchange step) between them: the accumulator is the sum of the twin's snapshots,
    every row of counts sums to snapshots x ladders, fetch resets nothing, fetch with reset frees the form."""
    G, L, n = max(R, 1), eng.n_chains // max(R, 1), form[2]
    cols = bin(form[3]).count("1")
    want = [np.zeros((G, n + 4), dtype=np.uint64), np.zeros((G, cols, n), dtype=np.int64)]
    for step in range(3):
        if step == 1:
            eng.sweep(3)
        if step == 2:
            eng.exchange(1) if R else eng.sweep(1)
        eng.energy_moments_accumulate(*form)
        c, s = twin_now(eng, potential, form, R, dtype)
        want[0] += c
        want[1] += s
    counts, sums, n_snap, got_form = eng.energy_moments_fetch()
    same((counts, sums), want, what)
    assert n_snap == 3 and got_form == (float(form[0]), float(form[1]), n, form[3], float(form[4]))
    assert np.array_equal(counts.sum(axis=1), np.full(G, 3 * L, dtype=np.uint64))          # the row-sum identity of the contract
    again = eng.energy_moments_fetch(reset=True)
    assert np.array_equal(again[0], counts) and np.array_equal(again[1], sums) and again[2] == 3
    empty = eng.energy_moments_fetch()
    assert empty[0].shape == (G, 0) and empty[1].shape == (G, 0, 0) and empty[2] == 0 and empty[3] == (0.0, 0.0, 0, 0, 0.0)
    return counts, sums


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 1027])
def test_shapes_without_a_ladder(gpu, M):
    """Fewer chains than threads, on the smallest grid the knob gives and on the default one: every chain is taken by the one-by-one
    loop, most threads hold none."""
    for env in ({"AMC_BLOCKS_PER_CU": "1"}, None):
        eng = make(gpu, M, env=env)
        counts, _ = check_sequence(eng, "double_well", FORM, 0, f"M={M} env={env}")
        eng.close()
    if M == 1027:
        assert counts[0, FORM[2] + 3] > 0 and counts[0, :FORM[2]].sum() > 0          # the form does put chains beyond the bound


def test_grid_stride(gpu):
    """One block per CU caps the grid at 65 536 threads: 300 011 chains walk it five times -- four loads in flight, then the tail
    loop -- and end ragged; with R = 3 a trip is 21 845 ladders and the last threads of the grid hold none."""
    for M, R in ((300011, 0), (3 * 100003, 3)):
        eng = make(gpu, M, R, env={"AMC_BLOCKS_PER_CU": "1"})
        eng.sweep(2)
        eng.energy_moments_accumulate(*FORM)
        counts, sums, n_snap, _ = eng.energy_moments_fetch()
        same((counts, sums), twin_now(eng, "double_well", FORM, R), f"M={M} R={R}")
        assert n_snap == 1
        eng.close()


@pytest.mark.parametrize("n_bins", [1, 200])
def test_a_ladder_of_three_rungs_and_five_ladders(gpu, n_bins):
    eng = make(gpu, 3 * 5, 3)
    check_sequence(eng, "double_well", (0.125, 2.5, n_bins, ALL, 1.5), 3, f"R=3 L=5 bins={n_bins}")
    eng.close()


@pytest.mark.parametrize("mask,n_bins", [(E.XX, 62), (E.XX, 63), (ALL, 26), (ALL, 27)])
def test_both_sides_of_the_lds_word_count(gpu, mask, n_bins):
    """G = 64: one column takes 64 (n + 4) + 128 n words -- 12160 at 62 bins (the per-block path), 12352 at 63 (a global atomic per
    deposit); three columns take 64 (n + 4) + 384 n -- 11904 at 26, 12352 at 27."""
    G, cols = 64, bin(mask).count("1")
    words = G * (n_bins + 4) + 2 * cols * G * n_bins
    assert (words <= LDS_WORDS) == (n_bins in (62, 26))
    eng = make(gpu, G * 3, G)
    check_sequence(eng, "double_well", (0.0, 3.0, n_bins, mask, 1.5), G, f"mask={mask} bins={n_bins} words={words}")
    eng.close()


@pytest.mark.parametrize("mask", [E.X, E.POS, E.X | E.POS, E.XX | E.POS])
def test_every_column_choice_keeps_its_columns_in_bit_order(gpu, mask):
    eng = make(gpu, 5 * 41, 5)
    check_sequence(eng, "double_well", (0.125, 2.5, 50, mask, 1.5), 5, f"mask={mask}")
    eng.close()


# ---- 2. models and state types ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("potential", ["harmonic", CUSTOM], ids=["harmonic", "custom"])
def test_models_and_float32_state(gpu, potential, dtype):
    """A built-in potential and one compiled at run time (every kernel of a Float32 handle is), a non-power-of-two bound."""
    form = (-1.25, 2.5, 200, ALL, 1.45) if potential is CUSTOM else (0.125, 2.5, 200, ALL, 1.45)
    for R, L in ((0, 257), (5, 103)):
        eng = make(gpu, L * max(R, 1), R, potential=potential, dtype=dtype)
        check_sequence(eng, potential, form, R, f"{dtype} R={R}", dtype)
        eng.close()


def test_global_path_with_float32_state(gpu):
    eng = make(gpu, 3 * 85, 3, potential="harmonic", dtype="f32")
    check_sequence(eng, "harmonic", (0.0, 3.0, 8192, ALL, 1.5), 3, "f32 global path", "f32")
    eng.close()


# ---- 3. planted positions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("R", [0, 3])
def test_planted_positions(gpu, R, dtype):
    """Harmonic e = x x on [0.25, 2.25) with x_bound = 1.25: NaN (the NaN cell, no sum), +-Inf and 10^200 (e = +Inf: at or above hi),
    +-0.5 (e = lo: bin 0), +-1.5 (e = hi), -0.0 (below lo), +-1.25 (the bound itself: inside), +-1.375 (e = 1.890625 inside the bins,
    |x| beyond the bound: the fourth cell, no sum).  All exact in both state types."""
    M = 3 * 43
    x, _ = start_state(M, R)
    x = np.clip(x, -1.2, 1.2)                              # (the rest stays inside the bound)
    plant = {4: np.nan, 5: np.inf, 6: -np.inf, 7: 1e200, 8: 0.5, 9: -0.5, 10: 1.5, 11: -1.5, 12: -0.0, 13: 1.25, 14: -1.25, 15: 1.375, 16: -1.375}
    for i, v in plant.items():
        x[i] = v
    lo, hi, n, x_bound = 0.25, 2.25, 16, 1.25
    form = (lo, hi, n, ALL, x_bound)
    eng = make(gpu, M, R, potential="harmonic", dtype=dtype, x=x)
    eng.energy_moments_accumulate(*form)
    counts, sums, n_snap, _ = eng.energy_moments_fetch()
    same((counts, sums), twin_now(eng, "harmonic", form, R, dtype), f"planted R={R} {dtype}")
    assert n_snap == 1
    G = max(R, 1)
    # the planted chains alone, cell by cell, from the text of the rule: where each is counted, and which of them reach a sum
    cell_of = {4: n + 2, 5: n + 1, 6: n + 1, 7: n + 1, 8: 0, 9: 0, 10: n + 1, 11: n + 1, 12: n, 13: 10, 14: 10, 15: n + 3, 16: n + 3}
    xs = eng.download_state(want_e=False)[0]
    rest = np.delete(np.arange(M), list(plant))
    alone = E.snapshot("harmonic", xs[rest], *form, 1, dtype == "f32")[0]
    assert alone[0, n + 3] == 0 and alone[0, n + 2] == 0          # (of the rest, nothing is beyond the bound or NaN)
    want_c = np.zeros((G, n + 4), dtype=np.uint64)
    want_s = np.zeros((G, 3, n), dtype=np.int64)
    e_x, e_xx = E.exponents(x_bound)
    for i in rest:
        c1, s1 = E.snapshot("harmonic", xs[i:i + 1], *form, 1, dtype == "f32")
        want_c[i % G] += c1[0]
        want_s[i % G] += s1[0]
    for i, cell in cell_of.items():
        want_c[i % G, cell] += 1
        if cell < n:                                       # +-0.5 into bin 0, +-1.25 into bin 10: x in quanta of 2^(1 - 32), x^2 of 2^(2 - 32)
            v = plant[i]
            want_s[i % G, 0, cell] += int(round(v * 2.0 ** -e_x))
            want_s[i % G, 1, cell] += int(round(v * v * 2.0 ** -e_xx))
            want_s[i % G, 2, cell] += 1 if v > 0 else 0
    same((counts, sums), (want_c, want_s), "planted cells")
    assert counts[:, n + 3].sum() == 2 and counts[:, n + 2].sum() == 1
    eng.close()


# ---- 4. grids, shards, the checkpoint pair ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 4])
def test_two_grids_and_two_shards_hold_the_same_integers(gpu, R):
    G = max(R, 1)
    M = G * 1300
    cut = G * 514
    whole = make(gpu, M, R, seed=31)
    small = make(gpu, M, R, seed=31, env={"AMC_BLOCKS_PER_CU": "1"})
    parts = [make(gpu, cut, R, offset=0, n_global=M, seed=31), make(gpu, M - cut, R, offset=cut, n_global=M, seed=31)]
    for eng in [whole, small] + parts:
        eng.sweep(2)
        eng.energy_moments_accumulate(*FORM)
        if R:
            eng.exchange(2)
        eng.sweep(1)
        eng.energy_moments_accumulate(*FORM)
    want = whole.energy_moments_fetch()
    other = small.energy_moments_fetch()
    same(other[:2], want[:2], f"another grid R={R}")
    got = [p.energy_moments_fetch() for p in parts]
    assert all(g[2] == want[2] == 2 for g in got) and other[2] == 2
    same((got[0][0] + got[1][0], got[0][1] + got[1][1]), want[:2], f"two shards R={R}")
    for eng in [whole, small] + parts:
        eng.close()


@pytest.mark.parametrize("R", [0, 5])
def test_set_round_trip_then_one_more_snapshot(gpu, R):
    a, b = make(gpu, 5 * 61, R), make(gpu, 5 * 61, R)
    a.sweep(2)
    a.energy_moments_accumulate(*FORM)
    a.sweep(1)
    a.energy_moments_accumulate(*FORM)
    counts, sums, n_snap, form = a.energy_moments_fetch()
    b.upload_state(a.download_state(want_e=False)[0], start_state(5 * 61, R)[1])
    b.step = a.step
    b.set_energy_moments(*form, counts, sums, n_snap)
    back = b.energy_moments_fetch()
    assert np.array_equal(back[0], counts) and np.array_equal(back[1], sums) and back[2:] == (n_snap, form)
    for eng in (a, b):
        eng.sweep(2)
        eng.energy_moments_accumulate(*FORM)
    ca, cb = a.energy_moments_fetch(), b.energy_moments_fetch()
    same(cb[:2], ca[:2], "restored accumulator")
    assert ca[2] == cb[2] == 3
    b.set_energy_moments()                                 # None clears
    assert b.energy_moments_fetch()[3] == (0.0, 0.0, 0, 0, 0.0)
    b.energy_moments_accumulate(0.0, 1.0, 7, E.X, 2.0)     # ... and frees the form
    got = b.energy_moments_fetch()
    assert got[0].shape == (max(R, 1), 11) and got[1].shape == (max(R, 1), 1, 7)
    a.close()
    b.close()


# ---- 5. beside the energy histograms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 4])
def test_with_nothing_beyond_the_bound_the_counts_are_the_energy_histograms(gpu, R):
    """Both accumulators stand on one handle, independent of each other; with a bound no chain reaches the first n_bins + 3 cells of
    every row are amc_energy_histogram_accumulate's."""
    eng = make(gpu, 4 * 300, R)
    lo, hi, n = 0.125, 2.5, 200
    for _ in range(2):
        eng.sweep(2)
        eng.energy_histogram_accumulate(lo, hi, n)
        eng.energy_moments_accumulate(lo, hi, n, ALL, 64.0)
    eng.energy_histogram_accumulate(lo, hi, n)             # (a third snapshot of the plain one alone)
    plain, n_plain, _ = eng.energy_histogram_fetch()
    eng.energy_histogram_fetch(reset=True)                 # ... whose reset leaves the moments alone
    eng.energy_histogram_accumulate(lo, hi, n)
    counts, sums, n_snap, _ = eng.energy_moments_fetch()
    assert n_plain == 3 and n_snap == 2 and not counts[:, n + 3].any()
    third = eng.energy_histogram_fetch()[0]
    assert np.array_equal(counts[:, :n + 3], plain - third)
    eng.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def fetch_sizes(eng):
    ng, nb, nc, lo, hi, mask, bound, ns = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0), C.c_int(0), C.c_double(0), C.c_uint64(0)
    args = (C.byref(ng), C.byref(nb), C.byref(nc), C.byref(lo), C.byref(hi), C.byref(mask), C.byref(bound), C.byref(ns))
    return args, lambda: (ng.value, nb.value, nc.value, lo.value, hi.value, mask.value, bound.value, ns.value)


def test_a_refused_first_call_leaves_nothing_allocated(gpu):
    eng = make(gpu, 4 * 50, 4)
    lib, h = eng._lib, eng._h
    acc = lib.amc_energy_moments_accumulate
    assert acc(h, 0.125, 2.5, 200, 0, 1.5) == ERR_BAD_ARG and b"mask" in lib.amc_last_error()
    assert acc(h, 0.125, 2.5, 200, 8, 1.5) == ERR_BAD_ARG and acc(h, 0.125, 2.5, 200, -1, 1.5) == ERR_BAD_ARG
    for bound in (0.0, -1.5, float("nan"), float("inf"), -float("inf"), 5e-324, 2.0 ** 500):
        assert acc(h, 0.125, 2.5, 200, ALL, bound) == ERR_BAD_ARG and b"x_bound" in lib.amc_last_error(), bound
    for lo, hi, n in ((0.0, 1.0, 0), (0.0, 1.0, 8193), (1.0, 1.0, 4), (2.0, 1.0, 4), (float("nan"), 1.0, 4), (0.0, float("inf"), 4)):
        assert acc(h, lo, hi, n, ALL, 1.5) == ERR_BAD_ARG, (lo, hi, n)
    args, values = fetch_sizes(eng)
    assert lib.amc_energy_moments_fetch(h, None, None, 0, 0, *args, 0) == 0 and values() == (4, 0, 0, 0.0, 0.0, 0, 0.0, 0)
    assert eng.energy_moments_fetch()[3] == (0.0, 0.0, 0, 0, 0.0)
    eng.energy_moments_accumulate(0.0, 1.0, 3, E.POS, 1.0)           # any form may still begin
    assert eng.energy_moments_fetch()[1].shape == (4, 1, 3)
    eng.close()


def test_refusals_change_nothing(gpu):
    eng = make(gpu, 4 * 50, 4)
    lib, h = eng._lib, eng._h
    eng.sweep(2)
    eng.exchange(1)
    eng.energy_moments_accumulate(*FORM)
    before = eng.energy_moments_fetch()
    x_before = eng.download_state(want_e=False)[0].copy()
    acc = lib.amc_energy_moments_accumulate
    lo, hi, n, mask, bound = FORM
    assert acc(h, lo, hi, 199, mask, bound) == ERR_STATE and b"another form" in lib.amc_last_error()
    assert acc(h, 0.25, hi, n, mask, bound) == ERR_STATE and acc(h, lo, 2.75, n, mask, bound) == ERR_STATE
    assert acc(h, lo, hi, n, E.X | E.XX, bound) == ERR_STATE and acc(h, lo, hi, n, mask, 1.75) == ERR_STATE
    assert acc(h, lo, hi, n, 0, bound) == ERR_BAD_ARG and acc(h, lo, hi, n, mask, 0.0) == ERR_BAD_ARG
    counts, sums = np.zeros(4 * 204, dtype=np.uint64), np.zeros(4 * 3 * 200, dtype=np.int64)
    args, values = fetch_sizes(eng)
    fetch = lib.amc_energy_moments_fetch
    pc, ps = counts.ctypes.data_as(C.POINTER(C.c_uint64)), sums.ctypes.data_as(C.POINTER(C.c_int64))
    assert fetch(h, pc, ps, counts.size - 1, sums.size, *args, 1) == ERR_BAD_ARG and b"capacities" in lib.amc_last_error()
    assert fetch(h, pc, ps, counts.size, sums.size - 1, *args, 1) == ERR_BAD_ARG
    assert fetch(h, pc, None, counts.size, sums.size, *args, 1) == ERR_BAD_ARG
    assert fetch(h, None, None, 0, 0, *args, 1) == 0 and values() == (4, 200, 3, lo, hi, mask, bound, 0)      # the sizes alone, nothing reset
    assert fetch(h, pc, ps, counts.size, sums.size, None, *args[1:], 0) == ERR_BAD_ARG
    # amc_set_energy_moments: rows that do not sum, a sum cell beyond what its count can hold, a POS cell above its count or negative
    c0, s0 = before[0], before[1]
    short = c0.copy()
    short[0, int(np.argmax(short[0]))] -= np.uint64(1)
    with pytest.raises(gpu.AmcError, match="does not sum"):
        eng.set_energy_moments(*FORM, short, s0, 1)
    with pytest.raises(gpu.AmcError, match="does not sum"):
        eng.set_energy_moments(*FORM, c0, s0, 2)
    b = int(np.argmax(c0[2, :n]))
    for col, value in ((0, (int(c0[2, b]) << 32) + 1), (1, -(int(c0[2, b]) << 32) - 1), (2, int(c0[2, b]) + 1), (2, -1)):
        bad = s0.copy()
        bad[2, col, b] = value
        with pytest.raises(gpu.AmcError, match="more than"):
            eng.set_energy_moments(*FORM, c0, bad, 1)
    empty_bin = int(np.argmin(c0[1, :n]))
    assert c0[1, empty_bin] == 0
    bad = s0.copy()
    bad[1, 0, empty_bin] = 1
    with pytest.raises(gpu.AmcError, match="more than"):
        eng.set_energy_moments(*FORM, c0, bad, 1)
    with pytest.raises(gpu.AmcError):
        eng.set_energy_moments(lo, hi, n, 0, bound, c0, s0, 1)
    with pytest.raises(gpu.AmcError):
        eng.set_energy_moments(lo, hi, n, mask, float("nan"), c0, s0, 1)
    after = eng.energy_moments_fetch()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and after[2:] == before[2:]
    assert np.array_equal(eng.download_state(want_e=False)[0].view(np.uint64), x_before.view(np.uint64))
    eng.energy_moments_accumulate(*FORM)                   # ... and the accumulator goes on
    assert eng.energy_moments_fetch()[2] == 2
    eng.close()


def test_capacity_is_refused_before_a_launch(gpu):
    """A cell holds fewer than 2^31 deposits: with 4 chains in one group, 2^29 - 1 snapshots are the most (reached through
    amc_set_energy_moments, not by running); the next accumulate is AMC_ERR_STATE and changes nothing, one snapshot fewer goes on."""
    eng = make(gpu, 4)
    lo, hi, n, mask, bound = 0.0, 4.0, 3, ALL, 2.0
    full = 2 ** 29 - 1
    counts = np.zeros((1, n + 4), dtype=np.uint64)
    counts[0, 1] = 4 * full
    sums = np.zeros((1, 3, n), dtype=np.int64)
    sums[0, :, 1] = (-(4 * full) << 32, (4 * full) << 32, 4 * full)          # the largest magnitudes the cell's count allows
    with pytest.raises(gpu.AmcError, match="2\\^31"):
        eng.set_energy_moments(lo, hi, n, mask, bound, counts * np.uint64(2), sums, 2 * full)
    with pytest.raises(gpu.AmcError, match="2\\^31"):
        c1 = counts.copy()
        c1[0, 1] += np.uint64(4)
        eng.set_energy_moments(lo, hi, n, mask, bound, c1, sums, full + 1)
    assert eng.energy_moments_fetch()[3][2] == 0           # nothing stands after the refusals
    eng.set_energy_moments(lo, hi, n, mask, bound, counts, sums, full)
    assert eng._lib.amc_energy_moments_accumulate(eng._h, lo, hi, n, mask, bound) == ERR_STATE and b"2^31" in eng._lib.amc_last_error()
    got = eng.energy_moments_fetch()
    assert np.array_equal(got[0], counts) and np.array_equal(got[1], sums) and got[2] == full
    counts[0, 1] -= np.uint64(4)
    sums[0, :, 1] = 0
    eng.set_energy_moments(lo, hi, n, mask, bound, counts, sums, full - 1)
    eng.energy_moments_accumulate(lo, hi, n, mask, bound)
    assert eng.energy_moments_fetch()[2] == full
    assert eng._lib.amc_energy_moments_accumulate(eng._h, lo, hi, n, mask, bound) == ERR_STATE
    eng.close()


# ---- 7. what clears it, what keeps it ---------------------------------------------------------------------------------------------------
def test_set_ladder_clears(gpu):
    eng = make(gpu, 6 * 40, 6)
    eng.energy_moments_accumulate(*FORM)
    eng.set_ladder(3)
    assert eng.energy_moments_fetch()[3] == (0.0, 0.0, 0, 0, 0.0)
    form = (0.0, 2.0, 9, E.X | E.POS, 2.0)                 # other groups, another form
    eng.energy_moments_accumulate(*form)
    got = eng.energy_moments_fetch()
    same(got[:2], twin_now(eng, "double_well", form, 3), "behind set_ladder")
    eng.set_ladder(0)
    assert eng.energy_moments_fetch()[0].shape == (1, 0)
    eng.close()


def test_respacing(gpu):
    """A respacing that is not taken (no exchange attempt yet: status 2) leaves the cells; one that is taken (status 0) zeroes counts
    and sums in stream order and keeps the form."""
    R = 4
    eng = make(gpu, R * 64, R)
    eng.sweep(2)
    eng.energy_moments_accumulate(*FORM)
    kept = eng.energy_moments_fetch()
    eng.respace_ladder("acceptance", 1.0, 0.01)
    assert eng.respace_status()[0] == 2
    now = eng.energy_moments_fetch()
    assert np.array_equal(now[0], kept[0]) and np.array_equal(now[1], kept[1]) and now[2] == 1
    eng.respace_ladder("acceptance", 0.5, 0.01, counts=[100] * (R - 1) + [30, 50, 70])
    eng.sweep(1)
    eng.energy_moments_accumulate(*FORM)                   # queued behind the respacing: the only snapshot left
    assert eng.respace_status()[0] == 0
    got = eng.energy_moments_fetch()
    assert got[2] == 1 and got[3] == kept[3]
    same(got[:2], twin_now(eng, "double_well", FORM, R), "behind a respacing")
    assert eng._lib.amc_energy_moments_accumulate(eng._h, 0.0, 1.0, 5, ALL, 1.5) == ERR_STATE          # the form stays fixed
    eng.close()


def test_what_leaves_it_alone(gpu):
    R = 3
    eng = make(gpu, R * 70, R, per_chain_counters=True)
    eng.sweep(2)
    eng.energy_moments_accumulate(*FORM)
    kept = eng.energy_moments_fetch()
    x, beta = start_state(R * 70, R)
    eng.upload_state(x[::-1].copy(), beta)
    eng.set_blocks(2)
    eng.set_blocks(0)
    eng.sweep(4)
    eng.exchange(2)
    eng.energy_histogram_accumulate(0.0, 1.0, 4)
    eng.energy_histogram_fetch(reset=True)
    eng.init_uniform(-1.0, 1.0)
    now = eng.energy_moments_fetch()
    assert np.array_equal(now[0], kept[0]) and np.array_equal(now[1], kept[1]) and now[2:] == kept[2:]
    eng.close()


def test_a_handle_that_accumulates_ends_as_one_that_never_did(gpu):
    a, b = make(gpu, 4 * 129, 4), make(gpu, 4 * 129, 4)
    for _ in range(3):
        for eng in (a, b):
            eng.sweep(3)
            eng.exchange(1)
        a.energy_moments_accumulate(*FORM)
    a.energy_moments_fetch(reset=True)
    for eng in (a, b):
        eng.sweep(2)
    xa, xb = a.download_state(), b.download_state()
    assert all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(xa, xb))
    assert a.step == b.step and a.exchange_step == b.exchange_step
    assert all(np.array_equal(u, v) for u, v in zip(a.counter_totals(), b.counter_totals()))
    a.close()
    b.close()
