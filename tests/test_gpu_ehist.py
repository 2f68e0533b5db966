"""Energy histograms on the device (include/amc.h amc_energy_histogram_accumulate .. amc_set_energy_histogram)
against their host twin (tests/ehist_twin.py: the oracle's energies, the bin rule in numpy Float64), integer for integer -- no tolerance
anywhere.  The twin is applied to download_state() taken right behind each snapshot; download_state's bits are pinned by the parity and
exchange tests.  Shapes are the smallest at which the kernel takes another path: one chain, a wave and its neighbours, more than one
block, a grid that is walked more than four times with a ragged tail (four loads in flight, then the tail loop); with a ladder R = 2
with one ladder, odd R straddling a wave and a block, R = 64; one bin and 200; the static LDS cell count (12288 = 64 rows of 189 + 3)
from both sides."""
import ctypes as C

import numpy as np
import pytest

from montecarlo_amd.system import CustomPotential

import ehist_twin as T

pytestmark = pytest.mark.gpu
CUSTOM = CustomPotential("x*x*x*x - 2.0*x*x + 0.25*x")
LADDER = lambda R: 0.5 * 1.5 ** np.arange(R)
ERR_BAD_ARG, ERR_STATE = -1, -5
LDS_CELLS = 12288                       # EHIST_LDS_CELLS of amc_ehist.h
BINS = (0.125, 2.5, 200)                # lo, hi, n_bins of most tests: energies below, inside and above


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


def twin_now(eng, potential, bins, R, dtype="f64"):
    return T.snapshot(potential, eng.download_state(want_e=False)[0], *bins, max(R, 1), dtype == "f32")


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.uint64, (what, got.shape, want.shape, got.dtype)
    if not np.array_equal(got, want):
        g, c = (int(v) for v in np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: counts differ from the twin, first at group {g} cell {c}: {int(got[g, c])} != {int(want[g, c])}")


def check_sequence(eng, potential, bins, R, what, dtype="f64"):
    """[snapshot; 3 sweeps; snapshot; exchange; snapshot]: the accumulator is the sum of the twin's histograms, every row sums to
    snapshots x ladders, fetch resets nothing, fetch with reset frees the bins."""
    G, L = max(R, 1), eng.n_chains // max(R, 1)
    want = np.zeros((G, bins[2] + 3), dtype=np.uint64)
    eng.energy_histogram_accumulate(*bins)
    want += twin_now(eng, potential, bins, R, dtype)
    eng.sweep(3)
    eng.energy_histogram_accumulate(*bins)
    want += twin_now(eng, potential, bins, R, dtype)
    if R:
        eng.exchange(1)
    eng.energy_histogram_accumulate(*bins)
    want += twin_now(eng, potential, bins, R, dtype)
    got, n_snap, got_bins = eng.energy_histogram_fetch()
    same(got, want, what)
    assert n_snap == 3 and got_bins == (float(bins[0]), float(bins[1]), bins[2])
    assert np.array_equal(got.sum(axis=1), np.full(G, 3 * L, dtype=np.uint64))          # the row-sum identity of the contract
    again = eng.energy_histogram_fetch(reset=True)
    assert np.array_equal(again[0], got) and again[1] == 3
    empty = eng.energy_histogram_fetch()
    assert empty[0].shape == (G, 0) and empty[1] == 0 and empty[2] == (0.0, 0.0, 0)
    return got


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
def test_shapes_without_a_ladder(gpu, M):
    eng = make(gpu, M)
    check_sequence(eng, "double_well", BINS, 0, f"M={M}")
    eng.close()


@pytest.mark.parametrize("n_bins", [1, 200])
@pytest.mark.parametrize("R,L", [(2, 1), (3, 22), (7, 37), (64, 5)])
def test_shapes_with_a_ladder(gpu, R, L, n_bins):
    eng = make(gpu, R * L, R)
    check_sequence(eng, "double_well", (0.125, 2.5, n_bins), R, f"R={R} L={L} bins={n_bins}")
    eng.close()


@pytest.mark.parametrize("M,R", [(300011, 0), (3 * 100003, 3)])
def test_grid_stride(gpu, M, R):
    """One block per CU caps the histogram's grid at 65 536 threads: 300 011 chains walk it five times -- four loads in flight, then
    the tail loop -- and end ragged; with R = 3 a trip is 21 845 ladders and the last threads of the grid hold none."""
    eng = make(gpu, M, R, env={"AMC_BLOCKS_PER_CU": "1"})
    bins = BINS
    eng.sweep(2)
    eng.energy_histogram_accumulate(*bins)
    got, n_snap, _ = eng.energy_histogram_fetch()
    same(got, twin_now(eng, "double_well", bins, R), f"M={M} R={R}")
    assert n_snap == 1
    eng.close()


@pytest.mark.parametrize("R,L,n_bins", [(64, 3, 189), (64, 3, 190), (0, 257, 8192), (3, 85, 8192)])
def test_both_sides_of_the_lds_cell_count(gpu, R, L, n_bins):
    """64 rows of 189 + 3 cells are exactly the static LDS array (the per-block path), 64 rows of 190 + 3 one row too many (one global
    atomic per chain); the largest single row fits, three of them do not."""
    cells = max(R, 1) * (n_bins + 3)
    assert (cells <= LDS_CELLS) == ((R, n_bins) in ((64, 189), (0, 8192)))
    eng = make(gpu, max(R, 1) * L, R)
    check_sequence(eng, "double_well", (0.0, 3.0, n_bins), R, f"R={R} bins={n_bins} cells={cells}")
    eng.close()


# ---- 2. models and state types ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("potential", ["harmonic", "double_well", CUSTOM], ids=["harmonic", "double_well", "custom"])
def test_models_and_float32_state(gpu, potential, dtype):
    bins = (-1.25, 2.5, 200) if potential is CUSTOM else BINS
    for R, L in ((0, 257), (5, 103)):
        eng = make(gpu, L * max(R, 1), R, potential=potential, dtype=dtype)
        check_sequence(eng, potential, bins, R, f"{dtype} R={R}", dtype)
        eng.close()


def test_global_path_with_float32_state(gpu):
    eng = make(gpu, 3 * 85, 3, potential="harmonic", dtype="f32")
    check_sequence(eng, "harmonic", (0.0, 3.0, 8192), 3, "f32 global path", "f32")
    eng.close()


# ---- 3. planted positions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("R", [0, 3])
def test_planted_positions(gpu, R, dtype):
    """NaN, +-Inf, 10^200 (e = +Inf; Float32 state: x itself narrows to +Inf), and positions whose energy is exactly lo (bin 0) and
    exactly hi (the ">= hi" cell): harmonic e = x x, 0.5^2 = 0.25, 1.5^2 = 2.25, exact in both state types."""
    M = 3 * 43
    x, _ = start_state(M, R)
    plant = {4: np.nan, 5: np.inf, 6: -np.inf, 7: 1e200, 8: 0.5, 9: -0.5, 10: 1.5, 11: -1.5, 12: -0.0}
    for i, v in plant.items():
        x[i] = v
    lo, hi, n = 0.25, 2.25, 16
    eng = make(gpu, M, R, potential="harmonic", dtype=dtype, x=x)
    eng.energy_histogram_accumulate(lo, hi, n)
    got, n_snap, _ = eng.energy_histogram_fetch()
    same(got, twin_now(eng, "harmonic", (lo, hi, n), R, dtype), f"planted R={R} {dtype}")
    G = max(R, 1)
    alone = np.zeros((G, n + 3), dtype=np.uint64)          # the planted chains alone, cell by cell, from the text of the rule
    for i, cell in {4: n + 2, 5: n + 1, 6: n + 1, 7: n + 1, 8: 0, 9: 0, 10: n + 1, 11: n + 1, 12: n}.items():
        alone[i % G, cell] += 1
    rest = np.delete(np.arange(M), list(plant))
    e_rest = T.energies("harmonic", eng.download_state(want_e=False)[0][rest], dtype == "f32")
    for g in range(G):
        alone[g] += np.bincount(T.cells(e_rest[rest % G == g], lo, hi, n), minlength=n + 3).astype(np.uint64)
    same(got, alone, "planted cells")
    assert n_snap == 1
    eng.close()


# ---- 4. shards, the checkpoint pair -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 4])
def test_three_shards_add_to_the_single_handle(gpu, R):
    G = max(R, 1)
    M = G * 300
    cuts = [0, G * 64, G * 194, M]                       # (shards split on chain pairs)
    whole = make(gpu, M, R, seed=31)
    parts = [make(gpu, cuts[i + 1] - cuts[i], R, offset=cuts[i], n_global=M, seed=31) for i in range(3)]
    for eng in [whole] + parts:
        eng.sweep(2)
        eng.energy_histogram_accumulate(*BINS)
        if R:
            eng.exchange(2)
        eng.sweep(1)
        eng.energy_histogram_accumulate(*BINS)
    want, n_snap, _ = whole.energy_histogram_fetch()
    got = [p.energy_histogram_fetch() for p in parts]
    assert all(g[1] == n_snap == 2 for g in got)
    same(np.sum([g[0] for g in got], axis=0).astype(np.uint64), want, f"three shards R={R}")
    for eng in [whole] + parts:
        eng.close()


@pytest.mark.parametrize("R", [0, 5])
def test_set_round_trip_then_one_more_snapshot(gpu, R):
    a, b = make(gpu, 5 * 61, R), make(gpu, 5 * 61, R)
    a.sweep(2)
    a.energy_histogram_accumulate(*BINS)
    a.sweep(1)
    a.energy_histogram_accumulate(*BINS)
    counts, n_snap, bins = a.energy_histogram_fetch()
    b.upload_state(a.download_state(want_e=False)[0], start_state(5 * 61, R)[1])
    b.step = a.step
    b.set_energy_histogram(*bins, counts, n_snap)
    back = b.energy_histogram_fetch()
    assert np.array_equal(back[0], counts) and back[1:] == (n_snap, bins)
    for eng in (a, b):
        eng.sweep(2)
        eng.energy_histogram_accumulate(*BINS)
    ca, cb = a.energy_histogram_fetch(), b.energy_histogram_fetch()
    same(cb[0], ca[0], "restored accumulator")
    assert ca[1] == cb[1] == 3
    b.set_energy_histogram()                               # None clears
    assert b.energy_histogram_fetch()[2] == (0.0, 0.0, 0)
    b.energy_histogram_accumulate(0.0, 1.0, 7)             # ... and frees the bins
    assert b.energy_histogram_fetch()[0].shape == (max(R, 1), 10)
    a.close()
    b.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def snapshot_of_everything(eng):
    x, e = eng.download_state()
    acc, tot = eng.counter_totals()
    out = dict(x=x.copy(), e=e.copy(), acc=np.array(acc), tot=np.array(tot), step=eng.step, est=eng.estimator_step)
    if eng.n_rungs:
        out.update(xstep=eng.exchange_step, gaps=np.concatenate([np.ravel(v) for v in eng.exchange_counters()]))
    return out


def same_everything(a, b):
    assert a.keys() == b.keys()
    for k in a:
        va, vb = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(va.view(np.uint64) if va.dtype == np.float64 else va, vb.view(np.uint64) if vb.dtype == np.float64 else vb), k


def test_refusals_change_nothing(gpu):
    eng = make(gpu, 4 * 50, 4)
    lib, h = eng._lib, eng._h
    eng.sweep(2)
    eng.exchange(1)
    eng.energy_histogram_accumulate(*BINS)
    before, state = eng.energy_histogram_fetch(), snapshot_of_everything(eng)
    acc = lib.amc_energy_histogram_accumulate
    assert acc(h, 0.125, 2.5, 199) == ERR_STATE and b"other bins" in lib.amc_last_error()
    assert acc(h, 0.25, 2.5, 200) == ERR_STATE and acc(h, 0.125, 2.75, 200) == ERR_STATE
    for lo, hi, n in ((0.0, 1.0, 0), (0.0, 1.0, 8193), (1.0, 1.0, 4), (2.0, 1.0, 4), (float("nan"), 1.0, 4), (0.0, float("inf"), 4)):
        assert acc(h, lo, hi, n) == ERR_BAD_ARG, (lo, hi, n)
    out = np.zeros(4 * 203, dtype=np.uint64)
    ng, nb, lo, hi, ns = C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0), C.c_uint64(0)
    args = (C.byref(ng), C.byref(nb), C.byref(lo), C.byref(hi), C.byref(ns))
    fetch = lib.amc_energy_histogram_fetch
    assert fetch(h, out.ctypes.data_as(C.POINTER(C.c_uint64)), 4 * 203 - 1, *args, 1) == ERR_BAD_ARG and b"capacity" in lib.amc_last_error()
    assert fetch(h, None, 0, *args, 1) == 0 and (ng.value, nb.value, ns.value) == (4, 200, 0)      # NULL counts: the sizes alone, nothing reset
    assert fetch(h, out.ctypes.data_as(C.POINTER(C.c_uint64)), 4 * 203, None, *args[1:], 0) == ERR_BAD_ARG
    # amc_set_energy_histogram: one row one count short, one row one count long, a total that is no multiple of the ladders
    counts = before[0].copy()
    short, long = counts.copy(), counts.copy()
    short[0, int(np.argmax(short[0]))] -= np.uint64(1)
    long[3, 5] += np.uint64(1)
    for bad in (short, long):
        with pytest.raises(gpu.AmcError, match="does not sum"):
            eng.set_energy_histogram(*BINS, bad, 1)
    with pytest.raises(gpu.AmcError, match="does not sum"):
        eng.set_energy_histogram(*BINS, counts, 2)
    with pytest.raises(gpu.AmcError):
        eng.set_energy_histogram(0.0, 0.0, 200, counts, 1)
    after = eng.energy_histogram_fetch()
    assert np.array_equal(after[0], before[0]) and after[1:] == before[1:]
    same_everything(snapshot_of_everything(eng), state)
    eng.energy_histogram_accumulate(*BINS)                 # ... and the accumulator goes on
    assert eng.energy_histogram_fetch()[1] == 2
    eng.close()


# ---- 6. what clears it, what keeps it ---------------------------------------------------------------------------------------------------
def test_set_ladder_clears(gpu):
    eng = make(gpu, 6 * 40, 6)
    eng.energy_histogram_accumulate(*BINS)
    eng.set_ladder(3)
    assert eng.energy_histogram_fetch()[2] == (0.0, 0.0, 0)
    eng.energy_histogram_accumulate(0.0, 2.0, 9)           # other groups, other bins
    got = eng.energy_histogram_fetch()
    same(got[0], twin_now(eng, "double_well", (0.0, 2.0, 9), 3), "behind set_ladder")
    eng.set_ladder(0)
    assert eng.energy_histogram_fetch()[0].shape == (1, 0)
    eng.close()


def test_respacing(gpu):
    """A respacing that is not taken (no exchange attempt yet: status 2) leaves the cells; one that is taken (status 0) zeroes them in
    stream order and keeps the bins."""
    R = 4
    eng = make(gpu, R * 64, R)
    eng.sweep(2)
    eng.energy_histogram_accumulate(*BINS)
    kept = eng.energy_histogram_fetch()
    eng.respace_ladder("acceptance", 1.0, 0.01)
    assert eng.respace_status()[0] == 2
    assert np.array_equal(eng.energy_histogram_fetch()[0], kept[0])
    eng.respace_ladder("acceptance", 0.5, 0.01, counts=[100] * (R - 1) + [30, 50, 70])
    eng.sweep(1)
    eng.energy_histogram_accumulate(*BINS)                 # queued behind the respacing: the only snapshot left
    assert eng.respace_status()[0] == 0
    got = eng.energy_histogram_fetch()
    assert got[1] == 1 and got[2] == kept[2]
    same(got[0], twin_now(eng, "double_well", BINS, R), "behind a respacing")
    assert eng._lib.amc_energy_histogram_accumulate(eng._h, 0.0, 1.0, 5) == ERR_STATE          # the bins stay fixed
    eng.close()


def test_what_leaves_it_alone(gpu):
    R = 3
    eng = make(gpu, R * 70, R, per_chain_counters=True)
    eng.sweep(2)
    eng.energy_histogram_accumulate(*BINS)
    kept = eng.energy_histogram_fetch()
    x, beta = start_state(R * 70, R)
    eng.upload_state(x[::-1].copy(), beta)
    eng.set_blocks(2)
    eng.set_rung_sigma(np.full((1, R), 0.4))
    eng.sweep(4)
    eng.tune_rung_sigma(0.44, 1.0, 1)
    eng.exchange(2)
    eng.init_uniform(-1.0, 1.0)
    now = eng.energy_histogram_fetch()
    assert np.array_equal(now[0], kept[0]) and now[1:] == kept[1:]
    eng.close()
    flat = make(gpu, 257)                                  # no ladder: amc_anneal and amc_set_beta leave it alone too
    flat.energy_histogram_accumulate(*BINS)
    kept = flat.energy_histogram_fetch()
    flat.anneal(1.25)
    flat.beta = 1.5
    now = flat.energy_histogram_fetch()
    assert np.array_equal(now[0], kept[0]) and now[1:] == kept[1:]
    flat.energy_histogram_accumulate(*BINS)
    same(flat.energy_histogram_fetch()[0], kept[0] + twin_now(flat, "double_well", BINS, 0), "behind anneal")
    flat.close()


# ---- 7. no disturbance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 4])
def test_a_handle_that_accumulates_ends_as_one_that_never_did(gpu, R):
    a, b = make(gpu, 4 * 129, R), make(gpu, 4 * 129, R)
    for i in range(3):
        for eng in (a, b):
            eng.sweep(3)
            if R:
                eng.exchange(1)
        a.energy_histogram_accumulate(*BINS)
    a.energy_histogram_fetch(reset=True)
    for eng in (a, b):
        eng.sweep(2)
    same_everything(snapshot_of_everything(a), snapshot_of_everything(b))
    a.close()
    b.close()
