"""Energy histograms per jackknife block on the device (DESIGN.md section 3.17 "Per block"; include/amc.h
amc_energy_histogram_accumulate_blocks .. amc_set_energy_histogram_blocks) against their host twin (tests/ehist_blocks_twin.py:
ehist_twin's cells composed with the block of a ladder), block by block, integer for integer -- no tolerance anywhere.  The twin is
applied to download_state() taken right behind each snapshot.  Shapes: one chain per "ladder" with two and with 64 blocks, chunks
that the ladder count cuts, odd R straddling a wave, R = 64, more blocks than a HIP block has ladders per trip, a grid that is walked
more than four times; the static LDS cell count from both sides; Float32 state and a custom potential (the kernel built at run
time); shards whose offsets cut chunks and a shard in which a block has no ladder; every lifetime of the contract."""
import ctypes as C

import numpy as np
import pytest

from montecarlo_amd import AmcError
from montecarlo_amd.jackknife import block_counts, default_chunk
from montecarlo_amd.system import CustomPotential

import ehist_blocks_twin as KB
import ehist_twin as T

pytestmark = pytest.mark.gpu
CUSTOM = CustomPotential("x*x*x*x - 2.0*x*x + 0.25*x")
LADDER = lambda R: 0.5 * 1.5 ** np.arange(R)
ERR_BAD_ARG, ERR_STATE = -1, -5
BINS = (0.125, 2.5, 200)                # lo, hi, n_bins of most tests: energies below, inside and above
U64P = C.POINTER(C.c_uint64)


def start_state(M, R=0, offset=0):
    ids = np.arange(offset, offset + M)
    x = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)
    return x, (LADDER(R)[ids % R] if R else None)


def make(gpu, M, R=0, *, potential="double_well", dtype="f64", offset=0, n_global=None, seed=23, env=None, blocks=None, **kw):
    mp = pytest.MonkeyPatch()
    for k, v in (env or {}).items():
        mp.setenv(k, v)
    try:
        eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=n_global or offset + M, potential=potential, beta=1.0,
                            sigma=[0.5], weight=[1.0], seed=seed, dtype=dtype, **kw)
    finally:
        mp.undo()
    x0, beta = start_state(M, R, offset)
    eng.upload_state(x0, beta)
    if R:
        eng.set_ladder(R)
    if blocks:
        eng.set_blocks(*blocks)
    return eng


def twin_now(eng, potential, bins, R, part, first=0, dtype="f64"):
    return KB.snapshot(potential, eng.download_state(want_e=False)[0], *bins, max(R, 1), *part, first, dtype == "f32")


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.uint64, (what, got.shape, want.shape, got.dtype)
    if not np.array_equal(got, want):
        where = tuple(int(v) for v in np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: counts differ from the twin, first at (block, group, cell) {where}: {int(got[where])} != {int(want[where])}")


def check_sequence(eng, potential, bins, R, part, what, dtype="f64", first=0):
    """[snapshot; 3 sweeps; snapshot; exchange; snapshot] under the partition ``part``: every block's rows are the sum of the twin's,
    every (b, g) row sums to snapshots x ladders of b, the merged fetch is the sum over the blocks, fetch resets nothing and fetch
    with reset frees the bins and the form."""
    G, L = max(R, 1), eng.n_chains // max(R, 1)
    want = np.zeros((part[0], G, bins[2] + 3), dtype=np.uint64)
    for step in range(3):
        if step == 1:
            eng.sweep(3)
        if step == 2 and R:
            eng.exchange(1)
        eng.energy_histogram_accumulate_blocks(*bins)
        want += twin_now(eng, potential, bins, R, part, first, dtype)
    got, n_snap, got_bins = eng.energy_histogram_fetch_blocks()
    same(got, want, what)
    assert n_snap == 3 and got_bins == (float(bins[0]), float(bins[1]), bins[2])
    per_block = block_counts(L, *part, first)
    assert np.array_equal(per_block, KB.ladders(L, *part, first))
    assert np.array_equal(got.sum(axis=2), np.uint64(3) * np.repeat(per_block.astype(np.uint64)[:, None], G, axis=1))
    merged = eng.energy_histogram_fetch()
    assert np.array_equal(merged[0], got.sum(axis=0, dtype=np.uint64)) and merged[1:] == (3, got_bins)
    assert np.array_equal(merged[0].sum(axis=1), np.full(G, 3 * L, dtype=np.uint64))
    again = eng.energy_histogram_fetch_blocks(reset=True)
    assert np.array_equal(again[0], got) and again[1] == 3
    empty = eng.energy_histogram_fetch()
    assert empty[0].shape == (G, 0) and empty[1] == 0 and empty[2] == (0.0, 0.0, 0)
    with pytest.raises(AmcError, match="no accumulator kept per jackknife block"):
        eng.energy_histogram_fetch_blocks()
    return got


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
def test_fetch_blocks_of_the_smallest_ensemble(gpu):
    """Two chains, two blocks of one chain each: the entry exists, and each block holds its own chain."""
    eng = make(gpu, 2, blocks=(2, 1))
    eng.energy_histogram_accumulate_blocks(*BINS)
    got, n_snap, bins = eng.energy_histogram_fetch_blocks()
    same(got, twin_now(eng, "double_well", BINS, 0, (2, 1)), "two chains")
    assert got.shape == (2, 1, 203) and n_snap == 1 and bins == BINS and got.sum() == 2
    assert np.array_equal(got.sum(axis=(1, 2)), [1, 1])
    eng.close()


@pytest.mark.parametrize("R,L,B,chunk", [(0, 65, 2, 1), (0, 257, 64, 1), (3, 22, 4, 3), (7, 37, 5, 1), (64, 5, 2, 2), (2, 3, 3, 1)])
def test_shapes(gpu, R, L, B, chunk):
    eng = make(gpu, max(R, 1) * L, R, blocks=(B, chunk))
    check_sequence(eng, "double_well", BINS, R, (B, chunk), f"R={R} L={L} B={B} C={chunk}")
    eng.close()


def test_grid_stride(gpu):
    """One block per CU caps the grid (rounded up to a multiple of 64): 100 003 ladders of R = 3 in chunks of 85 are walked several
    times by every HIP block -- four loads in flight, then the rest one by one -- and the last chunk is cut."""
    R, L, B = 3, 100003, 64
    part = (B, default_chunk(R))
    eng = make(gpu, R * L, R, env={"AMC_BLOCKS_PER_CU": "1"})
    eng.set_blocks(B)                                      # chunk 0: the default
    eng.sweep(2)
    eng.energy_histogram_accumulate_blocks(*BINS)
    got, n_snap, _ = eng.energy_histogram_fetch_blocks()
    same(got, twin_now(eng, "double_well", BINS, R, part), "grid stride")
    assert n_snap == 1
    eng.close()


@pytest.mark.parametrize("n_bins", [189, 190])
def test_both_sides_of_the_lds_cell_count(gpu, n_bins):
    """64 rows of 189 + 3 cells are exactly the static LDS array of ONE jackknife block (the per-block path), 64 rows of 190 + 3 one
    row too many: every chain is one global atomic into its block's row."""
    R, L = 64, 3
    eng = make(gpu, R * L, R, blocks=(2, 1))
    check_sequence(eng, "double_well", (0.0, 3.0, n_bins), R, (2, 1), f"bins={n_bins}")
    eng.close()


# ---- 2. the merged fetch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 5])
def test_merged_fetch_is_the_plain_handles(gpu, R):
    M = max(R, 1) * 131
    plain, blocked = make(gpu, M, R), make(gpu, M, R, blocks=(4, 7))
    for i in range(3):
        for eng in (plain, blocked):
            eng.sweep(2)
            if R:
                eng.exchange(1)
        plain.energy_histogram_accumulate(*BINS)
        blocked.energy_histogram_accumulate_blocks(*BINS)
    want, got = plain.energy_histogram_fetch(), blocked.energy_histogram_fetch()
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] and got[1] == 3
    per_block = block_counts(M // max(R, 1), 4, 7).astype(np.uint64)
    rows = blocked.energy_histogram_fetch_blocks()[0].sum(axis=2)
    assert np.array_equal(rows, np.uint64(3) * np.repeat(per_block[:, None], max(R, 1), axis=1))
    plain.close()
    blocked.close()


# ---- 3. state types: the kernel built at run time ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("potential,dtype", [("harmonic", "f32"), (CUSTOM, "f64"), (CUSTOM, "f32")], ids=["harmonic-f32", "custom-f64", "custom-f32"])
def test_float32_state_and_a_custom_potential(gpu, potential, dtype):
    bins = (-1.25, 2.5, 200) if potential is CUSTOM else BINS
    R, L, part = 5, 103, (3, 4)
    eng = make(gpu, R * L, R, potential=potential, dtype=dtype, blocks=part)
    check_sequence(eng, potential, bins, R, part, f"{dtype}", dtype)
    eng.close()


# ---- 4. shards --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 4])
def test_three_shards_add_block_by_block(gpu, R):
    """Chunks of 5 ladders, shards that begin at ladders 64 and 194: both offsets cut a chunk."""
    G, part = max(R, 1), (4, 5)
    M = G * 300
    cuts = [0, G * 64, G * 194, M]
    whole = make(gpu, M, R, seed=31, blocks=part)
    parts = [make(gpu, cuts[i + 1] - cuts[i], R, offset=cuts[i], n_global=M, seed=31, blocks=part) for i in range(3)]
    for eng in [whole] + parts:
        eng.sweep(2)
        eng.energy_histogram_accumulate_blocks(*BINS)
        if R:
            eng.exchange(2)
        eng.sweep(1)
        eng.energy_histogram_accumulate_blocks(*BINS)
    want, n_snap, _ = whole.energy_histogram_fetch_blocks()
    got = [p.energy_histogram_fetch_blocks() for p in parts]
    assert all(g[1] == n_snap == 2 for g in got)
    for i, p in enumerate(parts):                          # every shard holds its own ladders of every block
        rows = got[i][0].sum(axis=2)[:, 0]
        assert np.array_equal(rows, np.uint64(2) * block_counts((cuts[i + 1] - cuts[i]) // G, *part, cuts[i] // G).astype(np.uint64))
    same(np.sum([g[0] for g in got], axis=0).astype(np.uint64), want, f"three shards R={R}")
    for eng in [whole] + parts:
        eng.close()


def test_a_block_without_a_local_ladder_is_a_zero_row(gpu):
    """A shard of 6 ladders that begins at global ladder 8, chunks of 4, 4 blocks: it holds ladders of blocks 2 and 3 alone."""
    R, part, first, L = 3, (4, 4), 8, 6
    eng = make(gpu, R * L, R, offset=R * first, n_global=R * 64, blocks=part)
    per_block = block_counts(L, *part, first)
    assert per_block.tolist() == [0, 0, 4, 2]
    eng.sweep(1)
    eng.energy_histogram_accumulate_blocks(*BINS)
    got, n_snap, _ = eng.energy_histogram_fetch_blocks()
    same(got, twin_now(eng, "double_well", BINS, R, part, first), "shard with empty blocks")
    assert n_snap == 1 and not got[:2].any() and got[2:].any()
    eng.close()


# ---- 5. lifetimes -----------------------------------------------------------------------------------------------------------------------
def test_respacing(gpu):
    """A respacing that is not taken (no exchange attempt yet: status 2) leaves every block's rows; one that is taken (status 0) zeroes
    them all in stream order and keeps the bins and the form."""
    R, part = 4, (4, 3)
    eng = make(gpu, R * 64, R, blocks=part)
    eng.sweep(2)
    eng.energy_histogram_accumulate_blocks(*BINS)
    kept = eng.energy_histogram_fetch_blocks()
    eng.respace_ladder("acceptance", 1.0, 0.01)
    assert eng.respace_status()[0] == 2
    assert np.array_equal(eng.energy_histogram_fetch_blocks()[0], kept[0])
    eng.respace_ladder("acceptance", 0.5, 0.01, counts=[100] * (R - 1) + [30, 50, 70])
    eng.sweep(1)
    eng.energy_histogram_accumulate_blocks(*BINS)          # queued behind the respacing: the only snapshot left
    assert eng.respace_status()[0] == 0
    got = eng.energy_histogram_fetch_blocks()
    assert got[1] == 1 and got[2] == kept[2]
    same(got[0], twin_now(eng, "double_well", BINS, R, part), "behind a respacing")
    eng.close()


def test_set_ladder_clears(gpu):
    eng = make(gpu, 6 * 40, 6, blocks=(2, 3))
    eng.energy_histogram_accumulate_blocks(*BINS)
    eng.set_ladder(3)                                      # (turns the partition off too)
    assert eng.energy_histogram_fetch()[2] == (0.0, 0.0, 0)
    assert eng._lib.amc_energy_histogram_accumulate_blocks(eng._h, *BINS) == ERR_STATE and b"no partition" in eng._lib.amc_last_error()
    eng.set_blocks(5, 2)
    eng.energy_histogram_accumulate_blocks(0.0, 2.0, 9)    # other groups, another partition, other bins
    same(eng.energy_histogram_fetch_blocks()[0], twin_now(eng, "double_well", (0.0, 2.0, 9), 3, (5, 2)), "behind set_ladder")
    eng.close()


@pytest.mark.parametrize("again", [(0, 0), (4, 3), (2, 0)], ids=["off", "same", "other"])
def test_set_blocks_folds_to_a_plain_accumulator(gpu, again):
    R, part = 3, (4, 3)
    eng = make(gpu, R * 70, R, blocks=part)
    eng.sweep(2)
    eng.energy_histogram_accumulate_blocks(*BINS)
    eng.sweep(1)
    eng.energy_histogram_accumulate_blocks(*BINS)
    merged = eng.energy_histogram_fetch()
    eng.set_blocks(*again)                                 # in stream order, nothing is lost: the form becomes plain
    now = eng.energy_histogram_fetch()
    assert np.array_equal(now[0], merged[0]) and now[1:] == merged[1:] and now[1] == 2
    with pytest.raises(gpu.AmcError, match="no accumulator kept per jackknife block"):
        eng.energy_histogram_fetch_blocks()
    if again[0]:
        assert eng._lib.amc_energy_histogram_accumulate_blocks(eng._h, *BINS) == ERR_STATE and b"fetch with reset" in eng._lib.amc_last_error()
    eng.energy_histogram_accumulate(*BINS)                 # ... and goes on as a plain one
    same3 = eng.energy_histogram_fetch()
    assert same3[1] == 3 and np.array_equal(same3[0], merged[0] + T.snapshot("double_well", eng.download_state(want_e=False)[0], *BINS, R))
    eng.close()


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
    R, part = 4, (5, 2)
    eng = make(gpu, R * 50, R)
    lib, h = eng._lib, eng._h
    acc, accb = lib.amc_energy_histogram_accumulate, lib.amc_energy_histogram_accumulate_blocks
    ints = [C.c_int(0) for _ in range(3)]
    lo, hi, ns = C.c_double(0), C.c_double(0), C.c_uint64(0)
    sizes = tuple(C.byref(v) for v in ints) + (C.byref(lo), C.byref(hi), C.byref(ns))
    fetchb = lib.amc_energy_histogram_fetch_blocks
    # without a partition; without an accumulator
    assert accb(h, *BINS) == ERR_STATE and b"no partition" in lib.amc_last_error()
    assert fetchb(h, None, 0, *sizes, 0) == ERR_STATE
    assert lib.amc_set_energy_histogram_blocks(h, *BINS, None, 0, 0) == ERR_STATE
    assert eng.energy_histogram_fetch()[2] == (0.0, 0.0, 0)
    # a plain accumulator stands: the blocked entry is refused, with or without a partition, and leaves it
    eng.sweep(2)
    eng.exchange(1)
    eng.energy_histogram_accumulate(*BINS)
    eng.set_blocks(*part)
    plain = eng.energy_histogram_fetch()
    assert accb(h, *BINS) == ERR_STATE and b"fetch with reset" in lib.amc_last_error()
    assert fetchb(h, None, 0, *sizes, 0) == ERR_STATE
    after = eng.energy_histogram_fetch()
    assert np.array_equal(after[0], plain[0]) and after[1:] == plain[1:]
    eng.energy_histogram_fetch(reset=True)
    # a blocked accumulator stands
    eng.energy_histogram_accumulate_blocks(*BINS)
    before, state = eng.energy_histogram_fetch_blocks(), snapshot_of_everything(eng)
    assert acc(h, *BINS) == ERR_STATE and b"fetch with reset" in lib.amc_last_error()
    assert accb(h, 0.125, 2.5, 199) == ERR_STATE and b"other bins" in lib.amc_last_error()
    assert accb(h, 0.25, 2.5, 200) == ERR_STATE and accb(h, 0.125, 2.75, 200) == ERR_STATE
    for a, b, n in ((0.0, 1.0, 0), (0.0, 1.0, 8193), (1.0, 1.0, 4), (2.0, 1.0, 4), (float("nan"), 1.0, 4), (0.0, float("inf"), 4)):
        assert accb(h, a, b, n) == ERR_BAD_ARG, (a, b, n)
    cells = part[0] * R * 203
    out = np.zeros(cells, dtype=np.uint64)
    assert fetchb(h, out.ctypes.data_as(U64P), cells - 1, *sizes, 1) == ERR_BAD_ARG and b"capacity" in lib.amc_last_error()
    assert fetchb(h, None, 0, *sizes, 1) == 0 and [v.value for v in ints] == [part[0], R, 200] and ns.value == 0      # the sizes alone, nothing reset
    assert fetchb(h, out.ctypes.data_as(U64P), cells, None, *sizes[1:], 0) == ERR_BAD_ARG
    # amc_set_energy_histogram_blocks: a count moved between two blocks (every total of the plain rule still holds), a row one short,
    # an empty block that is not empty would need a shard: see below; another B; a wrong snapshot count
    counts = before[0].copy()
    moved = counts.copy()
    cell = int(np.argmax(moved[0, 0]))
    moved[0, 0, cell] -= np.uint64(1)
    moved[1, 0, cell] += np.uint64(1)
    short = counts.copy()
    short[2, 3, int(np.argmax(short[2, 3]))] -= np.uint64(1)
    for bad in (moved, short):
        with pytest.raises(gpu.AmcError, match="does not sum"):
            eng.set_energy_histogram_blocks(*BINS, bad, 1)
    with pytest.raises(gpu.AmcError, match="does not sum"):
        eng.set_energy_histogram_blocks(*BINS, counts, 2)
    with pytest.raises(gpu.AmcError, match="the partition has 5 blocks"):
        eng.set_energy_histogram_blocks(*BINS, counts[:4], 1)
    with pytest.raises(gpu.AmcError):
        eng.set_energy_histogram_blocks(0.0, 0.0, 200, counts, 1)
    after = eng.energy_histogram_fetch_blocks()
    assert np.array_equal(after[0], before[0]) and after[1:] == before[1:]
    same_everything(snapshot_of_everything(eng), state)
    eng.energy_histogram_accumulate_blocks(*BINS)          # ... and the accumulator goes on
    assert eng.energy_histogram_fetch_blocks()[1] == 2
    eng.close()


def test_the_cell_cap(gpu):
    """64 blocks of 64 rows of 1024 cells are 2^22 cells, the cap; one bin more is refused and leaves nothing behind."""
    R = 64
    eng = make(gpu, R * 64, R, blocks=(64, 1))
    assert eng._lib.amc_energy_histogram_accumulate_blocks(eng._h, 0.0, 3.0, 1022) == ERR_BAD_ARG and b"AMC_EHIST_BLK_MAX_CELLS" in eng._lib.amc_last_error()
    assert eng.energy_histogram_fetch()[2] == (0.0, 0.0, 0)
    eng.energy_histogram_accumulate_blocks(0.0, 3.0, 1021)
    got = eng.energy_histogram_fetch_blocks()[0]
    assert got.shape == (64, 64, 1024) and np.array_equal(got.sum(axis=2), np.ones((64, 64), dtype=np.uint64))
    eng.close()


@pytest.mark.parametrize("R", [0, 5])
def test_set_round_trip_then_one_more_snapshot(gpu, R):
    part = (4, 6)
    a, b = make(gpu, 5 * 61, R, blocks=part), make(gpu, 5 * 61, R, blocks=part)
    a.sweep(2)
    a.energy_histogram_accumulate_blocks(*BINS)
    a.sweep(1)
    a.energy_histogram_accumulate_blocks(*BINS)
    counts, n_snap, bins = a.energy_histogram_fetch_blocks()
    b.upload_state(a.download_state(want_e=False)[0], start_state(5 * 61, R)[1])
    b.step = a.step
    b.set_energy_histogram_blocks(*bins, counts, n_snap)
    back = b.energy_histogram_fetch_blocks()
    assert np.array_equal(back[0], counts) and back[1:] == (n_snap, bins)
    for eng in (a, b):
        eng.sweep(2)
        eng.energy_histogram_accumulate_blocks(*BINS)
    ca, cb = a.energy_histogram_fetch_blocks(), b.energy_histogram_fetch_blocks()
    same(cb[0], ca[0], "restored accumulator")
    assert ca[1] == cb[1] == 3
    b.set_energy_histogram_blocks()                        # None clears
    assert b.energy_histogram_fetch()[2] == (0.0, 0.0, 0)
    b.energy_histogram_accumulate(0.0, 1.0, 7)             # ... and frees the bins and the form
    assert b.energy_histogram_fetch()[0].shape == (max(R, 1), 10)
    a.close()
    b.close()


def test_an_empty_block_must_be_restored_empty(gpu):
    R, part, first, L = 3, (4, 4), 8, 6
    eng = make(gpu, R * L, R, offset=R * first, n_global=R * 64, blocks=part)
    eng.energy_histogram_accumulate_blocks(*BINS)
    counts, n_snap, bins = eng.energy_histogram_fetch_blocks(reset=True)
    bad = counts.copy()
    bad[0, 1, 7] = 1
    with pytest.raises(gpu.AmcError, match="does not sum"):
        eng.set_energy_histogram_blocks(*bins, bad, n_snap)
    assert eng.energy_histogram_fetch()[2] == (0.0, 0.0, 0)
    eng.set_energy_histogram_blocks(*bins, counts, n_snap)
    assert np.array_equal(eng.energy_histogram_fetch_blocks()[0], counts)
    eng.close()


# ---- 6. no disturbance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 4])
def test_a_handle_that_accumulates_ends_as_one_that_never_did(gpu, R):
    a, b = make(gpu, 4 * 129, R, blocks=(4, 5)), make(gpu, 4 * 129, R, blocks=(4, 5))
    for i in range(3):
        for eng in (a, b):
            eng.sweep(3)
            if R:
                eng.exchange(1)
        a.energy_histogram_accumulate_blocks(*BINS)
    a.energy_histogram_fetch_blocks(reset=True)
    for eng in (a, b):
        eng.sweep(2)
    same_everything(snapshot_of_everything(a), snapshot_of_everything(b))
    a.close()
    b.close()
