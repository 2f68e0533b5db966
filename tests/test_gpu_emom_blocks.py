"""Moments per energy bin per jackknife block on the device (DESIGN.md section 3.17 "Moments per block"; include/amc.h
amc_energy_moments_accumulate_blocks .. amc_set_energy_moments_blocks) against their host twin (tests/emom_blocks_twin.py: emom_twin's
rule per chain composed with the block of a ladder), block by block, integer for integer -- counts AND sums, no tolerance anywhere.
The twin is applied to download_state() taken right behind each snapshot.  Shapes: one chain per "ladder" with two and with 64
blocks, chunks that the ladder count cuts, odd R straddling a wave, R = 64, more blocks than a HIP block has ladders per trip, a grid
that is walked more than four times; the static LDS word count from both sides for one column and for three; every column choice;
Float32 state and a custom potential (the kernel built at run time); planted positions in known blocks; shards whose offsets cut
chunks and a shard in which a block has no ladder; every lifetime of the contract."""
import ctypes as C

import numpy as np
import pytest

from montecarlo_amd import AmcError
from montecarlo_amd.jackknife import block_counts, default_chunk
from montecarlo_amd.system import CustomPotential

import emom_blocks_twin as EB
import emom_twin as E

pytestmark = pytest.mark.gpu
CUSTOM = CustomPotential("x*x*x*x - 2.0*x*x + 0.25*x")
LADDER = lambda R: 0.5 * 1.5 ** np.arange(R)
ERR_BAD_ARG, ERR_STATE = -1, -5
LDS_WORDS = 12288                       # EHIST_LDS_CELLS of amc_ehist.h
MAX_WORDS = 4194304                     # AMC_EMOM_BLK_MAX_WORDS of include/amc.h
ALL = E.X | E.XX | E.POS
FORM = (0.125, 2.5, 200, ALL, 1.5)      # lo, hi, n_bins, mask, x_bound of most tests: energies below, inside and above the bins, and
                                        # binned chains beyond the bound (the double well at 1.5 < |x| < 1.6 has e < 2.5)


def start_state(M, R=0, offset=0):
    ids = np.arange(offset, offset + M)
    x = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)
    return x, (LADDER(R)[ids % R] if R else None)


def make(gpu, M, R=0, *, potential="double_well", dtype="f64", offset=0, n_global=None, seed=23, env=None, blocks=None, x=None, **kw):
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
    if blocks:
        eng.set_blocks(*blocks)
    return eng


def twin_now(eng, potential, form, R, part, first=0, dtype="f64"):
    return EB.snapshot(potential, eng.download_state(want_e=False)[0], *form, max(R, 1), *part, first, dtype == "f32")


def same(got, want, what=""):
    """(counts, sums) against the twin's, as integers."""
    for name, g, w, dt in (("counts", got[0], want[0], np.uint64), ("sums", got[1], want[1], np.int64)):
        assert g.shape == w.shape and g.dtype == dt, (what, name, g.shape, w.shape, g.dtype)
        if not np.array_equal(g, w):
            at = tuple(int(v) for v in np.argwhere(g != w)[0])
            raise AssertionError(f"{what}: {name} differ from the twin, first at {at}: {int(g[at])} != {int(w[at])}")


def check_sequence(eng, potential, form, R, part, what, dtype="f64", first=0, plain=None):
    """[snapshot; 3 sweeps; snapshot; exchange; snapshot] under the partition ``part``: every block's cells are the sum of the twin's,
    every (b, g) count row sums to snapshots x ladders of b, the merged fetch is the sum over the blocks -- and the plain fetch of
    ``plain``, a handle without blocks taken through the same run --, fetch resets nothing and fetch with reset frees the form."""
    G, L, n = max(R, 1), eng.n_chains // max(R, 1), form[2]
    cols = bin(form[3]).count("1")
    want = [np.zeros((part[0], G, n + 4), dtype=np.uint64), np.zeros((part[0], G, cols, n), dtype=np.int64)]
    for step in range(3):
        for e in (eng, plain):
            if e is None:
                continue
            if step == 1:
                e.sweep(3)
            if step == 2:
                e.exchange(1) if R else e.sweep(1)
        eng.energy_moments_accumulate_blocks(*form)
        if plain is not None:
            plain.energy_moments_accumulate(*form)
        c, s = twin_now(eng, potential, form, R, part, first, dtype)
        want[0] += c
        want[1] += s
    counts, sums, n_snap, got_form = eng.energy_moments_fetch_blocks()
    same((counts, sums), want, what)
    assert n_snap == 3 and got_form == (float(form[0]), float(form[1]), n, form[3], float(form[4]))
    per_block = block_counts(L, *part, first)
    assert np.array_equal(counts.sum(axis=2), np.uint64(3) * np.repeat(per_block.astype(np.uint64)[:, None], G, axis=1))
    merged = eng.energy_moments_fetch()
    assert np.array_equal(merged[0], counts.sum(axis=0, dtype=np.uint64)) and np.array_equal(merged[1], sums.sum(axis=0, dtype=np.int64))
    assert merged[2:] == (3, got_form)
    if plain is not None:
        alone = plain.energy_moments_fetch()
        assert np.array_equal(merged[0], alone[0]) and np.array_equal(merged[1], alone[1]) and merged[2:] == alone[2:]
    again = eng.energy_moments_fetch_blocks(reset=True)
    assert np.array_equal(again[0], counts) and np.array_equal(again[1], sums) and again[2] == 3
    empty = eng.energy_moments_fetch()
    assert empty[0].shape == (G, 0) and empty[2] == 0 and empty[3] == (0.0, 0.0, 0, 0, 0.0)
    with pytest.raises(AmcError, match="no accumulator kept per jackknife block"):
        eng.energy_moments_fetch_blocks()
    return counts, sums


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
def test_fetch_blocks_of_the_smallest_ensemble(gpu):
    """Two chains, two blocks of one chain each: the entries exist, and each block holds its own chain."""
    eng = make(gpu, 2, blocks=(2, 1))
    eng.energy_moments_accumulate_blocks(*FORM)
    counts, sums, n_snap, form = eng.energy_moments_fetch_blocks()
    same((counts, sums), twin_now(eng, "double_well", FORM, 0, (2, 1)), "two chains")
    assert counts.shape == (2, 1, 204) and sums.shape == (2, 1, 3, 200) and n_snap == 1 and form == FORM
    assert np.array_equal(counts.sum(axis=(1, 2)), [1, 1])
    eng.close()


@pytest.mark.parametrize("R,L,B,chunk", [(0, 65, 2, 1), (0, 257, 64, 1), (3, 22, 4, 3), (7, 37, 5, 1), (64, 5, 2, 2), (2, 3, 3, 1)])
def test_shapes(gpu, R, L, B, chunk):
    eng, plain = make(gpu, max(R, 1) * L, R, blocks=(B, chunk)), make(gpu, max(R, 1) * L, R)
    check_sequence(eng, "double_well", FORM, R, (B, chunk), f"R={R} L={L} B={B} C={chunk}", plain=plain)
    eng.close()
    plain.close()


def test_grid_stride(gpu):
    """One block per CU caps the grid (rounded up to a multiple of 64): 100 003 ladders of R = 3 in chunks of 85 are walked several
    times by every HIP block -- four loads in flight, then the rest one by one -- and the last chunk is cut."""
    R, L, B = 3, 100003, 64
    part = (B, default_chunk(R))
    eng = make(gpu, R * L, R, env={"AMC_BLOCKS_PER_CU": "1"})
    eng.set_blocks(B)                                      # chunk 0: the default
    eng.sweep(2)
    eng.energy_moments_accumulate_blocks(*FORM)
    counts, sums, n_snap, _ = eng.energy_moments_fetch_blocks()
    same((counts, sums), twin_now(eng, "double_well", FORM, R, part), "grid stride")
    assert n_snap == 1
    assert counts[:, :, FORM[2] + 3].sum() > 0 and counts[:, :, :FORM[2]].sum() > 0          # the form does put chains beyond the bound
    eng.close()


@pytest.mark.parametrize("mask,n_bins", [(E.XX, 62), (E.XX, 63), (ALL, 26), (ALL, 27)])
def test_both_sides_of_the_lds_word_count(gpu, mask, n_bins):
    """G = 64, the words of ONE jackknife block: one column takes 64 (n + 4) + 128 n -- 12160 at 62 bins (the per-block path), 12352
    at 63 (a global atomic per deposit into the block's set); three columns take 64 (n + 4) + 384 n -- 11904 at 26, 12352 at 27."""
    G, cols = 64, bin(mask).count("1")
    words = G * (n_bins + 4) + 2 * cols * G * n_bins
    assert (words <= LDS_WORDS) == (n_bins in (62, 26))
    eng = make(gpu, G * 3, G, blocks=(2, 1))
    check_sequence(eng, "double_well", (0.0, 3.0, n_bins, mask, 1.5), G, (2, 1), f"mask={mask} bins={n_bins} words={words}")
    eng.close()


@pytest.mark.parametrize("mask", [E.X, E.XX, E.X | E.XX, E.POS, E.X | E.POS, E.XX | E.POS, ALL])
def test_every_column_choice_keeps_its_columns_in_bit_order(gpu, mask):
    eng = make(gpu, 5 * 41, 5, blocks=(3, 4))
    check_sequence(eng, "double_well", (0.125, 2.5, 50, mask, 1.5), 5, (3, 4), f"mask={mask}")
    eng.close()


# ---- 2. models and state types ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("potential,dtype", [("harmonic", "f64"), ("harmonic", "f32"), (CUSTOM, "f64"), (CUSTOM, "f32")],
                         ids=["harmonic-f64", "harmonic-f32", "custom-f64", "custom-f32"])
def test_models_and_float32_state(gpu, potential, dtype):
    """A built-in potential and one compiled at run time (every kernel of a Float32 handle is), a non-power-of-two bound."""
    form = (-1.25, 2.5, 200, ALL, 1.45) if potential is CUSTOM else (0.125, 2.5, 200, ALL, 1.45)
    R, L, part = 5, 103, (3, 4)
    eng = make(gpu, R * L, R, potential=potential, dtype=dtype, blocks=part)
    check_sequence(eng, potential, form, R, part, f"{dtype}", dtype)
    eng.close()


def test_global_path_with_float32_state(gpu):
    eng = make(gpu, 3 * 85, 3, potential="harmonic", dtype="f32", blocks=(4, 5))
    check_sequence(eng, "harmonic", (0.0, 3.0, 8192, ALL, 1.5), 3, (4, 5), "f32 global path", "f32")
    eng.close()


# ---- 3. planted positions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("R", [0, 3])
def test_planted_positions(gpu, R, dtype):
    """Harmonic e = x x on [0.25, 2.25) with x_bound = 1.25, B = 3 blocks of chunk 2: NaN (the NaN cell, no sum), +-Inf and 10^200
    (e = +Inf: at or above hi), +-0.5 (e = lo: bin 0), +-1.5 (e = hi), -0.0 (below lo), +-1.25 (the bound itself: inside), +-1.375
    (e = 1.890625 inside the bins, |x| beyond the bound: the fourth cell, no sum) -- each in the block the rule gives its ladder:
    chain i is ladder i div G, block (ladder div 2) mod 3.  All exact in both state types."""
    M, part = 3 * 43, (3, 2)
    G = max(R, 1)
    x, _ = start_state(M, R)
    x = np.clip(x, -1.2, 1.2)                              # (the rest stays inside the bound)
    plant = {4: np.nan, 5: np.inf, 6: -np.inf, 7: 1e200, 8: 0.5, 9: -0.5, 10: 1.5, 11: -1.5, 12: -0.0, 13: 1.25, 14: -1.25, 15: 1.375, 16: -1.375}
    for i, v in plant.items():
        x[i] = v
    lo, hi, n, x_bound = 0.25, 2.25, 16, 1.25
    form = (lo, hi, n, ALL, x_bound)
    eng = make(gpu, M, R, potential="harmonic", dtype=dtype, x=x, blocks=part)
    eng.energy_moments_accumulate_blocks(*form)
    counts, sums, n_snap, _ = eng.energy_moments_fetch_blocks()
    same((counts, sums), twin_now(eng, "harmonic", form, R, part, 0, dtype), f"planted R={R} {dtype}")
    assert n_snap == 1
    # the planted chains alone, cell by cell and block by block, from the text of the rule
    cell_of = {4: n + 2, 5: n + 1, 6: n + 1, 7: n + 1, 8: 0, 9: 0, 10: n + 1, 11: n + 1, 12: n, 13: 10, 14: 10, 15: n + 3, 16: n + 3}
    block = lambda i: ((i // G) // part[1]) % part[0]
    xs = eng.download_state(want_e=False)[0]
    want_c = np.zeros((part[0], G, n + 4), dtype=np.uint64)
    want_s = np.zeros((part[0], G, 3, n), dtype=np.int64)
    e_x, e_xx = E.exponents(x_bound)
    for i in range(M):
        if i in plant:
            continue
        c1, s1 = E.snapshot("harmonic", xs[i:i + 1], *form, 1, dtype == "f32")
        assert c1[0, n + 2] == 0 and c1[0, n + 3] == 0    # (of the rest, nothing is NaN or beyond the bound)
        want_c[block(i), i % G] += c1[0]
        want_s[block(i), i % G] += s1[0]
    for i, cell in cell_of.items():
        want_c[block(i), i % G, cell] += 1
        if cell < n:                                       # +-0.5 into bin 0, +-1.25 into bin 10: x in quanta of 2^(1 - 32), x^2 of 2^(2 - 32)
            v = plant[i]
            want_s[block(i), i % G, 0, cell] += int(round(v * 2.0 ** -e_x))
            want_s[block(i), i % G, 1, cell] += int(round(v * v * 2.0 ** -e_xx))
            want_s[block(i), i % G, 2, cell] += 1 if v > 0 else 0
    same((counts, sums), (want_c, want_s), "planted cells")
    assert counts[:, :, n + 3].sum() == 2 and counts[:, :, n + 2].sum() == 1
    eng.close()


# ---- 4. grids and shards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 4])
def test_two_grids_and_two_shards_hold_the_same_integers(gpu, R):
    """Chunks of 5 ladders and a shard that begins at ladder 514: the offset cuts a chunk."""
    G, part = max(R, 1), (4, 5)
    M = G * 1300
    cut = G * 514
    whole = make(gpu, M, R, seed=31, blocks=part)
    small = make(gpu, M, R, seed=31, env={"AMC_BLOCKS_PER_CU": "1"}, blocks=part)
    parts = [make(gpu, cut, R, offset=0, n_global=M, seed=31, blocks=part), make(gpu, M - cut, R, offset=cut, n_global=M, seed=31, blocks=part)]
    for eng in [whole, small] + parts:
        eng.sweep(2)
        eng.energy_moments_accumulate_blocks(*FORM)
        if R:
            eng.exchange(2)
        eng.sweep(1)
        eng.energy_moments_accumulate_blocks(*FORM)
    want = whole.energy_moments_fetch_blocks()
    other = small.energy_moments_fetch_blocks()
    same(other[:2], want[:2], f"another grid R={R}")
    got = [p.energy_moments_fetch_blocks() for p in parts]
    assert all(g[2] == want[2] == 2 for g in got) and other[2] == 2
    for p, g, first in zip(parts, got, (0, 514)):          # every shard holds its own ladders of every block
        assert np.array_equal(g[0].sum(axis=2)[:, 0], np.uint64(2) * block_counts(p.n_chains // G, *part, first).astype(np.uint64))
    same((got[0][0] + got[1][0], got[0][1] + got[1][1]), want[:2], f"two shards R={R}")
    for eng in [whole, small] + parts:
        eng.close()


def test_a_block_without_a_local_ladder_is_a_zero_set(gpu):
    """A shard of 6 ladders that begins at global ladder 8, chunks of 4, 4 blocks: it holds ladders of blocks 2 and 3 alone, and the
    snapshot count comes from block 2."""
    R, part, first, L = 3, (4, 4), 8, 6
    eng = make(gpu, R * L, R, offset=R * first, n_global=R * 64, blocks=part)
    assert block_counts(L, *part, first).tolist() == [0, 0, 4, 2]
    eng.sweep(1)
    eng.energy_moments_accumulate_blocks(*FORM)
    counts, sums, n_snap, form = eng.energy_moments_fetch_blocks()
    same((counts, sums), twin_now(eng, "double_well", FORM, R, part, first), "shard with empty blocks")
    assert n_snap == 1 and not counts[:2].any() and not sums[:2].any() and counts[2:].any()
    # ... and an empty block must be restored empty
    bad = counts.copy()
    bad[0, 1, 7] = 1
    with pytest.raises(AmcError, match="does not sum"):
        eng.set_energy_moments_blocks(*form, bad, sums, n_snap)
    eng.set_energy_moments_blocks(*form, counts, sums, n_snap)
    back = eng.energy_moments_fetch_blocks()
    assert np.array_equal(back[0], counts) and np.array_equal(back[1], sums) and back[2] == 1
    eng.close()


# ---- 5. lifetimes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 5])
def test_set_round_trip_then_one_more_snapshot(gpu, R):
    part = (4, 6)
    a, b = make(gpu, 5 * 61, R, blocks=part), make(gpu, 5 * 61, R, blocks=part)
    a.sweep(2)
    a.energy_moments_accumulate_blocks(*FORM)
    a.sweep(1)
    a.energy_moments_accumulate_blocks(*FORM)
    counts, sums, n_snap, form = a.energy_moments_fetch_blocks()
    b.upload_state(a.download_state(want_e=False)[0], start_state(5 * 61, R)[1])
    b.step = a.step
    b.set_energy_moments_blocks(*form, counts, sums, n_snap)
    back = b.energy_moments_fetch_blocks()
    assert np.array_equal(back[0], counts) and np.array_equal(back[1], sums) and back[2:] == (n_snap, form)
    for eng in (a, b):
        eng.sweep(2)
        eng.energy_moments_accumulate_blocks(*FORM)
    ca, cb = a.energy_moments_fetch_blocks(), b.energy_moments_fetch_blocks()
    same(cb[:2], ca[:2], "restored accumulator")
    assert ca[2] == cb[2] == 3
    b.set_energy_moments_blocks()                          # None clears
    assert b.energy_moments_fetch()[3] == (0.0, 0.0, 0, 0, 0.0)
    b.energy_moments_accumulate(0.0, 1.0, 7, E.X, 2.0)     # ... and frees the form, plain or per block
    got = b.energy_moments_fetch()
    assert got[0].shape == (max(R, 1), 11) and got[1].shape == (max(R, 1), 1, 7)
    # amc_set_energy_moments replaces a blocked accumulator by a plain one
    merged = a.energy_moments_fetch()
    a.set_energy_moments(*merged[3], merged[0], merged[1], merged[2])
    with pytest.raises(AmcError, match="no accumulator kept per jackknife block"):
        a.energy_moments_fetch_blocks()
    now = a.energy_moments_fetch()
    assert np.array_equal(now[0], merged[0]) and np.array_equal(now[1], merged[1]) and now[2:] == merged[2:]
    a.close()
    b.close()


def fetch_sizes():
    v = [C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0), C.c_int(0), C.c_double(0), C.c_uint64(0)]
    return tuple(C.byref(x) for x in v), lambda: tuple(x.value for x in v)


def test_a_refused_first_call_leaves_nothing_allocated(gpu):
    eng = make(gpu, 4 * 50, 4)
    lib, h = eng._lib, eng._h
    accb = lib.amc_energy_moments_accumulate_blocks
    args, values = fetch_sizes()
    # without a partition; without an accumulator
    assert accb(h, *FORM) == ERR_STATE and b"no partition" in lib.amc_last_error()
    assert lib.amc_energy_moments_fetch_blocks(h, None, None, 0, 0, *args, 0) == ERR_STATE
    assert lib.amc_set_energy_moments_blocks(h, *FORM, None, None, 0, 0) == ERR_STATE
    eng.set_blocks(5, 2)
    assert accb(h, 0.125, 2.5, 200, 0, 1.5) == ERR_BAD_ARG and b"mask" in lib.amc_last_error()
    assert accb(h, 0.125, 2.5, 200, 8, 1.5) == ERR_BAD_ARG and accb(h, 0.125, 2.5, 200, -1, 1.5) == ERR_BAD_ARG
    for bound in (0.0, -1.5, float("nan"), float("inf"), -float("inf"), 5e-324, 2.0 ** 500):
        assert accb(h, 0.125, 2.5, 200, ALL, bound) == ERR_BAD_ARG and b"x_bound" in lib.amc_last_error(), bound
    for lo, hi, n in ((0.0, 1.0, 0), (0.0, 1.0, 8193), (1.0, 1.0, 4), (2.0, 1.0, 4), (float("nan"), 1.0, 4), (0.0, float("inf"), 4)):
        assert accb(h, lo, hi, n, ALL, 1.5) == ERR_BAD_ARG, (lo, hi, n)
    assert lib.amc_energy_moments_fetch_blocks(h, None, None, 0, 0, *args, 0) == ERR_STATE
    assert eng.energy_moments_fetch()[3] == (0.0, 0.0, 0, 0, 0.0)
    eng.energy_moments_accumulate_blocks(0.0, 1.0, 3, E.POS, 1.0)    # any form may still begin
    assert eng.energy_moments_fetch_blocks()[1].shape == (5, 4, 1, 3)
    eng.close()


def test_plain_and_blocked_entries_refuse_each_other_and_refusals_change_nothing(gpu):
    R, part = 4, (5, 2)
    eng = make(gpu, R * 50, R)
    lib, h = eng._lib, eng._h
    acc, accb = lib.amc_energy_moments_accumulate, lib.amc_energy_moments_accumulate_blocks
    args, values = fetch_sizes()
    fetchb = lib.amc_energy_moments_fetch_blocks
    # a plain accumulator stands: the blocked entry is refused, and leaves it
    eng.sweep(2)
    eng.exchange(1)
    eng.energy_moments_accumulate(*FORM)
    eng.set_blocks(*part)                                  # (leaves a plain accumulator alone)
    plain = eng.energy_moments_fetch()
    assert plain[2] == 1
    assert accb(h, *FORM) == ERR_STATE and b"fetch with reset" in lib.amc_last_error()
    assert fetchb(h, None, None, 0, 0, *args, 0) == ERR_STATE
    after = eng.energy_moments_fetch()
    assert np.array_equal(after[0], plain[0]) and np.array_equal(after[1], plain[1]) and after[2:] == plain[2:]
    eng.energy_moments_fetch(reset=True)
    # a blocked accumulator stands
    eng.energy_moments_accumulate_blocks(*FORM)
    before = eng.energy_moments_fetch_blocks()
    x_before = eng.download_state(want_e=False)[0].copy()
    lo, hi, n, mask, bound = FORM
    assert acc(h, *FORM) == ERR_STATE and b"fetch with reset" in lib.amc_last_error()
    assert accb(h, lo, hi, 199, mask, bound) == ERR_STATE and b"another form" in lib.amc_last_error()
    assert accb(h, 0.25, hi, n, mask, bound) == ERR_STATE and accb(h, lo, 2.75, n, mask, bound) == ERR_STATE
    assert accb(h, lo, hi, n, E.X | E.XX, bound) == ERR_STATE and accb(h, lo, hi, n, mask, 1.75) == ERR_STATE
    B = part[0]
    counts, sums = np.zeros(B * R * 204, dtype=np.uint64), np.zeros(B * R * 3 * 200, dtype=np.int64)
    pc, ps = counts.ctypes.data_as(C.POINTER(C.c_uint64)), sums.ctypes.data_as(C.POINTER(C.c_int64))
    assert fetchb(h, pc, ps, counts.size - 1, sums.size, *args, 1) == ERR_BAD_ARG and b"capacities" in lib.amc_last_error()
    assert fetchb(h, pc, ps, counts.size, sums.size - 1, *args, 1) == ERR_BAD_ARG
    assert fetchb(h, pc, None, counts.size, sums.size, *args, 1) == ERR_BAD_ARG
    assert fetchb(h, None, None, 0, 0, *args, 1) == 0 and values() == (B, R, 200, 3, lo, hi, mask, bound, 0)      # the sizes alone, nothing reset
    assert fetchb(h, pc, ps, counts.size, sums.size, None, *args[1:], 0) == ERR_BAD_ARG
    # amc_set_energy_moments_blocks: a count moved between two blocks (every total of the plain rule still holds), a row one short,
    # another snapshot count, another B, a sum cell beyond what its bin's count can hold, a POS cell above its count or negative
    c0, s0 = before[0], before[1]
    moved = c0.copy()
    cell = int(np.argmax(moved[0, 0, :n]))
    moved[0, 0, cell] -= np.uint64(1)
    moved[1, 0, cell] += np.uint64(1)
    short = c0.copy()
    short[2, 3, int(np.argmax(short[2, 3]))] -= np.uint64(1)
    for bad in (moved, short):
        with pytest.raises(AmcError, match="does not sum"):
            eng.set_energy_moments_blocks(*FORM, bad, s0, 1)
    with pytest.raises(AmcError, match="does not sum"):
        eng.set_energy_moments_blocks(*FORM, c0, s0, 2)
    with pytest.raises(AmcError, match="the partition has 5 blocks"):
        eng.set_energy_moments_blocks(*FORM, c0[:4], s0[:4], 1)
    b = int(np.argmax(c0[3, 2, :n]))
    for col, value in ((0, (int(c0[3, 2, b]) << 32) + 1), (1, -(int(c0[3, 2, b]) << 32) - 1), (2, int(c0[3, 2, b]) + 1), (2, -1)):
        bad = s0.copy()
        bad[3, 2, col, b] = value
        with pytest.raises(AmcError, match="more than"):
            eng.set_energy_moments_blocks(*FORM, c0, bad, 1)
    with pytest.raises(AmcError):
        eng.set_energy_moments_blocks(lo, hi, n, 0, bound, c0, s0, 1)
    after = eng.energy_moments_fetch_blocks()
    assert np.array_equal(after[0], c0) and np.array_equal(after[1], s0) and after[2:] == before[2:]
    assert np.array_equal(eng.download_state(want_e=False)[0].view(np.uint64), x_before.view(np.uint64))
    eng.energy_moments_accumulate_blocks(*FORM)            # ... and the accumulator goes on
    assert eng.energy_moments_fetch_blocks()[2] == 2
    eng.close()


def test_the_word_cap_from_both_sides(gpu):
    """64 blocks of 64 rows: one column takes 64 (n + 4) + 64 n words per set, 64 sets of 510 bins exactly 2^22 words, the cap; one
    bin more is refused, names the constant and leaves nothing behind."""
    R = 64
    assert 64 * (R * (510 + 4) + R * 510) == MAX_WORDS
    eng = make(gpu, R * 64, R, blocks=(64, 1))
    assert eng._lib.amc_energy_moments_accumulate_blocks(eng._h, 0.0, 3.0, 511, E.XX, 2.0) == ERR_BAD_ARG
    assert b"AMC_EMOM_BLK_MAX_WORDS" in eng._lib.amc_last_error()
    assert eng.energy_moments_fetch()[3] == (0.0, 0.0, 0, 0, 0.0)
    form = (0.0, 3.0, 510, E.XX, 2.0)
    eng.energy_moments_accumulate_blocks(*form)
    counts, sums, _, _ = eng.energy_moments_fetch_blocks()
    assert counts.shape == (64, 64, 514) and np.array_equal(counts.sum(axis=2), np.ones((64, 64), dtype=np.uint64))
    same((counts, sums), twin_now(eng, "double_well", form, R, (64, 1)), "at the cap")
    eng.close()


def test_capacity_is_refused_before_a_launch(gpu):
    """The plain rule: a cell holds fewer than 2^31 deposits, (n_snapshots + 1) * n_chains / G < 2^31.  With 4 chains in one group,
    2^29 - 1 snapshots are the most (reached through amc_set_energy_moments_blocks, not by running); the next accumulate is
    AMC_ERR_STATE and changes nothing, one snapshot fewer goes on."""
    eng = make(gpu, 4, blocks=(2, 1))
    lo, hi, n, mask, bound = 0.0, 4.0, 3, ALL, 2.0
    full = 2 ** 29 - 1
    counts = np.zeros((2, 1, n + 4), dtype=np.uint64)
    counts[:, 0, 1] = 2 * full                             # two chains per block
    sums = np.zeros((2, 1, 3, n), dtype=np.int64)
    sums[:, 0, :, 1] = (-(2 * full) << 32, (2 * full) << 32, 2 * full)          # the largest magnitudes the cell's count allows
    with pytest.raises(AmcError, match="2\\^31"):
        eng.set_energy_moments_blocks(lo, hi, n, mask, bound, counts * np.uint64(2), sums, 2 * full)
    with pytest.raises(AmcError, match="no accumulator kept per jackknife block"):
        eng.energy_moments_fetch_blocks()                  # nothing stands after the refusal
    eng.set_energy_moments_blocks(lo, hi, n, mask, bound, counts, sums, full)
    assert eng._lib.amc_energy_moments_accumulate_blocks(eng._h, lo, hi, n, mask, bound) == ERR_STATE and b"2^31" in eng._lib.amc_last_error()
    got = eng.energy_moments_fetch_blocks()
    assert np.array_equal(got[0], counts) and np.array_equal(got[1], sums) and got[2] == full
    merged = eng.energy_moments_fetch()                    # the sums of the two blocks: modulo 2^64, exact
    assert merged[1][0, :, 1].tolist() == [-(4 * full) << 32, (4 * full) << 32, 4 * full] and merged[2] == full
    counts[:, 0, 1] -= np.uint64(2)
    sums[:, 0, :, 1] = 0
    eng.set_energy_moments_blocks(lo, hi, n, mask, bound, counts, sums, full - 1)
    eng.energy_moments_accumulate_blocks(lo, hi, n, mask, bound)
    assert eng.energy_moments_fetch_blocks()[2] == full
    assert eng._lib.amc_energy_moments_accumulate_blocks(eng._h, lo, hi, n, mask, bound) == ERR_STATE
    eng.close()


@pytest.mark.parametrize("again", [(0, 0), (4, 3), (2, 0)], ids=["off", "same", "other"])
def test_set_blocks_folds_to_a_plain_accumulator(gpu, again):
    """In stream order, nothing is lost: the form becomes plain, a plain accumulate continues it, and the result is that of a handle
    that was plain throughout."""
    R, part = 3, (4, 3)
    eng, plain = make(gpu, R * 70, R, blocks=part), make(gpu, R * 70, R)
    for n_sweeps in (2, 1):
        for e in (eng, plain):
            e.sweep(n_sweeps)
        eng.energy_moments_accumulate_blocks(*FORM)
        plain.energy_moments_accumulate(*FORM)
    merged = eng.energy_moments_fetch()
    eng.set_blocks(*again)
    now = eng.energy_moments_fetch()
    assert np.array_equal(now[0], merged[0]) and np.array_equal(now[1], merged[1]) and now[2:] == merged[2:] and now[2] == 2
    with pytest.raises(AmcError, match="no accumulator kept per jackknife block"):
        eng.energy_moments_fetch_blocks()
    if again[0]:
        assert eng._lib.amc_energy_moments_accumulate_blocks(eng._h, *FORM) == ERR_STATE and b"fetch with reset" in eng._lib.amc_last_error()
    for e in (eng, plain):
        e.sweep(2)
        e.energy_moments_accumulate(*FORM)                 # ... and goes on as a plain one
    got, want = eng.energy_moments_fetch(), plain.energy_moments_fetch()
    same(got[:2], want[:2], "folded, then plain")
    assert got[2:] == want[2:] and got[2] == 3
    eng.close()
    plain.close()


def test_set_ladder_clears(gpu):
    eng = make(gpu, 6 * 40, 6, blocks=(2, 3))
    eng.energy_moments_accumulate_blocks(*FORM)
    eng.set_ladder(3)                                      # (turns the partition off too)
    assert eng.energy_moments_fetch()[3] == (0.0, 0.0, 0, 0, 0.0)
    assert eng._lib.amc_energy_moments_accumulate_blocks(eng._h, *FORM) == ERR_STATE and b"no partition" in eng._lib.amc_last_error()
    eng.set_blocks(5, 2)
    form = (0.0, 2.0, 9, E.X | E.POS, 2.0)                 # other groups, another partition, another form
    eng.energy_moments_accumulate_blocks(*form)
    same(eng.energy_moments_fetch_blocks()[:2], twin_now(eng, "double_well", form, 3, (5, 2)), "behind set_ladder")
    eng.close()


def test_respacing(gpu):
    """A respacing that is not taken (no exchange attempt yet: status 2) leaves every block's cells; one that is taken (status 0)
    zeroes them all in stream order and keeps the form."""
    R, part = 4, (4, 3)
    eng = make(gpu, R * 64, R, blocks=part)
    eng.sweep(2)
    eng.energy_moments_accumulate_blocks(*FORM)
    kept = eng.energy_moments_fetch_blocks()
    eng.respace_ladder("acceptance", 1.0, 0.01)
    assert eng.respace_status()[0] == 2
    now = eng.energy_moments_fetch_blocks()
    assert np.array_equal(now[0], kept[0]) and np.array_equal(now[1], kept[1]) and now[2] == 1
    eng.respace_ladder("acceptance", 0.5, 0.01, counts=[100] * (R - 1) + [30, 50, 70])
    eng.sweep(1)
    eng.energy_moments_accumulate_blocks(*FORM)            # queued behind the respacing: the only snapshot left
    assert eng.respace_status()[0] == 0
    got = eng.energy_moments_fetch_blocks()
    assert got[2] == 1 and got[3] == kept[3]
    same(got[:2], twin_now(eng, "double_well", FORM, R, part), "behind a respacing")
    eng.close()


# ---- 6. no disturbance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 4])
def test_a_handle_that_accumulates_and_resets_ends_as_one_that_never_did(gpu, R):
    a, b = make(gpu, 4 * 129, R, blocks=(4, 5)), make(gpu, 4 * 129, R, blocks=(4, 5))
    for _ in range(3):
        for eng in (a, b):
            eng.sweep(3)
            if R:
                eng.exchange(1)
        a.energy_moments_accumulate_blocks(*FORM)
    a.energy_moments_fetch_blocks(reset=True)
    for eng in (a, b):
        eng.sweep(2)
    xa, xb = a.download_state(), b.download_state()
    assert all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(xa, xb))
    assert a.step == b.step and (not R or a.exchange_step == b.exchange_step)
    assert all(np.array_equal(u, v) for u, v in zip(a.counter_totals(), b.counter_totals()))
    a.close()
    b.close()
