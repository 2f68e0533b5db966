"""Jackknife blocks on the device (include/amc.h amc_set_blocks, amc_bridge_fetch_blocks,
amc_corr_fetch_blocks) against their host twin (tests/blocks_twin.py: the partition as a mask over bridge_twin / corr_twin), bit for
bit on all 12 words of every record of every block, and the merge over the blocks against an unpartitioned handle.  Shapes: one
ladder, fewer chunks than blocks (all-zero blocks), chunks that a thread block walks in several trips (C = 37 with R = 64: four
ladders per trip), ladders beyond one grid, R that divides neither 64 nor 256, shards that cut chunks and one beyond 2^32."""
import os

import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd.system import CustomPotential

import blocks_twin as K
import bridge_twin as BT
import corr_twin as CT

pytestmark = pytest.mark.gpu
POOLS = {1: ([0.5], [1.0]), 2: ([0.5, 0.25], [0.625, 0.375])}
LADDER = lambda R: 0.5 * 1.5 ** (np.arange(R) * (8.0 / max(R, 8)))
CUSTOM = "x*x*x*x - 2.0*x*x + 0.25*x"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        at = tuple(int(i) for i in np.argwhere(bits(got) != bits(want))[0][:-1])
        raise AssertionError(f"{what}: records differ, first at {at}: {got[at].tolist()} != {want[at].tolist()}")


def ladder_engine(gpu, R, L, *, potential="harmonic", K_moves=1, dtype="f64", offset=0, n_global=None):
    M = R * L
    ids = np.arange(offset, offset + M, dtype=np.float64)
    x, beta = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids), LADDER(R)[np.arange(offset, offset + M) % R]
    sigma, weight = POOLS[K_moves]
    eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=n_global or offset + M, potential=potential, beta=1.0, sigma=sigma,
                        weight=weight, seed=23, dtype=dtype)
    eng.upload_state(x, beta)
    eng.set_ladder(R)
    return eng, (beta.astype(np.float32).astype(np.float64) if dtype == "f32" else beta)


def chain_engine(gpu, M, *, potential="double_well", dtype="f64", offset=0, n_global=None):
    ids = np.arange(offset, offset + M, dtype=np.float64)
    eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=n_global or offset + M, potential=potential, beta=1.0, sigma=[0.5],
                        weight=[1.0], seed=5, dtype=dtype)
    eng.upload_state(1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids))
    return eng


def bridge_twin_now(eng, beta, R, n_blocks, chunk, columns=BT.ALL, f32=False, first=0):
    return K.bridge_records(eng.download_state()[1], beta, R, n_blocks, chunk, columns, f32, first)


# ---- 1. bridge -------------------------------------------------------------------------------------------------------------------------
BRIDGE = [(2, 1, 2, 1, "harmonic", 1), (3, 37, 3, 5, "double_well", 2), (7, 37, 64, 1, "harmonic", 1), (64, 37, 3, 37, "double_well", 1),
          (64, 37, 64, 5, "harmonic", 2), (2, 30001, 64, 37, "double_well", 1), (3, 37, 2, 37, "harmonic", 1), (7, 211, 3, 5, "double_well", 1)]


@pytest.mark.parametrize("R,L,n_blocks,chunk,potential,K_moves", BRIDGE)
def test_bridge_blocks_match_the_twin_and_merge_to_the_unpartitioned_records(gpu, R, L, n_blocks, chunk, potential, K_moves):
    eng, beta = ladder_engine(gpu, R, L, potential=potential, K_moves=K_moves)
    plain, _ = ladder_engine(gpu, R, L, potential=potential, K_moves=K_moves)
    eng.set_blocks(n_blocks, chunk)
    parts = []
    for i in range(2):                                  # two snapshots with sweeps and exchange steps between them
        for e in (eng, plain):
            e.sweep(2); e.exchange(1 + i); e.sweep(1)
            e.bridge_accumulate()
        parts.append(bridge_twin_now(eng, beta, R, n_blocks, chunk))
    got, n = eng.bridge_fetch_blocks()
    assert n == 2 and got.shape == (n_blocks, R, 6, 12)
    want = np.stack([BT.merge([p[b] for p in parts]) for b in range(n_blocks)])
    same(got, want, f"R={R} L={L} B={n_blocks} C={chunk}")
    empty = K.counts(L, n_blocks, chunk) == 0
    assert not got[empty].any() and (L > chunk * (n_blocks - 1) or empty.any())
    merged, n_m = eng.bridge_fetch()
    ref, n_p = plain.bridge_fetch()
    assert n_m == n_p == 2
    same(merged, ref, "the merge over the blocks against a handle without a partition")
    eng.close(); plain.close()


def test_bridge_default_mask_subset(gpu):
    R, L, n_blocks, chunk = 5, 103, 8, 5
    eng, beta = ladder_engine(gpu, R, L)
    eng.set_blocks(n_blocks, chunk)
    eng.sweep(1)
    eng.bridge_accumulate(BT.ACCEPTANCE_SET)
    got, n = eng.bridge_fetch_blocks(reset=True)
    same(got, bridge_twin_now(eng, beta, R, n_blocks, chunk, BT.ACCEPTANCE_SET), "mask E | EE | MF | MB")
    assert eng.bridge_fetch_blocks()[1] == 0 and not eng.bridge_fetch_blocks()[0].any()
    eng.bridge_accumulate(BT.E)                          # the reset freed the mask
    eng.close()


# ---- 2. time correlation ---------------------------------------------------------------------------------------------------------------
def corr_run(eng, kind, potential, f32=False):
    series = []
    eng.corr_mark(kind)
    series.append(CT.observable(kind, potential, eng.download_state()[0], f32))
    for _ in range(3):
        eng.sweep(2)
        eng.corr_sample()
        series.append(CT.observable(kind, potential, eng.download_state()[0], f32))
    return series


@pytest.mark.parametrize("M,n_blocks,chunk,kind", [(1, 2, 1, "x"), (255, 3, 5, "energy"), (257, 64, 1, "x"), (100003, 32, 0, "energy"),
                                                   (100003, 3, 37, "x")])
def test_corr_blocks_without_a_ladder(gpu, M, n_blocks, chunk, kind):
    eng = chain_engine(gpu, M)
    eng.set_blocks(n_blocks, chunk)
    C = chunk or 256
    series = corr_run(eng, kind, "double_well")
    got, steps, obs = eng.corr_fetch_blocks()
    assert got.shape == (n_blocks, 4, 1, 3, 12) and list(steps) == [0, 2, 4, 6] and obs == CT.OBSERVABLES[kind]
    same(got, K.corr_records(series, 1, n_blocks, C), f"M={M} B={n_blocks} C={C} {kind}")
    same(eng.corr_fetch()[0], CT.records(series, 1), "the merge over the blocks against the unpartitioned twin")
    eng.close()


@pytest.mark.parametrize("R,L,n_blocks,chunk,kind", [(3, 211, 3, 5, "energy"), (64, 37, 2, 37, "x"), (64, 9, 64, 1, "energy")])
def test_corr_blocks_with_a_ladder(gpu, R, L, n_blocks, chunk, kind):
    eng, _ = ladder_engine(gpu, R, L)
    eng.set_blocks(n_blocks, chunk)
    series = corr_run(eng, kind, "harmonic")
    same(eng.corr_fetch_blocks()[0], K.corr_records(series, R, n_blocks, chunk), f"R={R} B={n_blocks} C={chunk} {kind}")
    same(eng.corr_fetch()[0], CT.records(series, R), "merged")
    eng.close()


# ---- 3. grid invariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_cu", ["1", "8"])
def test_grid_invariance(gpu, monkeypatch, per_cu):
    """AMC_BLOCKS_PER_CU = 1 and 8 (the knob is read at amc_create): the same bits, and 37 ladders of 3 rungs ask for ONE block before
    the grid is rounded up to B = 64."""
    monkeypatch.setenv("AMC_BLOCKS_PER_CU", per_cu)
    for R, L, n_blocks, chunk in ((3, 37, 64, 1), (2, 30001, 3, 5)):
        eng, beta = ladder_engine(gpu, R, L)
        eng.set_blocks(n_blocks, chunk)
        eng.sweep(1)
        eng.bridge_accumulate()
        same(eng.bridge_fetch_blocks()[0], bridge_twin_now(eng, beta, R, n_blocks, chunk), f"AMC_BLOCKS_PER_CU={per_cu} L={L}")
        eng.close()


# ---- 4. shards -------------------------------------------------------------------------------------------------------------------------
def test_shards_that_cut_chunks_merge_to_one_handle(gpu):
    R, L, n_blocks, chunk = 3, 211, 8, 5
    cuts = [0, 52, 134, L]                               # ladder boundaries inside chunks (52 = 10 * 5 + 2, 134 = 26 * 5 + 4; even chain offsets)
    whole, beta = ladder_engine(gpu, R, L)
    whole.set_blocks(n_blocks, chunk)
    whole.bridge_accumulate()
    want = whole.bridge_fetch_blocks()[0]
    parts = []
    for a, z in zip(cuts[:-1], cuts[1:]):
        eng, _ = ladder_engine(gpu, R, z - a, offset=a * R, n_global=L * R)
        eng.set_blocks(n_blocks, chunk)
        eng.bridge_accumulate()
        parts.append(eng.bridge_fetch_blocks()[0])
        same(parts[-1], K.bridge_records(eng.download_state()[1], beta[a * R:z * R], R, n_blocks, chunk, first=a), f"shard [{a}, {z})")
        eng.close()
    same(np.stack([BT.merge([p[b] for p in parts]) for b in range(n_blocks)]), want, "three shards merged block by block")
    whole.close()


def test_a_shard_beyond_two_to_the_32(gpu):
    M, n_blocks, chunk = 1000, 3, 37
    first = 2 ** 32 - 500                                # l_global crosses 2^32 inside the shard (G = 1: a ladder is a chain)
    eng = chain_engine(gpu, M, offset=first, n_global=2 ** 33)
    eng.set_blocks(n_blocks, chunk)
    eng.corr_mark("x")
    x = eng.download_state()[0]
    same(eng.corr_fetch_blocks()[0], K.corr_records([x], 1, n_blocks, chunk, first), "offset beyond 2^32")
    eng.close()


# ---- 5. flags --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_planted_value_flags_its_own_block_alone(gpu, bad):
    M, n_blocks, chunk = 600, 8, 5
    eng = chain_engine(gpu, M, potential="harmonic")
    x = eng.download_state()[0]
    x[233] = bad                                         # chain 233: chunk 46, block 46 mod 8 = 6
    eng.upload_state(x)
    eng.set_blocks(n_blocks, chunk)
    eng.corr_mark("x")
    got = eng.corr_fetch_blocks()[0]
    same(got, K.corr_records([x], 1, n_blocks, chunk), f"planted {bad}")
    flagged = [b for b in range(n_blocks) if got[b, 0, 0, 0, 2] != 0.0]
    assert flagged == [6]
    eng.close()


# ---- 6. Float32 state and a custom potential --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,potential", [("f32", "double_well"), ("f64", "custom")])
def test_run_time_compiled_handles_take_the_same_route(gpu, dtype, potential):
    R, L, n_blocks, chunk = 5, 103, 3, 5
    pot = CustomPotential(CUSTOM) if potential == "custom" else potential
    eng, beta = ladder_engine(gpu, R, L, potential=pot, dtype=dtype)
    eng.set_blocks(n_blocks, chunk)
    eng.sweep(2); eng.exchange(1)
    eng.bridge_accumulate()
    same(eng.bridge_fetch_blocks()[0], bridge_twin_now(eng, beta, R, n_blocks, chunk, f32=dtype == "f32"), f"{dtype} {potential}")
    eng.corr_mark("x")
    x = eng.download_state()[0]
    same(eng.corr_fetch_blocks()[0], K.corr_records([x], R, n_blocks, chunk), f"{dtype} {potential} corr")
    eng.close()


# ---- 7. lifetime -----------------------------------------------------------------------------------------------------------------------
def test_lifetime(gpu):
    R, L = 4, 64
    eng, beta = ladder_engine(gpu, R, L)
    with pytest.raises(ma.AmcError):
        eng.bridge_fetch_blocks()                        # no partition
    eng.bridge_accumulate()
    before = eng.bridge_fetch()[0]                       # a handle that never set a partition: the records it always returned
    same(before, BT.records(eng.download_state()[1], beta, R), "no partition")
    eng.corr_mark("x")
    eng.set_blocks(4, 3)                                 # clears the accumulator and the mark
    assert eng.bridge_fetch()[1] == 0 and eng.corr_fetch()[2] == 0
    for bad in ((1, 1), (65, 1), (4, -1), (4, 2 ** 40 + 1)):
        with pytest.raises(ma.AmcError):
            eng.set_blocks(*bad)
    eng.bridge_accumulate()
    eng.corr_mark("x")
    with pytest.raises(ma.AmcError):
        eng.set_bridge(before, 1)                        # merged records cannot be split into blocks
    eng.set_blocks(4, 3)
    assert eng.bridge_fetch_blocks()[1] == 0 and eng.corr_fetch_blocks()[2] == 0
    eng.bridge_accumulate()
    eng.set_ladder(R)                                    # turns the partition off
    with pytest.raises(ma.AmcError):
        eng.bridge_fetch_blocks()
    eng.bridge_accumulate()
    same(eng.bridge_fetch()[0], BT.records(eng.download_state()[1], beta, R), "after set_ladder: unpartitioned again")
    eng.close()


def test_a_respacing_that_is_taken_zeroes_every_block(gpu):
    R, L = 4, 129
    eng, _ = ladder_engine(gpu, R, L, potential="double_well")
    eng.set_blocks(4, 8)
    eng.sweep(2)
    eng.bridge_accumulate()
    eng.respace_ladder("acceptance", 1.0, 0.01)                # refused on the device (no gap was attempted yet): the blocks stay
    assert eng.respace_status()[0] == 2 and eng.bridge_fetch_blocks()[1] == 1
    eng.sweep_exchange(8, 1)
    eng.respace_ladder("acceptance", 1.0, 0.01)                # taken
    assert eng.respace_status()[0] == 0
    rec, n = eng.bridge_fetch_blocks()
    assert n == 0 and not rec.any()
    eng.bridge_accumulate()                                    # ... and the blocks go on at the new ladder
    same(eng.bridge_fetch_blocks()[0], bridge_twin_now(eng, np.tile(eng.ladder(), L), R, 4, 8), "after the respacing")
    eng.close()


def test_anneal_is_refused_while_a_partition_is_set(gpu):
    eng = gpu.HipEngine(n_chains=512, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=5)
    eng.init_uniform(-1.0, 1.0)
    eng.set_blocks(4, 16)
    with pytest.raises(ma.AmcError, match="partition"):
        eng.anneal(1.5)
    eng.set_blocks(0)
    eng.anneal(1.5)
    eng.close()


# ---- 5b. flags on a ladder handle: the bridge columns ------------------------------------------------------------------------------------
def test_a_planted_value_flags_its_own_block_rung_and_columns_on_a_ladder(gpu):
    """x = NaN at one chain of a ladder handle: the records that read its energy -- its own rung's columns, and the neighbours' W and M
    columns that reweight with it -- are flagged in ITS block alone; every word against the twin."""
    R, L, n_blocks, chunk = 3, 40, 4, 5
    eng, beta = ladder_engine(gpu, R, L)
    x = eng.download_state()[0]
    x[17 * R + 1] = np.nan                               # ladder 17 (chunk 3, block 3), rung 1
    eng.upload_state(x, beta)
    eng.set_ladder(R)
    eng.set_blocks(n_blocks, chunk)
    eng.bridge_accumulate()
    got = eng.bridge_fetch_blocks()[0]
    same(got, bridge_twin_now(eng, beta, R, n_blocks, chunk), "planted NaN on a ladder")
    assert not got[:3, :, :, 2].any() and got[3, 1, :, 2].all()


# ---- 5c. levels: every branch of the block end in one slot of one HIP block ----------------------------------------------------------------
@pytest.mark.parametrize("sums", ["bridge", "corr"])
def test_levels_differ_among_the_lanes_of_one_slot_of_one_block(gpu, sums):
    """R = 3, L = 64, B = 2, C = 32: two HIP blocks, each with the one chunk of its jackknife block, a chain per lane.  The ladders of
    rung 1 hold |x| near 1, 2^-20, 2^-40, 2^-90 in turn, so every chunk holds all four and neighbouring lanes of that rung sit 0, 1
    and >= 2 levels of 50 bits below the slot's top: O = x at the levels 0, -1, -1, -2; the harmonic e = x^2 at 0, -1, -2, -4."""
    R, L, n_blocks, chunk = 3, 64, 2, 32
    eng, beta = ladder_engine(gpu, R, L)
    l = np.arange(L)
    x = eng.download_state()[0].reshape(L, R)
    x[:, 1] = np.where(l % 3 == 0, -1.0, 1.0) * (1.0 + 0.37 * np.sin(l)) * np.array([1.0, 2.0 ** -20, 2.0 ** -40, 2.0 ** -90])[l % 4]
    eng.upload_state(x.reshape(-1), beta)
    eng.set_ladder(R)
    eng.set_blocks(n_blocks, chunk)
    if sums == "bridge":
        eng.bridge_accumulate()
        same(eng.bridge_fetch_blocks()[0], bridge_twin_now(eng, beta, R, n_blocks, chunk), "levels in one slot of one block, bridge")
    else:
        eng.corr_mark("x")
        series = [eng.download_state()[0]]
        same(eng.corr_fetch_blocks()[0], K.corr_records(series, R, n_blocks, chunk), "levels in one slot of one block, corr")
    eng.close()


# ---- 8. the setters and a resume -----------------------------------------------------------------------------------------------------------
def test_setters_refuse_what_their_twins_refuse_and_a_resumed_handle_ends_on_the_same_bits(gpu):
    R, L, n_blocks, chunk = 3, 211, 8, 5
    whole, beta = ladder_engine(gpu, R, L)
    part, _ = ladder_engine(gpu, R, L)

    def stretch(e):
        e.sweep(2); e.exchange(1); e.bridge_accumulate(); e.sweep(1); e.corr_sample()

    with pytest.raises(ma.AmcError, match="no partition"):
        part.set_bridge_blocks(np.zeros((n_blocks, R, 6, 12)), 1)
    for e in (whole, part):
        e.set_blocks(n_blocks, chunk)
        e.corr_mark("x")
        stretch(e)
    rec, n = part.bridge_fetch_blocks()
    crec, steps, obs = part.corr_fetch_blocks()
    origin = part.corr_origin()

    def refused(call, *args):
        with pytest.raises(ma.AmcError):
            call(*args)
        same(part.bridge_fetch_blocks()[0], rec, "a refused call leaves the handle as it was")
        same(part.corr_fetch_blocks()[0], crec, "a refused call leaves the handle as it was")

    def changed(a, at, value):
        out = a.copy()
        out[at] = value
        return out

    refused(part.set_bridge_blocks, rec[:4], n)                                      # another number of blocks
    refused(part.set_bridge_blocks, changed(rec, (2, 1, 0, 0), 5.0), n)              # no kind-R record
    refused(part.set_bridge_blocks, changed(rec, (2, 1, 0, 1), 1e9), n)              # a level outside the range
    refused(part.set_bridge_blocks, changed(rec, (2, 1, 0, 1), 0.5), n)              # a level that is no integer
    refused(part.set_bridge_blocks, changed(rec, (2, 1, 0, 2), 0.5), n)              # flags that are no integer
    refused(part.set_bridge_blocks, changed(rec, (2, 1, 0, 5), 0.5), n)              # a word that is no integer
    refused(part.set_bridge_blocks, changed(rec, (2, 1, 0, 5), 2.0 ** 53), n)        # ... not below 2^53
    refused(part.set_bridge_blocks, changed(rec, (2, R - 1, 2), rec[2, 0, 2]), n)    # WF at the last rung has no summand
    refused(part.set_bridge_blocks, changed(rec, (2, 1, 0), 0.0), n)                 # a column with records at some rungs only
    refused(part.set_bridge_blocks, changed(rec, (2, slice(None), 0), 0.0), n)       # a mask that differs between blocks
    refused(part.set_bridge_blocks, changed(rec, (2,), 0.0), n)                      # an all-zero block that has ladders
    refused(part.set_bridge, part.bridge_fetch()[0], n)                              # merged records under a partition
    refused(part.set_corr_blocks, "x", origin, crec[:4], steps)
    refused(part.set_corr_blocks, 7, origin, crec, steps)
    refused(part.set_corr_blocks, "x", origin, crec, steps[::-1].copy())
    refused(part.set_corr_blocks, "x", origin, changed(crec, (1, 0, 0, 0, 0), 5.0), steps)
    refused(part.set_corr_blocks, "x", origin, changed(crec, (1, 0, 0, 0, 7), 0.25), steps)
    refused(part.set_corr_blocks, "x", origin, changed(crec, (1, 1, 0, 0), 0.0), steps)          # every sample had a summand
    refused(part.set_corr, "x", origin, part.corr_fetch()[0], steps)
    with pytest.raises(ma.AmcError):
        part.set_corr_blocks("x", origin, crec[:, :0], steps[:0])                    # no sample

    part.set_blocks(n_blocks, chunk)                                                  # forgets everything, as a fresh handle
    assert part.bridge_fetch_blocks()[1] == 0 and part.corr_fetch_blocks()[2] == 0
    part.set_bridge_blocks(rec, n)
    part.set_corr_blocks("x", origin, crec, steps)
    same(part.bridge_fetch_blocks()[0], rec, "what was set comes back")
    same(part.corr_fetch_blocks()[0], crec, "what was set comes back")
    for e in (whole, part):
        stretch(e)
    want, n_w = whole.bridge_fetch_blocks()
    got, n_g = part.bridge_fetch_blocks()
    assert n_w == n_g == 2
    same(got, want, "the resumed bridge sums")
    same(part.corr_fetch_blocks()[0], whole.corr_fetch_blocks()[0], "the resumed time correlation")
    assert list(part.corr_fetch_blocks()[1]) == list(whole.corr_fetch_blocks()[1])
    part.set_bridge_blocks(None)
    assert part.bridge_fetch_blocks()[1] == 0
    whole.close(); part.close()
