"""The passes over the energy bins against EACH OTHER on the same positions (section 3.14 "Error bars"): the
histogram per group, per jackknife block and per block of families, and the moments per group and per jackknife block are two deposit
rules on three traversals of the chains, so a slip in one traversal shows against the others and not only against its own twin.
Everything is integers: no tolerance anywhere.

Shapes: 3 rungs x 257 ladders (257 = 4 x 64 + 1 is no multiple of 4 or of B x chunk = 12: the tail of the traversal by group runs,
and the walk over the blocks ends with one to three ladders left over), once as a shard that begins at ladder 10, inside a chunk (a shard begins at an even chain); 7 bins (the cells of
a HIP block in LDS) and 4100 bins (3 x 4103 = 12 309 cells, just over the 12 288 of the LDS path: a global atomic per deposit; the
moments' threshold is lower, so they take both paths too); chains below lo, at or above hi, and one NaN."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
R, L, B, CHUNK = 3, 257, 4, 3
M = R * L
LO, HI = 0.125, 2.5
MASK, X_BOUND = 7, 4.0                  # every column; |x| < 2 everywhere, so no chain lands in the fourth tail cell
N_BINS = (7, 4100)
NAN_AT = 100


def start_x(offset=0, nan=True):
    ids = np.arange(offset, offset + M)
    x = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)
    if nan:
        x[NAN_AT] = np.nan
    return x


def ladder_engine(gpu, offset=0):
    eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=offset + M, potential="double_well", beta=1.0, sigma=[0.5],
                        weight=[1.0], seed=23)
    eng.upload_state(start_x(offset), (0.5 * 1.5 ** np.arange(R))[np.arange(offset, offset + M) % R])
    eng.set_ladder(R)
    eng.set_blocks(B, CHUNK)
    return eng


def plain_histogram(eng, n):
    eng.energy_histogram_accumulate(LO, HI, n)
    counts, snaps, _ = eng.energy_histogram_fetch(reset=True)
    assert snaps == 1
    return counts


def plain_moments(eng, n):
    eng.energy_moments_accumulate(LO, HI, n, MASK, X_BOUND)
    counts, sums, snaps, _ = eng.energy_moments_fetch(reset=True)
    assert snaps == 1
    return counts, sums


@pytest.mark.parametrize("offset", [0, R * 10], ids=["whole", "l_first=10"])
@pytest.mark.parametrize("n", N_BINS)
def test_blocked_passes_sum_to_the_plain_ones_and_moments_count_as_the_histogram(gpu, n, offset):
    eng = ladder_engine(gpu, offset)
    hist = plain_histogram(eng, n)
    assert hist.shape == (R, n + 3) and np.array_equal(hist.sum(axis=1), np.full(R, L, dtype=np.uint64))
    assert hist[:, n].sum() > 0 and hist[:, n + 1].sum() > 0 and hist[:, n + 2].sum() == 1 and hist[:, :n].sum() > 0      # below, above, the NaN, inside

    eng.energy_histogram_accumulate_blocks(LO, HI, n)
    hist_b, snaps, _ = eng.energy_histogram_fetch_blocks(reset=True)
    assert hist_b.shape == (B, R, n + 3) and snaps == 1
    assert np.array_equal(hist_b.sum(axis=0, dtype=np.uint64), hist), "the histogram per block, summed over the blocks, is not the plain one"
    assert (hist_b.sum(axis=(1, 2)) > 0).all()                 # every block has ladders here

    counts, sums = plain_moments(eng, n)
    eng.energy_moments_accumulate_blocks(LO, HI, n, MASK, X_BOUND)
    counts_b, sums_b, snaps, _ = eng.energy_moments_fetch_blocks(reset=True)
    assert counts_b.shape == (B, R, n + 4) and sums_b.shape == (B, R, 3, n) and snaps == 1
    assert np.array_equal(counts_b.sum(axis=0, dtype=np.uint64), counts), "the moments' counts per block do not sum to the plain ones"
    assert np.array_equal(sums_b.sum(axis=0, dtype=np.int64), sums), "the moments' sums per block do not sum to the plain ones"
    assert sums.any()

    assert not counts[:, n + 3].any()
    assert np.array_equal(counts[:, :n + 3], hist), "the moments' count cells are not the histogram's"
    assert np.array_equal(counts_b[:, :, :n + 3], hist_b), "the moments' count cells per block are not the histogram's per block"
    eng.close()


def test_histogram_per_block_of_families_sums_to_the_plain_one(gpu):
    eng = gpu.HipEngine(n_chains=M, potential="double_well", beta=0.5, sigma=[0.5], weight=[1.0], seed=23)
    eng.upload_state(start_x(nan=False))
    eng.set_anneal_families(True)
    eng.set_anneal_blocks(B)
    eng.sweep(2)
    eng.anneal(2.0)                                             # one resampling: the blocks' families are uneven from here on
    x = eng.download_state(want_e=False)[0]
    x[NAN_AT] = np.nan                                          # (behind the resampling: its weights want finite energies)
    eng.upload_state(x)
    for n in N_BINS:                                            # 4 x 10 cells in LDS, 4 x 4103 beyond
        eng.energy_histogram_accumulate_blocks(LO, HI, n)
        by_block, snaps, _ = eng.energy_histogram_fetch_blocks(reset=True)
        assert by_block.shape == (B, 1, n + 3) and snaps == 1 and by_block.sum() == M
        assert not np.array_equal(by_block.sum(axis=(1, 2)), [193, 193, 193, 192])      # (the blocks' sizes before the resampling)
        hist = plain_histogram(eng, n)
        assert np.array_equal(by_block.sum(axis=0, dtype=np.uint64), hist), ("the histogram per block of families does not sum to the plain one", n)
    eng.close()


@pytest.mark.parametrize("n", N_BINS)
def test_another_partition_folds_the_blocked_accumulators_into_the_plain_result(gpu, n):
    eng = ladder_engine(gpu)
    hist = plain_histogram(eng, n)
    counts, sums = plain_moments(eng, n)
    eng.energy_histogram_accumulate_blocks(LO, HI, n)
    eng.energy_moments_accumulate_blocks(LO, HI, n, MASK, X_BOUND)
    eng.set_blocks(5, 2)                                        # both are folded on the stream
    for fetch_blocks in (eng.energy_histogram_fetch_blocks, eng.energy_moments_fetch_blocks):
        with pytest.raises(gpu.AmcError, match="no accumulator kept per jackknife block"):
            fetch_blocks()
    folded, snaps, _ = eng.energy_histogram_fetch()
    assert snaps == 1 and np.array_equal(folded, hist), "the folded histogram is not the plain one"
    folded_counts, folded_sums, snaps, _ = eng.energy_moments_fetch()
    assert snaps == 1 and np.array_equal(folded_counts, counts) and np.array_equal(folded_sums, sums), "the folded moments are not the plain ones"
    eng.close()
