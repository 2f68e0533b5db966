"""The host twin of the jackknife blocks (tests/blocks_twin.py) against the big-integer model of the
reproducible sums (tests/xsum_model.py), and the property every caller rests on: the merge over the blocks IS the unpartitioned twin,
word for word.  No GPU, no product code."""
import numpy as np
import pytest

import blocks_twin as K
import bridge_twin as BT
import corr_twin as CT
import oracle_lib as O
import xsum_model as XM

R, L = 3, 211
BETAS = np.array([0.5, 1.0, 2.5])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ensemble():
    rng = np.random.default_rng(11)
    x = rng.normal(size=L * R) * np.tile(1.0 / np.sqrt(2.0 * BETAS), L)
    x[7 * R + 1] = 3.0e5                       # one large summand: the level of its own block's record differs from the others'
    return BT.energies("harmonic", x), np.tile(BETAS, L), x


@pytest.mark.parametrize("n_blocks,chunk,first", [(2, 1, 0), (3, 5, 0), (8, 37, 0), (3, 5, 13), (64, 1, 2 ** 32 - 100), (64, 5, 0)])
def test_bridge_blocks_against_the_model_and_the_unpartitioned_twin(ensemble, n_blocks, chunk, first):
    e, beta, _ = ensemble
    rec = K.bridge_records(e, beta, R, n_blocks, chunk, first=first)
    blk = K.block_of(L, n_blocks, chunk, first)
    assert np.array_equal(K.counts(L, n_blocks, chunk, first), np.bincount(blk, minlength=n_blocks))
    cols = BT.summands(e, beta, R)
    for b in range(n_blocks):
        if not (blk == b).any():
            assert not rec[b].any()                                     # a block without a ladder: all-zero records
            continue
        for r, c in ((0, 0), (1, 1), (0, 2), (2, 3), (1, 4), (1, 5)):
            top, k1, k2, value = XM.sum_r([float(v) for v in cols[c][blk == b, r]])
            kind, lev, flags, m1, m2 = XM.record_ints(rec[b, r, c])
            assert (lev, flags) == (top, 0), (b, r, c)                  # the level is that of the block's own summands
            assert O.xsum_round(rec[b, r, c].reshape(1, -1))[0] == value
    assert np.array_equal(bits(K.merge_blocks(rec)), bits(BT.records(e, beta, R)))


@pytest.mark.parametrize("n_groups", [1, 3])
@pytest.mark.parametrize("n_blocks,chunk,first", [(2, 1, 0), (3, 5, 7), (64, 37, 0)])
def test_corr_blocks_merge_to_the_unpartitioned_twin(ensemble, n_groups, n_blocks, chunk, first):
    _, _, x = ensemble
    rng = np.random.default_rng(3)
    series = [x, x + 0.1 * rng.normal(size=x.size), 0.5 * x + rng.normal(size=x.size)]
    rec = K.corr_records(series, n_groups, n_blocks, chunk, first)
    n_ladders = x.size // n_groups
    present = [b for b in range(n_blocks) if K.counts(n_ladders, n_blocks, chunk, first)[b]]
    assert all(not rec[b].any() for b in range(n_blocks) if b not in present)
    assert np.array_equal(bits(CT.merge([rec[b] for b in present])), bits(CT.records(series, n_groups)))
    blk = K.block_of(n_ladders, n_blocks, chunk, first)
    b = present[-1]
    top, k1, k2, value = XM.sum_r([float(v) for v in (series[0] * series[2]).reshape(-1, n_groups)[blk == b, 0]])
    assert O.xsum_round(rec[b, 2, 0, 2].reshape(1, -1))[0] == value
