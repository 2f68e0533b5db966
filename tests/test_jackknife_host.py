"""montecarlo_amd.jackknife on the host: the estimator's identities on synthetic records.  No GPU: records
are made by the oracle's xsum_r, merged by the product's xsum_merge (record arithmetic of libamc.so, which needs no device)."""
import numpy as np
import pytest
from scipy import stats

import oracle_lib as O
from montecarlo_amd.jackknife import block_counts, default_chunk, jackknife, leave_one_out


def records(values_by_block):
    """records[B][columns][12] of values_by_block[b][column] = the summands."""
    return np.stack([np.stack([O.xsum_r(np.ascontiguousarray(col, dtype=np.float64)) for col in blk]) for blk in values_by_block])


def test_plain_mean_with_equal_blocks_is_the_textbook_standard_error():
    rng = np.random.default_rng(5)
    B, n = 16, 40
    data = 0.3 + rng.normal(size=(B, n))
    theta, se = jackknife(records([[d] for d in data]), np.full(B, n), lambda v, m: v[0] / m)
    means = data.mean(axis=1)
    assert theta == pytest.approx(data.mean(), rel=1e-14)
    assert se == pytest.approx(np.sqrt(((means - means.mean()) ** 2).sum() / (B * (B - 1))), rel=1e-12)


def test_leave_one_out_totals_are_exact_merges():
    rng = np.random.default_rng(6)
    data = rng.normal(size=(5, 2, 9)) * 10.0 ** rng.integers(-3, 4, size=(5, 2, 1))
    rec = records(data)
    total, loo = leave_one_out(rec)
    assert np.array_equal(total, records([[data[:, c].reshape(-1) for c in range(2)]])[0])
    for b in range(5):
        rest = np.delete(data, b, axis=0)
        assert np.array_equal(loo[b], records([[rest[:, c].reshape(-1) for c in range(2)]])[0]), b


def test_coverage_of_a_ratio_of_means():
    """200 replicas of theta = mean(y) / mean(x) over B = 16 blocks: the fraction with |theta - exact| <= 2 se lies within four binomial
    standard deviations of the Student-t value at B - 1 degrees of freedom."""
    rng = np.random.default_rng(20261020)
    B, n, reps = 16, 64, 200
    hits = 0
    for _ in range(reps):
        x = 2.0 + 0.5 * rng.normal(size=(B, n))
        y = 3.0 + 0.25 * (x - 2.0) + 0.7 * rng.normal(size=(B, n))
        theta, se = jackknife(records([[x[b], y[b]] for b in range(B)]), np.full(B, n), lambda v, m: v[1] / v[0])
        hits += abs(theta - 1.5) <= 2.0 * se
    p = 2.0 * stats.t.cdf(2.0, B - 1) - 1.0
    print(f"coverage {hits / reps:.4f}, Student-t {p:.4f}, four sd {4.0 * np.sqrt(p * (1.0 - p) / reps):.4f}")
    assert abs(hits / reps - p) <= 4.0 * np.sqrt(p * (1.0 - p) / reps)


def test_unequal_blocks_and_an_empty_block():
    rng = np.random.default_rng(8)
    sizes = [3, 40, 17, 1]
    data = [rng.normal(size=s) + 1.0 for s in sizes]
    theta, se = jackknife(records([[d] for d in data]), sizes, lambda v, m: v[0] / m)
    flat = np.concatenate(data)
    loo = np.array([np.delete(flat, np.arange(sum(sizes[:b]), sum(sizes[:b + 1]))).mean() for b in range(4)])
    assert theta == pytest.approx(flat.mean(), rel=1e-14)
    assert se == pytest.approx(np.sqrt(3.0 / 4.0 * ((loo - loo.mean()) ** 2).sum()), rel=1e-11)
    rec = records([[d] for d in data])
    rec[2] = 0.0
    with pytest.raises(ValueError, match="block 2 is empty"):
        jackknife(rec, [3, 40, 0, 1], lambda v, m: v[0] / m)
    with pytest.raises(ValueError, match="at least 2"):
        jackknife(rec[:1], [3], lambda v, m: v[0] / m)
    with pytest.raises(ValueError, match="shape"):
        jackknife(rec, [3, 40, 17], lambda v, m: v[0] / m)


@pytest.mark.parametrize("n,B,C,first", [(1, 2, 1, 0), (36, 3, 37, 0), (2369, 64, 37, 5), (30001, 8, 5, 2 ** 32 - 7), (100, 64, 5, 0)])
def test_block_counts_closed_form(n, B, C, first):
    want = np.bincount([((first + l) // C) % B for l in range(n)], minlength=B)
    assert np.array_equal(block_counts(n, B, C, first), want)
    assert default_chunk(1) == 256 and default_chunk(8) == 32 and default_chunk(64) == 4 and default_chunk(7) == 36


# ---- blocks= on the algorithms, over the engine double of the host tests ------------------------------------------------------------------
import montecarlo_amd as ma

import blocks_twin as KB
import corr_twin as CTW


class BlocksTwinEngine(CTW.CorrTwinEngine):
    """corr_twin.CorrTwinEngine plus the partition: set_blocks, corr_fetch_blocks and set_corr_blocks computed by blocks_twin (G = 1)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.part, self._series, self._kind, self._blk = None, None, None, None

    def set_blocks(self, n_blocks, chunk=0):
        self.calls.append(("blocks", int(n_blocks), int(chunk)))
        self.part, self._corr, self._series, self._blk = ((int(n_blocks), int(chunk)) if n_blocks else None), None, None, None

    def corr_mark(self, kind="energy"):
        super().corr_mark(kind)
        self._kind, self._series = kind, [self._observe(kind)]
        self._blk = [KB.corr_records(self._series, 1, *self.part)[:, 0]] if self.part else None

    def corr_sample(self):
        super().corr_sample()
        self._series.append(self._observe(self._kind))
        if self.part:
            self._blk.append(KB.corr_records([self._corr["origin"], self._series[-1]], 1, *self.part)[:, 1])

    def corr_fetch_blocks(self):
        assert self.part is not None
        self.calls.append(("fetch_blocks", self.step))
        return np.stack(self._blk, axis=1), np.array(self._corr["steps"], dtype=np.uint64), self._corr["observable"]

    def set_corr_blocks(self, kind, origin, records, steps):
        assert self.part is not None and np.shape(records)[0] == self.part[0]
        rec = np.asarray(records, dtype=np.float64)
        self.set_corr(kind, origin, KB.merge_blocks(rec), steps)
        self._kind, self._series, self._blk = kind, [np.array(origin, dtype=np.float64)], [rec[:, s] for s in range(rec.shape[1])]


def build_blocks(path, steps, scheduler, n_lags, anneal_at=None, M=64, **kw):
    chains = ma.ParticleChains.uniform(M, 1.0, potential="harmonic")
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.4], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=3, engine_factory=BlocksTwinEngine),
          dict(algorithm=ma.Autocorrelation, dependencies=(ma.Metropolis,), scheduler=scheduler, observable="x", n_lags=n_lags, **kw)]
    if anneal_at is not None:
        al.append(dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=anneal_at, betas=[1.5]))
    return ma.Simulation(chains, al, steps, path=str(path))


def test_blocks_are_set_once_in_front_of_the_first_mark_and_the_errors_are_the_jackknife_of_the_block_records(oracle, amc, tmp_path):
    sim = build_blocks(tmp_path, 10, [2, 4, 6, 8], n_lags=3, blocks=4, block_chunk=3)
    ma.run(sim)
    eng = sim.algorithms[0].engine
    ac = next(a for a in sim.algorithms if isinstance(a, ma.Autocorrelation))
    assert eng.calls[:5] == [("blocks", 4, 3), ("mark", 2), ("sample", 4), ("sample", 6), ("sample", 8)]
    assert [c for c in eng.calls if c[0] == "blocks"] == [("blocks", 4, 3)]
    rho, se = ac.rho(error=True)
    assert np.array_equal(rho, ac.rho()) and se.shape == rho.shape == (1, 4) and np.all(se[:, 1:] > 0)
    rec = KB.corr_records(eng._series, 1, 4, 3)
    want = jackknife(rec, KB.counts(64, 4, 3), lambda v, n: ma.correlation.rho_from_means(v / n))
    assert np.array_equal(want[0], rho) and np.array_equal(want[1], se)
    tau, tau_se, window, converged = ac.tau_int(error=True)
    assert np.array_equal(tau, ac.tau_int()[0]) and tau_se.shape == (1,) and np.isfinite(tau_se[0]) and tau_se[0] > 0
    assert np.array_equal(ma.callback_tau_int_error(sim), tau_se)


def test_refusals_of_blocks(oracle, amc, tmp_path):
    for kw, match in ((dict(blocks=1), "blocks"), (dict(blocks=65), "blocks"), (dict(blocks=2.5), "blocks"), (dict(blocks=4, block_chunk=0), "block_chunk"),
                      (dict(block_chunk=3), "without blocks"), (dict(blocks=4, block_chunk=32), "larger than the 2 chunks")):
        with pytest.raises(ValueError, match=match):
            build_blocks(tmp_path, 4, [1, 2], n_lags=1, **kw)
    with pytest.raises(ValueError, match="larger than the 1 chunks"):      # the default chunk without a ladder: 256 chains
        build_blocks(tmp_path, 4, [1, 2], n_lags=1, blocks=2)
    sim = build_blocks(tmp_path / "pa", 8, [1, 2], n_lags=1, anneal_at=[5], blocks=4, block_chunk=3)
    with pytest.raises(ValueError, match="PopulationAnnealing"):
        ma.run(sim)
    assert sim.algorithms[0].engine.calls == []
    sim = build_blocks(tmp_path / "no", 4, [1, 2], n_lags=1)
    ma.run(sim)
    with pytest.raises(ValueError, match="blocks=B"):
        next(a for a in sim.algorithms if isinstance(a, ma.Autocorrelation)).rho(error=True)
    assert all(c[0] != "blocks" for c in sim.algorithms[0].engine.calls)


@pytest.mark.parametrize("cut", [3, 5, 8])
def test_the_blocked_checkpoint_section_round_trip(oracle, amc, tmp_path, cut):
    """Stopped inside the first origin, between the origins and inside the second: the resumed run ends on the block records, and so
    on the error bars, of the whole one; a run that asks for another partition refuses the checkpoint."""
    sched, kw = [1, 2, 3, 4, 6, 7, 8, 9], dict(n_lags=3, origins=2, blocks=4, block_chunk=3)
    whole = build_blocks(tmp_path / "w", 10, sched, **kw)
    ma.run(whole)
    first = build_blocks(tmp_path / "a", cut, [t for t in sched if t <= cut], **kw)
    ma.run(first)
    d = np.load(ma.checkpoint(first.algorithms[0], str(tmp_path / "ck")))
    assert "corr_blocks" in d.files and ("corr_block_records" in d.files) == (int(d["corr_phase"]) >= 0)
    assert ("corr_acc_blocks" in d.files) == (int(d["corr_origins_done"]) > 0)
    second = build_blocks(tmp_path / "b", 10 - cut, [t - cut for t in sched if t > cut], **kw)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = (next(x for x in sim.algorithms if isinstance(x, ma.Autocorrelation)) for sim in (second, whole))
    assert np.array_equal(a.block_records()[0].view(np.uint64), b.block_records()[0].view(np.uint64))
    assert np.array_equal(a.records().view(np.uint64), b.records().view(np.uint64))
    for x, y in zip(a.rho(error=True) + a.tau_int(error=True), b.rho(error=True) + b.tau_int(error=True)):
        assert np.array_equal(x, y)
    other = build_blocks(tmp_path / "c", 10 - cut, [t - cut for t in sched if t > cut], n_lags=3, origins=2, blocks=5, block_chunk=3)
    with pytest.raises(ValueError, match="partition"):
        ma.restore(other.algorithms[0], str(tmp_path / "ck"))
