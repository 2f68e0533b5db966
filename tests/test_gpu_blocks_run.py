"""``run(...)`` with ``ReplicaExchange(bridge=..., blocks=B)`` on the device, end to end: ``error=True`` returns
the values the estimators always returned, bit for bit, and the standard errors of a jackknife restated here over the twin's
estimators (bridge_twin.log_z_* on leave-one-out merges of the device's block records); the refusals; and a run checkpointed inside
an origin of an ``Autocorrelation`` WITHOUT blocks of its own -- which keeps its sums under the exchange's partition -- resumes and
ends on the same bits."""
import numpy as np
import pytest

import montecarlo_amd as ma

import blocks_twin as K
import bridge_twin as BT

pytestmark = pytest.mark.gpu
R, L, B, C = 4, 500, 8, 16                       # 32 chunks, the last one cut: blocks of 64 and 52 ladders
BETAS = tuple(1.1 ** np.arange(R))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def build(path, steps, corr=None, exchange=None, corr_kw=None):
    x0 = np.random.default_rng(5).standard_normal(R * L) / np.sqrt(2.0 * np.tile(BETAS, L))
    chains = ma.ParticleChains.ladder(L, BETAS, potential="harmonic", x=x0)
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.8], 1.0),)
    kw = dict(bridge=BT.ALL, blocks=B, block_chunk=C) if exchange is None else exchange
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=9), dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), **kw)]
    if corr is not None:
        al.append(dict(algorithm=ma.Autocorrelation, dependencies=(ma.Metropolis,), scheduler=corr, observable="energy", n_lags=3, **(corr_kw or {})))
    return ma.Simulation(chains, al, steps, path=str(path))


def restated(rec, counts, fn):
    """(theta of the full merge, se) of fn(records[R][6][12], ladders): the jackknife written out over bridge_twin.merge."""
    n_blocks = rec.shape[0]
    reps = np.stack([fn(BT.merge([rec[j] for j in range(n_blocks) if j != b]), int(counts.sum() - counts[b])) for b in range(n_blocks)])
    dev = reps - reps.mean(axis=0)
    return fn(BT.merge(list(rec)), int(counts.sum())), np.sqrt((n_blocks - 1) / n_blocks * (dev * dev).sum(axis=0))


def test_error_true_returns_the_values_of_always_and_the_jackknife_of_the_block_records(gpu, tmp_path):
    sim = build(tmp_path, 24)
    ma.run(sim)
    rx, eng = sim.algorithms[1], sim.algorithms[0].engine
    rec, n = eng.bridge_fetch_blocks()
    counts = K.counts(L, B, C)
    assert n == 24 and rec.shape == (B, R, 6, 12) and sorted(set(counts)) == [52, 64]
    got, n_b, ladders = rx.bridge_blocks()
    assert n_b == n and np.array_equal(ladders, counts) and np.array_equal(bits(got), bits(rec))
    betas = rx.betas()
    cases = {"acceptance": lambda r, nl: BT.log_z_acceptance(r), "exponential": lambda r, nl: BT.log_z_exponential(r, float(n) * float(nl)),
             "ti": lambda r, nl: BT.log_z_ti(r, float(n) * float(nl), betas)}
    for method, fn in cases.items():
        value, se = rx.log_z_ratios(method, error=True)
        want, want_se = restated(rec, counts, fn)
        assert np.array_equal(bits(value), bits(rx.log_z_ratios(method))) and np.array_equal(bits(value), bits(want)), method
        assert se.shape == value.shape and np.all(se > 0) and np.all(np.isfinite(se))
        np.testing.assert_allclose(se, want_se, rtol=1e-12, atol=0.0, err_msg=method)     # (the same replicates; a sum of B squares)
    cum = lambda r, nl: np.concatenate([[0.0], np.cumsum(BT.log_z_acceptance(r))])
    value, se = rx.log_z(error=True)
    want, want_se = restated(rec, counts, cum)
    assert np.array_equal(bits(value), bits(rx.log_z())) and np.array_equal(bits(value), bits(want)) and se[0] == 0.0
    np.testing.assert_allclose(se, want_se, rtol=1e-12, atol=0.0)
    gaps_se = rx.log_z_ratios("acceptance", error=True)[1]
    assert not np.allclose(se[-1], np.sqrt((gaps_se ** 2).sum()), rtol=1e-6)      # the cumulative sum itself, not the gaps' errors added
    value, se = rx.heat_capacity(error=True)
    want, want_se = restated(rec, counts, lambda r, nl: BT.heat_capacity(r, float(n) * float(nl), betas))
    assert np.array_equal(bits(value), bits(rx.heat_capacity())) and np.array_equal(bits(value), bits(want))
    np.testing.assert_allclose(se, want_se, rtol=1e-12, atol=0.0)
    assert np.array_equal(ma.callback_log_z_error(sim), rx.log_z(error=True)[1])
    assert np.array_equal(ma.callback_heat_capacity_error(sim), se)
    plain = build(tmp_path / "plain", 24, exchange=dict(bridge=BT.ALL))           # the values do not depend on the partition by a bit
    ma.run(plain)
    assert np.array_equal(bits(plain.algorithms[1].log_z()), bits(rx.log_z()))
    with pytest.raises(ValueError, match="blocks=B"):
        plain.algorithms[1].log_z(error=True)


def test_refusals(gpu, tmp_path):
    for kw, match in ((dict(bridge=True, blocks=1), "blocks"), (dict(bridge=True, blocks=65), "blocks"), (dict(bridge=True, block_chunk=4), "without blocks"),
                      (dict(bridge=True, blocks=8, block_chunk=100), "larger than the 5 chunks"), (dict(bridge=True, blocks=16), "larger than the 8 chunks")):
        with pytest.raises(ValueError, match=match):
            build(tmp_path, 4, exchange=kw)
    with pytest.raises(ValueError, match="one partition"):
        build(tmp_path, 4, corr=[1, 2], corr_kw=dict(blocks=4, block_chunk=16))
    sim = build(tmp_path / "a", 8, corr=[1, 2, 3, 4], exchange=dict(bridge=True), corr_kw=dict(blocks=B, block_chunk=C))
    with pytest.raises(ValueError, match="would clear the bridge sums"):
        ma.run(sim)
    sim = build(tmp_path / "b", 4, exchange=dict(blocks=B, block_chunk=C))
    ma.run(sim)
    with pytest.raises(ValueError, match="bridge=True"):
        sim.algorithms[1].log_z(error=True)


@pytest.mark.parametrize("cut", [9, 11])
def test_a_checkpointed_and_resumed_run_ends_on_the_same_block_records(gpu, tmp_path, cut):
    """cut = 9: inside the origin marked at t = 4 (samples at 6, 8 taken, 10 to come); 11: behind its last sample."""
    sched = [4, 6, 8, 10, 12]
    whole = build(tmp_path / "w", 20, corr=sched)
    ma.run(whole)
    first = build(tmp_path / "a", cut, corr=[t for t in sched if t <= cut])
    ma.run(first)
    d = np.load(ma.checkpoint(first.algorithms[0], str(tmp_path / "ck")))
    assert {"bridge_blocks", "bridge_block_records", "bridge_block_snapshots", "corr_blocks"} <= set(d.files)
    assert int(d["bridge_block_snapshots"]) == cut and tuple(d["bridge_blocks"]) == (B, C) and "corr_block_records" in d.files
    second = build(tmp_path / "b", 20 - cut, corr=[t - cut for t in sched if t > cut])
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    (rx_a, ac_a), (rx_b, ac_b) = second.algorithms[1:3], whole.algorithms[1:3]
    a, b = rx_a.bridge_blocks(), rx_b.bridge_blocks()
    assert a[1] == b[1] == 20 and np.array_equal(bits(a[0]), bits(b[0]))
    assert np.array_equal(bits(rx_a.log_z(error=True)), bits(rx_b.log_z(error=True)))
    assert np.array_equal(bits(ac_a.records()), bits(ac_b.records())) and np.array_equal(bits(ac_a.block_records()[0]), bits(ac_b.block_records()[0]))
    assert np.array_equal(bits(ac_a.tau_int(error=True)[1]), bits(ac_b.tau_int(error=True)[1]))
    assert np.array_equal(bits(second.chains.x), bits(whole.chains.x))
    other = build(tmp_path / "c", 20 - cut, exchange=dict(bridge=BT.ALL, blocks=4, block_chunk=C))
    with pytest.raises(ValueError, match="partition"):
        ma.restore(other.algorithms[0], str(tmp_path / "ck"))
