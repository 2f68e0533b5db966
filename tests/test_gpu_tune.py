"""Tuning the widths per rung on the device (DESIGN.md section 3.13 "Tuning the widths"; include/amc.h amc_tune_rung_sigma,
amc_tune_status, amc_rung_window_*) against its host twin (tests/tune_twin.py), bit for bit: the table and the status per entry, and --
through the sweeps and exchange steps that follow -- x, e, the Move counters, the gap counters and the step indices, which pins the
four derived rows the tuning kernel rewrites.  Shapes: K = 1 with R = 2, 3, 4, 7, 64; K = 2 with R = 3 and R = 32 (all 64 entries);
K = 5 with R = 3 (two move groups in the totals kernel, a last move without a total array); 1, 2, 257 and 30 001 ladders."""
import numpy as np
import pytest

import tune_twin as TT
from test_gpu_rung_sigma import bits, compare, make_engine, pool, start_state, table

pytestmark = pytest.mark.gpu


def make_pair(gpu, K, R, L, *, potential="harmonic", dtype="f64", offset=0, n_global=None, twin=True, tab=None):
    tab = table(K, R) if tab is None else tab
    eng = make_engine(gpu, R, L, K, tab=tab, potential=potential, dtype=dtype, offset=offset, n_global=n_global)
    if not twin:
        return eng, None
    M = R * L
    x, beta = start_state(R, M, offset)
    tw = TT.TuneTwin(M, tab, beta, R, seed=23, potential=potential, chain_offset=offset, weight=pool(K)[1], dtype=dtype)
    tw.state.put(x.astype(np.float32).astype(np.float64) if dtype == "f32" else x, tw.pot)
    return eng, tw


def compare_tuning(eng, tw):
    st, n = eng.tune_status()
    assert np.array_equal(st, tw.status) and n == tw.n_tuned, ("tune_status() differs from the twin", st, tw.status, n, tw.n_tuned)
    assert np.array_equal(bits(eng.rung_sigma()), bits(tw.table)), ("the table differs from the twin", eng.rung_sigma(), tw.table)
    acc, tot = eng.rung_window_base()
    assert np.array_equal(acc, tw.base[0]) and np.array_equal(tot, tw.base[1]), "the window base differs from the twin"


def tune_both(eng, tw, **kw):
    eng.tune_rung_sigma(kw.get("target", 0.44), kw.get("gamma", 1.0), kw.get("min_calls", 4), kw.get("lo", 1e-100), kw.get("hi", 1e100))
    tw.tune(**kw)


def run_and_tune(eng, tw, exchange=True):
    for obj in (eng, tw):
        obj.sweep(6)
        if exchange:
            obj.exchange(1)
        obj.sweep(4)
    tune_both(eng, tw, target=0.44, gamma=0.8, min_calls=4)
    compare_tuning(eng, tw)
    for obj in (eng, tw):
        obj.sweep(3)
        if exchange:
            obj.exchange(2)
        obj.sweep(2)
    compare(eng, tw)
    tune_both(eng, tw, target=0.3, gamma=1.0, min_calls=4, lo=0.05, hi=0.6)
    compare_tuning(eng, tw)
    for obj in (eng, tw):
        obj.sweep(2)
    compare(eng, tw)


@pytest.mark.parametrize("K,R,L", [(1, 2, 1), (1, 3, 2), (1, 4, 257), (1, 7, 75), (1, 64, 9), (2, 3, 171), (2, 32, 9), (5, 3, 103)])
def test_tuning_matches_the_twin(gpu, K, R, L):
    eng, tw = make_pair(gpu, K, R, L)
    run_and_tune(eng, tw)
    if L > 2:
        assert tw.n_tuned == 2 and not np.array_equal(tw.table, table(K, R))
    eng.close()


def test_thirty_thousand_ladders(gpu):
    """More chains than one trip of the totals kernel's grid; sweeps only (the twin's exchange step is a Python loop over the ladders)."""
    eng, tw = make_pair(gpu, 2, 3, 30001)
    run_and_tune(eng, tw, exchange=False)
    assert np.all(tw.status != 1) and tw.n_tuned == 2
    eng.close()


@pytest.mark.parametrize("kw", [dict(potential="double_well"), dict(dtype="f32")], ids=["double_well", "f32"])
def test_tuning_in_the_other_forms(gpu, kw):
    eng, tw = make_pair(gpu, 2, 3, 171, **kw)
    run_and_tune(eng, tw)
    assert tw.n_tuned == 2
    eng.close()


def test_chain_offsets_across_2_to_the_32(gpu):
    R, L = 4, 129
    offset = 2 ** 32 - R * 64
    eng, tw = make_pair(gpu, 1, R, L, offset=offset, n_global=offset + R * L)
    run_and_tune(eng, tw)
    assert tw.n_tuned == 2
    eng.close()


def test_counters_uploaded_above_65536(gpu):
    """u16 planes with their high planes (K = 2 keeps narrow counters) and, beyond 2^32, the carried 64-bit bases: the window is formed
    from every storage the counters have."""
    K, R, L = 2, 3, 57
    M = R * L
    for steps in (70000, 2 ** 32 + 70000):
        eng, tw = make_pair(gpu, K, R, L)
        ids = np.arange(M)
        tot0 = steps // 2 + (ids % 11)
        tot = np.array([tot0, steps - tot0], dtype=np.int64)
        acc = np.array([tot0 // 3 + (ids % 5), (steps - tot0) // 2 - (ids % 3)], dtype=np.int64)
        eng.upload_counters(acc, tot)
        tw.sim.acc[:], tw.sim.tot[:] = acc, tot
        ra, rt = eng.rung_counter_totals()
        assert np.array_equal(ra, tw.rung_totals()[0]) and np.array_equal(rt, tw.rung_totals()[1])
        tune_both(eng, tw, target=0.44, min_calls=1000)          # the first window: since the counters began
        compare_tuning(eng, tw)
        assert np.all(tw.status == 0)
        for obj in (eng, tw):
            obj.sweep(5)
        tune_both(eng, tw, target=0.44, min_calls=4)
        compare_tuning(eng, tw)
        x, xo = eng.download_state()[0], tw.sim.state()[0]
        assert np.array_equal(bits(x), bits(xo))
        a, t = eng.download_counters()
        assert np.array_equal(a, tw.sim.acc) and np.array_equal(t, tw.sim.tot)
        eng.close()


def test_stream_order(gpu):
    """Sweeps, a tuning, sweeps, exchange steps, a tuning, sweeps queued with nothing that waits for the device in between: the final
    state is the twin's.  A tuning with every cell under min_calls leaves the table's bits, and the base still moves."""
    eng, tw = make_pair(gpu, 2, 3, 171)
    eng.sweep(7); eng.tune_rung_sigma(0.44, 0.7, 4, 1e-100, 1e100); eng.sweep(3); eng.exchange(2)
    eng.tune_rung_sigma(0.5, 1.0, 4, 1e-100, 1e100); eng.sweep(4)
    tw.sweep(7); tw.tune(0.44, 0.7, 4); tw.sweep(3); tw.exchange(2); tw.tune(0.5, 1.0, 4); tw.sweep(4)
    compare(eng, tw)
    compare_tuning(eng, tw)
    before = bits(eng.rung_sigma()).copy()
    tune_both(eng, tw, target=0.44, min_calls=10 ** 9)
    compare_tuning(eng, tw)
    assert np.all(tw.status == 1) and np.array_equal(bits(eng.rung_sigma()), before) and eng.tune_status()[1] == 2
    assert np.array_equal(eng.rung_window_base()[1], eng.rung_counter_totals()[1])
    assert np.all(eng.rung_window_counts()[1] == 0)
    eng.close()


def test_the_window(gpu):
    eng, tw = make_pair(gpu, 1, 4, 129)
    eng.sweep(5); tw.sweep(5)
    first = eng.rung_counter_totals()
    assert all(np.array_equal(w, f) for w, f in zip(eng.rung_window_counts(), first))           # the first window: since the counters began
    eng.rung_window_restart(); tw.restart()
    assert all(np.array_equal(b, f) for b, f in zip(eng.rung_window_base(), first))
    eng.sweep(6); tw.sweep(6)
    second = eng.rung_counter_totals()
    assert all(np.array_equal(w, s - f) for w, s, f in zip(eng.rung_window_counts(), second, first))
    assert np.all(eng.rung_window_counts()[1] == 6 * 129)
    # counters replaced below the base at rung 1: -1 / -1 there and status 2, the rest of the table still tunes
    acc, _ = eng.download_counters()
    acc[:, 1::4] = 0
    eng.upload_counters(acc)
    tw.sim.acc[:, 1::4] = 0
    wa, wt = eng.rung_window_counts()
    assert np.all(wa[:, 1] == -1) and np.all(wt[:, 1] == -1) and np.all(wa[:, [0, 2, 3]] >= 0) and np.all(wt[:, [0, 2, 3]] == 6 * 129)
    tune_both(eng, tw, target=0.44, min_calls=4)
    compare_tuning(eng, tw)
    assert tw.status[0].tolist() == [0, 2, 0, 0] and bits(tw.table)[0, 1] == bits(table(1, 4))[0, 1]
    for obj in (eng, tw):
        obj.sweep(3)
    compare(eng, tw)
    eng.close()


def snapshot(eng, table_too=True):
    x, e = eng.download_state()
    s = [bits(x), bits(e), *eng.download_counters(), *eng.exchange_counters(), np.array([eng.exchange_step, eng.step]), *eng.rung_counter_totals(),
         np.array(eng.counter_totals())]
    if table_too:
        s += [bits(eng.rung_sigma()), eng.tune_status()[0], np.array([eng.tune_status()[1]]), *eng.rung_window_base()]
    return s


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def test_a_tuned_then_cleared_handle_equals_one_that_never_tuned(gpu):
    """The Move counters are never written and nothing but the table's rows changes: with the widths in force equal -- a tuning under
    min_calls keeps every width -- a handle that tunes, restarts its window and then drops its table ends where a handle that does
    none of it ends, in x, e, the step indices, the Move counters and their totals, the gap counters, the labels and the records of
    a callback reduction."""
    from test_gpu_tracking import raw_labels
    a, _ = make_pair(gpu, 2, 3, 171, twin=False)
    b, _ = make_pair(gpu, 2, 3, 171, twin=False)
    for eng in (a, b):
        eng.set_tracking(True)
        eng.sweep(5); eng.exchange(1)
    a.tune_rung_sigma(0.44, 1.0, 10 ** 9, 1e-100, 1e100)
    a.rung_window_restart()
    for eng in (a, b):
        eng.sweep(3); eng.exchange(2)
    assert same(snapshot(a, False), snapshot(b, False)) and np.array_equal(a.rung_sigma(), b.rung_sigma())
    for eng in (a, b):
        eng.set_rung_sigma(None)
        eng.sweep(4); eng.exchange(1); eng.sweep(1)
    assert same(snapshot(a, False), snapshot(b, False))
    assert np.array_equal(raw_labels(a), raw_labels(b)) and a.tracking_counters() == b.tracking_counters()
    ra, rb = a.reduce_exact(), b.reduce_exact()
    assert np.array_equal(bits(ra[0]), bits(rb[0])) and ra[1] == rb[1]
    a.close(); b.close()


def test_any_split_into_shards(gpu):
    """Three handles hold a third of the ladders each; their windows are summed on the host and given to all three: same table bits as
    one handle that holds all ladders and tunes with its own window, same chains afterwards."""
    K, R, L = 2, 3, 174                # (a third is 58 ladders, 174 chains: shards start on chain pairs)
    M, third = R * L, R * L // 3
    whole, _ = make_pair(gpu, K, R, L, twin=False)
    parts = [make_pair(gpu, K, R, L // 3, offset=o, n_global=M, twin=False)[0] for o in (0, third, 2 * third)]
    for rnd in range(2):
        for e in [whole] + parts:
            e.sweep(5); e.exchange(1); e.sweep(2)
        counts = tuple(np.sum([p.rung_window_counts()[i] for p in parts], axis=0) for i in (0, 1))
        assert all(np.array_equal(c, w) for c, w in zip(counts, whole.rung_window_counts()))
        whole.tune_rung_sigma(0.44, 0.9, 4, 1e-100, 1e100)
        for p in parts:
            p.tune_rung_sigma(0.44, 0.9, 4, 1e-100, 1e100, counts=counts)
        for p in parts:
            assert np.array_equal(bits(p.rung_sigma()), bits(whole.rung_sigma()))
            assert np.array_equal(p.tune_status()[0], whole.tune_status()[0]) and p.tune_status()[1] == rnd + 1
            assert np.all(p.rung_window_counts()[1] == 0)               # the base moved to the shard's own totals
    assert not np.array_equal(whole.rung_sigma(), table(K, R))
    for e in [whole] + parts:
        e.sweep(3); e.exchange(2); e.sweep(1)
    cat = lambda f: np.concatenate([f(p) for p in parts], axis=-1)
    for i in (0, 1):
        assert np.array_equal(bits(cat(lambda p: p.download_state()[i])), bits(whole.download_state()[i]))
        assert np.array_equal(cat(lambda p: p.download_counters()[i]), whole.download_counters()[i])
        assert np.array_equal(sum(p.exchange_counters()[i] for p in parts), whole.exchange_counters()[i])
    for e in [whole] + parts:
        e.close()


def test_get_rung_sigma_and_the_resets(gpu):
    K, R, L = 2, 3, 57
    tab = table(K, R)
    eng, tw = make_pair(gpu, K, R, L)
    assert np.array_equal(eng.rung_sigma(), tab) and eng.tune_status()[1] == 0 and np.all(eng.tune_status()[0] == 0)
    for obj in (eng, tw):
        obj.sweep(8)
    tune_both(eng, tw, target=0.44, min_calls=4)
    compare_tuning(eng, tw)
    assert not np.array_equal(eng.rung_sigma(), tab) and eng.tune_status()[1] == 1
    base = eng.rung_window_base()
    eng.set_rung_sigma(tab * 0.5)                              # a table that is given: the record starts over, the window stays
    assert np.array_equal(eng.rung_sigma(), tab * 0.5) and eng.tune_status()[1] == 0 and np.all(eng.tune_status()[0] == 0)
    assert same(eng.rung_window_base(), base)
    eng.set_tuned(7)
    assert eng.tune_status()[1] == 7
    eng.sweep(2)
    eng.tune_rung_sigma(0.44, 1.0, 4, 1e-100, 1e100)
    assert eng.tune_status()[1] == 8
    eng.set_ladder(R)                                          # a ladder that is set: no table, no record, no base
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*amc_get_rung_sigma"):
        eng.rung_sigma()
    assert np.all(eng.rung_window_base()[1] == 0)
    eng.set_rung_sigma(tab)
    assert np.array_equal(eng.rung_sigma(), tab) and eng.tune_status()[1] == 0
    eng.close()


def test_refusals_leave_the_handle_alone(gpu):
    K, R, L = 2, 3, 57
    eng, _ = make_pair(gpu, K, R, L, twin=False)
    eng.sweep(6); eng.exchange(1)
    eng.tune_rung_sigma(0.44, 1.0, 4, 1e-100, 1e100)
    eng.sweep(2)
    before = snapshot(eng)

    def refused(code, pattern, *a, **k):
        with pytest.raises(gpu.AmcError, match=r"amc error %d.*amc_tune_rung_sigma.*%s" % (code, pattern)):
            eng.tune_rung_sigma(*a, **k)
        assert same(snapshot(eng), before)

    for target in (0.0, 1.0, -0.2, 1.5, np.nan, np.inf):
        refused(-1, "target", target, 1.0, 4, 1e-100, 1e100)
    for gamma in (0.0, -0.5, 1.5, np.nan, np.inf):
        refused(-1, "gamma", 0.44, gamma, 4, 1e-100, 1e100)
    for min_calls in (0, -3):
        refused(-1, "min_calls", 0.44, 1.0, min_calls, 1e-100, 1e100)
    for lo in (0.0, 1e-101, 1e101, np.nan, -1.0):
        refused(-1, "sigma_lo", 0.44, 1.0, 4, lo, 1e100)
    for hi in (0.0, 1e101, np.nan, np.inf):
        refused(-1, "sigma_hi", 0.44, 1.0, 4, 1e-100, hi)
    refused(-1, "sigma_lo.*above", 0.44, 1.0, 4, 2.0, 1.0)
    good = np.full((K, R), 50)
    neg, more = good.copy(), good.copy()
    neg[1, 2], more[0, 1] = -1, 51
    refused(-1, "counts.*entry 5.*negative", 0.44, 1.0, 4, 1e-100, 1e100, counts=(neg, good))
    refused(-1, "counts.*entry 1.*more accepted", 0.44, 1.0, 4, 1e-100, 1e100, counts=(more, good))
    with pytest.raises(gpu.AmcError, match="counts has 10 entries"):
        eng.tune_rung_sigma(0.44, 1.0, 4, 1e-100, 1e100, counts=(good.reshape(-1)[:5], good.reshape(-1)[:5]))
    assert same(snapshot(eng), before)
    eng.set_rung_sigma(None)                                   # no table
    for call in (lambda: eng.tune_rung_sigma(0.44, 1.0, 4, 1e-100, 1e100), eng.tune_status):
        with pytest.raises(gpu.AmcError, match=r"amc error -5.*no widths per rung"):
            call()
    assert eng.rung_window_counts()[0].shape == (K, R)         # the window needs no table
    eng.set_ladder(0)                                          # no ladder
    for call in (eng.rung_window_counts, eng.rung_window_restart, eng.rung_window_base):
        with pytest.raises(gpu.AmcError, match=r"amc error -5.*no ladder"):
            call()
    eng.close()
    # no per-chain counters
    plain = gpu.HipEngine(n_chains=12, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=3, per_chain_counters=False)
    x, beta = start_state(3, 12)
    plain.upload_state(x, beta)
    plain.set_ladder(3)
    for call in (lambda: plain.tune_rung_sigma(0.44, 1.0, 4, 1e-100, 1e100), plain.rung_window_counts, plain.rung_window_restart):
        with pytest.raises(gpu.AmcError, match=r"amc error -5.*per_chain_counters"):
            call()
    plain.close()
