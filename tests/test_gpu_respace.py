"""Respacing the ladder on the device (DESIGN.md section 3.13 "Respacing"; include/amc.h amc_respace_ladder, amc_respace_status,
amc_get_ladder) against its host twin (tests/respace_twin.py), bit for bit: beta per chain (through the sweeps and exchange steps that
follow: x, e, the Move counters), the gap counters, labels, trip counters, flow counts, the exchange step index, ladder() and
respace_status().  Shapes as in test_gpu_tracking.py: ladders that straddle wave and block boundaries, odd R, R = 7 for a label array
that is no whole number of words, one ladder alone, R = 2 (no interior rung) and R = 64.

The start ladders are CLOSE: beta_r = 0.6 x 4^(r / (R - 1)), a factor 4 from end to end whatever R is.  (With exactly equal beta, as
test_gpu_tracking.py uses to complete trips, the rule answers status 3 -- such a ladder is not strictly monotone -- so the ladders here
are as close as that allows: most swaps are accepted, walkers complete trips within 4R steps and f is informative, and some swaps are
rejected, which is what the acceptance rule divides.)"""
import numpy as np
import pytest

from montecarlo_amd.system import CustomPotential

import oracle_lib as O
import respace_twin as RT
import rung_sigma_twin as RS
from test_gpu_exchange import CUSTOM, POOLS, bits, compare, start_state
from test_gpu_tracking import raw_labels

pytestmark = pytest.mark.gpu


def close_ladder(R):
    return 0.6 * 4.0 ** (np.arange(R) / max(R - 1, 1))


def make_pair(gpu, R, L, *, potential="harmonic", dtype="f64", offset=0, n_global=None, seed=23, track=True, ladder=None, twin=True):
    """(HipEngine, RespaceTwin over the matching host simulation): the same start state, a close ladder of R rungs, tracking on."""
    M = R * L
    sigma, weight = POOLS[1]
    x = start_state(R, M, offset)[0]
    b = np.tile(close_ladder(R) if ladder is None else np.asarray(ladder, dtype=np.float64), L)
    eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=n_global or offset + M, potential=potential, beta=1.0,
                        sigma=sigma, weight=weight, seed=seed, per_chain_counters=True, dtype=dtype)
    eng.upload_state(x, b)
    eng.set_ladder(R)
    if track:
        eng.set_tracking(True)
    if not twin:
        return eng, None
    sim = O.OracleSim(M, chain_offset=offset, potential=potential, beta=1.0, sigma=sigma, weight=weight, seed=seed, dtype=dtype)
    sim.set_beta(b)
    tw = RT.RespaceTwin(sim, b, R, seed=seed, potential=potential, chain_offset=offset, f32=dtype == "f32")
    tw.state.put(x.astype(np.float32).astype(np.float64) if dtype == "f32" else x, tw.pot)
    if track:
        tw.set_tracking(True)
    return eng, tw


def compare_all(eng, tw):
    """Every compared field.  beta per chain is not downloadable; it is compared through ladder() here and, chain by chain, through
    the x and e of the sweeps and exchange steps that follow a respacing (every chain's accept decisions read its beta)."""
    assert np.array_equal(bits(eng.ladder()), bits(tw.ladder())), ("ladder() differs from the twin", eng.ladder(), tw.ladder())
    assert eng.respace_status() == (tw.status, tw.n_respaced), ("respace_status() differs from the twin", eng.respace_status(), tw.status, tw.n_respaced)
    if tw.lab is not None:
        assert np.array_equal(raw_labels(eng), tw.lab), "labels differ from the twin"
        assert eng.tracking_counters() == (tw.round_trips, tw.up_trips), ("trip counters differ from the twin", eng.tracking_counters())
        assert np.array_equal(eng.flow_rungs(), tw.flow_rungs()), "flow counts differ from the twin"
    compare(eng, tw)                                   # x, e, Move counters, gap counters, t_x


def snapshot(eng, track=True):
    x, e = eng.download_state()
    s = [bits(x), bits(e), bits(eng.ladder()), *eng.download_counters(), *eng.exchange_counters(), np.array([eng.exchange_step, eng.step])]
    if track:
        s += [raw_labels(eng), np.array(eng.tracking_counters()), eng.flow_rungs()]
    return s


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def run_and_respace(eng, tw, R, rule, gamma=1.0, eps=0.01):
    for obj in (eng, tw):
        obj.sweep_exchange(4 * R, 2)
    eng.respace_ladder(rule, gamma, eps)
    tw.respace(rule, gamma, eps)
    compare_all(eng, tw)
    for obj in (eng, tw):
        obj.sweep_exchange(8, 2)
    compare_all(eng, tw)


SHAPES = [(2, 1), (3, 1), (3, 171), (4, 129), (7, 75), (64, 9)]


@pytest.mark.parametrize("rule", ["acceptance", "flow"])
@pytest.mark.parametrize("R,L", SHAPES)
def test_respacing_matches_the_twin(gpu, R, L, rule):
    eng, tw = make_pair(gpu, R, L)
    run_and_respace(eng, tw, R, rule)
    if L > 1:
        assert tw.status == 0 and tw.n_respaced == 1          # (one ladder alone may have too few counts: then the refusal is compared)
        if R > 2:
            assert not np.array_equal(tw.ladder(), close_ladder(R))
    eng.close()


@pytest.mark.parametrize("rule", ["acceptance", "flow"])
@pytest.mark.parametrize("R,L", [(3, 171), (7, 75)])
def test_respacing_with_float32_state(gpu, R, L, rule):
    eng, tw = make_pair(gpu, R, L, dtype="f32")
    run_and_respace(eng, tw, R, rule, gamma=0.8)
    assert tw.status == 0
    lad = eng.ladder()
    assert np.array_equal(lad, lad.astype(np.float32).astype(np.float64))
    eng.close()


def test_respacing_with_a_custom_potential(gpu):
    eng, tw = make_pair(gpu, 3, 171, potential=CustomPotential(CUSTOM))
    run_and_respace(eng, tw, 3, "flow")
    assert tw.status == 0
    eng.close()


def test_two_respacings_and_an_untracked_handle(gpu):
    """Damped respacings one after the other count up; without tracking the acceptance rule needs no labels."""
    eng, tw = make_pair(gpu, 4, 129, track=False)
    for gamma in (0.5, 1.0):
        run_and_respace(eng, tw, 4, "acceptance", gamma=gamma, eps=0.0)
    assert eng.respace_status() == (0, 2)
    eng.set_ladder(4)                                          # a new ladder: nobody has respaced it
    assert eng.respace_status() == (0, 0)
    eng.close()


def test_refused_on_the_device(gpu):
    """FLOW straight after set_tracking(True): the interior rungs have no direction yet; ACCEPTANCE before any exchange step: no gap was
    attempted.  Status 2 both times, and the whole state is what it was."""
    eng, tw = make_pair(gpu, 4, 129)
    eng.sweep(2); tw.sweep(2)
    before = snapshot(eng)
    eng.respace_ladder("acceptance", 1.0, 0.01)
    assert eng.respace_status() == (2, 0) and same(snapshot(eng), before)
    eng.exchange(1); tw.exchange(1)
    eng.set_tracking(True); tw.set_tracking(True)
    before = snapshot(eng)
    eng.respace_ladder("flow", 1.0, 0.01)
    assert eng.respace_status() == (2, 0) and same(snapshot(eng), before)
    assert tw.respace("flow", 1.0, 0.01) == 2
    for obj in (eng, tw):
        obj.sweep_exchange(3, 1)
    compare_all(eng, tw)
    # a ladder that is not monotone (status 3) after one that was taken: the count stays, the status changes
    eng.close()
    eng, tw = make_pair(gpu, 3, 171, ladder=[0.6, 2.4, 1.2])
    for obj in (eng, tw):
        obj.sweep_exchange(6, 1)
    before = snapshot(eng)
    eng.respace_ladder("acceptance", 1.0, 0.01)
    assert tw.respace("acceptance", 1.0, 0.01) == 3
    assert eng.respace_status() == (3, 0) and same(snapshot(eng), before)
    eng.close()


@pytest.mark.parametrize("rule", ["acceptance", "flow"])
def test_any_split_into_shards(gpu, rule):
    """Two handles hold the ladders [0, L/2) and [L/2, L); the counts are summed on the host and given to both: together they equal
    one handle that holds all ladders (which respaces with its own counts), in every compared field."""
    R, L = 4, 130
    M, half = R * L, R * L // 2
    whole, tw = make_pair(gpu, R, L)
    parts = [make_pair(gpu, R, L // 2, offset=o, n_global=M, twin=False)[0] for o in (0, half)]
    for e in [whole, tw] + parts:
        e.sweep_exchange(4 * R, 2)
    if rule == "acceptance":
        acc, att = np.sum([p.exchange_counters() for p in parts], axis=0)
        counts = np.concatenate([att, acc])
    else:
        counts = sum(p.flow_rungs() for p in parts)
    whole.respace_ladder(rule, 0.9, 0.01)
    tw.respace(rule, 0.9, 0.01)
    for p in parts:
        p.respace_ladder(rule, 0.9, 0.01, counts=counts)
    for e in [whole, tw] + parts:
        e.sweep_exchange(8, 2)
    compare_all(whole, tw)
    assert tw.status == 0
    cat = lambda f: np.concatenate([f(p) for p in parts], axis=-1)
    assert all(np.array_equal(bits(p.ladder()), bits(whole.ladder())) and p.respace_status() == (0, 1) for p in parts)
    for i in (0, 1):
        assert np.array_equal(bits(cat(lambda p: p.download_state()[i])), bits(whole.download_state()[i]))
        assert np.array_equal(cat(lambda p: p.download_counters()[i]), whole.download_counters()[i])
        assert np.array_equal(sum(p.exchange_counters()[i] for p in parts), whole.exchange_counters()[i])
    assert np.array_equal(cat(raw_labels), raw_labels(whole))
    assert tuple(np.sum([p.tracking_counters() for p in parts], axis=0)) == whole.tracking_counters()
    assert np.array_equal(sum(p.flow_rungs() for p in parts), whole.flow_rungs())
    assert all(p.exchange_step == whole.exchange_step for p in parts)
    for e in [whole] + parts:
        e.close()


def test_stream_order(gpu):
    """sweep_exchange -> respace_ladder (local counts) -> sweep_exchange queued without a call in between that waits for the device
    equals the same sequence with a respace_status() (which synchronises) after each call."""
    R, L = 7, 75
    a, _ = make_pair(gpu, R, L, twin=False)
    b, _ = make_pair(gpu, R, L, twin=False)
    a.sweep_exchange(4 * R, 2); a.respace_ladder("flow", 1.0, 0.01); a.sweep_exchange(8, 2)
    b.sweep_exchange(4 * R, 2); b.respace_status()
    b.respace_ladder("flow", 1.0, 0.01); assert b.respace_status() == (0, 1)
    b.sweep_exchange(8, 2); b.respace_status()
    assert same(snapshot(a), snapshot(b)) and a.respace_status() == (0, 1)
    a.close(); b.close()


def test_a_handle_that_never_respaces(gpu):
    """The paths this feature does not touch: x, counters and labels of a fixed short run against the twin of tracking, as before."""
    eng, tw = make_pair(gpu, 5, 103, ladder=0.5 * 1.5 ** np.arange(5))
    for obj in (eng, tw):
        obj.sweep(1); obj.exchange(1); obj.sweep(3); obj.exchange(2); obj.sweep_exchange(4, 2)
    compare_all(eng, tw)
    assert eng.respace_status() == (0, 0) and np.array_equal(eng.ladder(), 0.5 * 1.5 ** np.arange(5))
    eng.close()


def test_widths_per_rung_stay_across_a_respacing(gpu):
    R, L = 4, 129
    M = R * L
    tab = np.array([[0.5 * 1.3 ** (-r) for r in range(R)]])
    x = start_state(R, M)[0]
    b = np.tile(close_ladder(R), L)
    eng = gpu.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=23, per_chain_counters=True)
    eng.upload_state(x, b)
    eng.set_ladder(R)
    eng.set_rung_sigma(tab)
    sim = RS.RungSigmaTwin(M, tab, potential="harmonic", beta=1.0, weight=[1.0], seed=23)
    sim.set_beta(b)
    tw = RT.RespaceTwin(sim, b, R, seed=23, potential="harmonic")
    tw.state.put(x, tw.pot)
    for obj in (eng, tw):
        obj.sweep_exchange(4 * R, 2)
    eng.respace_ladder("acceptance", 1.0, 0.01)
    assert tw.respace("acceptance", 1.0, 0.01) == 0
    assert np.array_equal(eng.rung_sigma(), tab)
    for obj in (eng, tw):
        obj.sweep_exchange(8, 2)
    assert np.array_equal(eng.rung_sigma(), tab)
    compare_all(eng, tw)
    eng.close()


def test_errors_leave_the_handle_alone(gpu):
    eng, tw = make_pair(gpu, 4, 33, track=False)
    for obj in (eng, tw):
        obj.sweep_exchange(8, 1)
    before = snapshot(eng, track=False)

    def refused(code, pattern, *a, **k):
        with pytest.raises(gpu.AmcError, match=r"amc error %d.*amc_respace_ladder.*%s" % (code, pattern)):
            eng.respace_ladder(*a, **k)
        assert same(snapshot(eng, track=False), before) and eng.respace_status() == (0, 0)

    refused(-5, "tracking is off", "flow")
    refused(-1, "rule", 3)
    refused(-1, "rule", 0)
    for gamma in (0.0, -0.5, 1.5, np.nan, np.inf):
        refused(-1, "gamma", "acceptance", gamma, 0.0)
    for eps in (-0.1, 1.0, 2.0, np.nan, np.inf):
        refused(-1, "eps", "acceptance", 1.0, eps)
    refused(-1, "counts.*gap 1", "acceptance", 1.0, 0.0, counts=[5, 5, 5, 1, 6, 1])
    with pytest.raises(gpu.AmcError, match="counts has 5 entries"):
        eng.respace_ladder("acceptance", counts=[5, 5, 5, 1, 1])
    with pytest.raises(gpu.AmcError, match="rule 'nearest'"):
        eng.respace_ladder("nearest")
    eng.respace_ladder("flow", 1.0, 0.0, counts=[[0, 8, 0], [0, 8, 0], [0, 0, 8], [0, 0, 8]])       # given flow counts need no labels
    assert eng.respace_status() == (0, 1)
    eng.set_ladder(0)
    for call in (lambda: eng.respace_ladder("acceptance"), eng.respace_status, eng.ladder):
        with pytest.raises(gpu.AmcError, match=r"amc error -5.*no ladder"):
            call()
    eng.close()
