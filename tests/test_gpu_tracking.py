"""Walker tracking on the device (DESIGN.md section 3.13 "Walker tracking"; include/amc.h amc_set_tracking .. amc_set_tracking_counters)
against its host twin (tests/track_twin.py), bit for bit: the label bytes, both trip counters and the flow counts, and -- because a
tracked handle launches another kernel -- positions, energies, the Move counters, the gap counters and the exchange step index as
well.  Shapes as in test_gpu_exchange.py (ladders that straddle wave and block boundaries, odd R, R = 2 where both end rules fire at
the one gap, a single ladder), R = 7 for a label array that is no whole number of 4-byte words, and equal-beta runs of 4R steps,
which are what completes trips."""
import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd.system import CustomPotential

import oracle_lib as O
import track_twin as T
from test_gpu_exchange import CUSTOM, POOLS, bits, compare, start_state

pytestmark = pytest.mark.gpu


def make_pair(gpu, R, L, *, potential="harmonic", dtype="f64", param_dtype="f64", offset=0, n_global=None, seed=23, K=1, beta=None, track=True):
    """(HipEngine, TrackTwin over the matching host simulation): the same start state, a ladder of R rungs, tracking on."""
    M = R * L
    sigma, weight = POOLS[K]
    x, b = start_state(R, M, offset)
    if beta is not None:
        b = np.full(M, float(beta))
    eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=n_global or offset + M, potential=potential, beta=1.0,
                        sigma=sigma, weight=weight, seed=seed, per_chain_counters=True, dtype=dtype, param_dtype=param_dtype)
    eng.upload_state(x, b)
    eng.set_ladder(R)
    if param_dtype == "f32":
        import f32_param_twin as F
        sim = F.TwinSim(M, chain_offset=offset, potential=potential, beta=1.0, sigma=sigma, weight=weight, seed=seed)
        sim.beta[:] = b.astype(np.float32)
    else:
        sim = O.OracleSim(M, chain_offset=offset, potential=potential, beta=1.0, sigma=sigma, weight=weight, seed=seed, dtype=dtype)
        sim.set_beta(b)
    tw = T.TrackTwin(sim, b, R, seed=seed, potential=potential, chain_offset=offset, f32=dtype == "f32")
    tw.state.put(x.astype(np.float32).astype(np.float64) if dtype == "f32" else x, tw.pot)
    if track:
        eng.set_tracking(True)
        tw.set_tracking(True)
    return eng, tw


def raw_labels(eng):
    w, d = eng.labels()
    return w | (d << np.uint8(6))


def compare_tracking(eng, tw):
    assert np.array_equal(raw_labels(eng), tw.lab), "labels differ from the twin"
    assert eng.tracking_counters() == (tw.round_trips, tw.up_trips), ("trip counters differ from the twin", eng.tracking_counters())
    flow = eng.flow_rungs()
    assert flow.dtype == np.int64 and np.array_equal(flow, tw.flow_rungs()), "flow counts differ from the twin"
    compare(eng, tw)                                   # x, e, Move counters, gap counters, t_x


def interleave(eng, tw):
    """test_gpu_exchange.interleave with the tracking state compared too: after the separate calls and at the end."""
    for obj in (eng, tw):
        obj.sweep(1); obj.exchange(1); obj.sweep(3); obj.exchange(2)
    compare_tracking(eng, tw)
    for obj in (eng, tw):
        obj.sweep_exchange(4, 2)
    compare_tracking(eng, tw)
    T.check_labels(raw_labels(eng), tw.R)


@pytest.mark.parametrize("R,L", [(2, 1), (2, 513), (3, 1), (3, 171), (4, 129), (7, 75), (64, 9)])
def test_tracking_matches_the_twin(gpu, R, L):
    eng, tw = make_pair(gpu, R, L)
    interleave(eng, tw)
    eng.close()


@pytest.mark.parametrize("R", [2, 3, 4])
def test_equal_beta_completes_trips(gpu, R):
    """Every attempted swap is accepted; after 4R steps every walker is back (tests/test_tracking_host.py works the numbers out by hand)."""
    L = 171
    eng, tw = make_pair(gpu, R, L, beta=1.25)
    for i in range(4):
        eng.exchange(R); tw.exchange(R)
        compare_tracking(eng, tw)
    rt, up = eng.tracking_counters()
    assert (rt, up) == {2: (4 * L, 4 * L), 3: (5 * L, 6 * L), 4: (7 * L, 7 * L)}[R] and rt > 0 and up > 0
    assert np.array_equal(eng.labels()[0], np.tile(np.arange(R, dtype=np.uint8), L))
    eng.close()


@pytest.mark.parametrize("potential,dtype,param_dtype", [("double_well", "f64", "f64"), ("harmonic", "f32", "f64"), ("double_well", "f32", "f32"),
                                                          (CustomPotential(CUSTOM), "f64", "f64")])
def test_tracking_with_other_models(gpu, potential, dtype, param_dtype):
    """The other built-in instantiation, and the tracked kernel as the run-time compiler builds it (Float32 state, a custom potential)."""
    eng, tw = make_pair(gpu, 3, 171, potential=potential, dtype=dtype, param_dtype=param_dtype)
    interleave(eng, tw)
    eng.close()


def test_grid_stride(gpu, monkeypatch):
    """One block per CU.  3 x 30 001 gaps per even step walk exchange_tracked_kernel's grid more than once; the labels of that handle
    are 45 002 words, one pass of 256 blocks, so rung_flow_kernel's loop is walked more than once by a second handle of 6 x 50 001
    labels, checked against a count of its downloaded labels (the flow counts are a function of the labels and of nothing else)."""
    monkeypatch.setenv("AMC_BLOCKS_PER_CU", "1")
    eng, tw = make_pair(gpu, 6, 30001)
    big, _ = make_pair(gpu, 6, 50001, track=False)
    monkeypatch.delenv("AMC_BLOCKS_PER_CU")
    for obj in (eng, tw):
        obj.sweep(1); obj.exchange(2)
    compare_tracking(eng, tw)
    eng.close()
    big.set_tracking(True)
    big.sweep(1); big.exchange(3)
    lab = raw_labels(big)
    T.check_labels(lab, 6)
    assert not np.array_equal(lab, T.initial_labels(lab.size, 6))
    assert np.array_equal(big.flow_rungs(), T.flow_counts(lab, 6))
    big.close()


def test_shard_invariance(gpu):
    """The global range as one handle and as two and three handles whose offsets are multiples of R: the concatenated labels are the
    whole's, trip counters and flow counts add up to the whole's."""
    R, L = 3, 342
    M = R * L
    whole, tw = make_pair(gpu, R, L, potential="double_well", K=2)
    seq = lambda o: (o.sweep(2), o.exchange(1), o.sweep(1), o.exchange(2), o.sweep_exchange(5, 1))
    seq(whole); seq(tw)
    compare_tracking(whole, tw)
    lab_w, trips_w, flow_w = raw_labels(whole), whole.tracking_counters(), whole.flow_rungs()
    for split in ([0, 402, M], [0, 258, 264, M]):
        parts = [make_pair(gpu, R, (b - a) // R, potential="double_well", K=2, offset=a, n_global=M)[0] for a, b in zip(split, split[1:])]
        for p in parts:
            seq(p)
        assert np.array_equal(np.concatenate([raw_labels(p) for p in parts]), lab_w)
        assert tuple(np.sum([p.tracking_counters() for p in parts], axis=0)) == trips_w
        assert np.array_equal(sum(p.flow_rungs() for p in parts), flow_w)
        for p in parts:
            p.close()
    whole.close()


def test_a_tracked_and_an_untracked_handle_agree(gpu):
    a, _ = make_pair(gpu, 5, 205, potential="double_well", K=2)
    b, _ = make_pair(gpu, 5, 205, potential="double_well", K=2, track=False)
    for e in (a, b):
        e.sweep(2); e.exchange(3); e.sweep_exchange(6, 1)
    (xa, ea), (xb, eb) = a.download_state(), b.download_state()
    assert np.array_equal(bits(xa), bits(xb)) and np.array_equal(bits(ea), bits(eb))
    assert all(np.array_equal(u, v) for u, v in zip(a.download_counters(), b.download_counters()))
    assert all(np.array_equal(u, v) for u, v in zip(a.exchange_counters(), b.exchange_counters()))
    assert a.exchange_step == b.exchange_step == 9 and a.step == b.step and a.estimator_step == b.estimator_step == 0
    assert a.exchange_counters()[0].sum() > 0
    a.close(); b.close()


def test_a_handle_without_tracking(gpu):
    """The new getters are refused with AMC_ERR_STATE, before and after an exchange step (which allocates no label buffer), and
    tracking cannot be turned on without a ladder."""
    eng, _ = make_pair(gpu, 3, 60, track=False)

    def refused():
        for call in (eng.labels, eng.flow_rungs, eng.tracking_counters, lambda: eng.set_tracking_counters(1, 1),
                     lambda: eng.set_labels(np.tile([0, 1, 2], 60), np.tile([1, 0, 2], 60))):
            with pytest.raises(gpu.AmcError, match=r"amc error -5.*tracking is off"):
                call()
    refused()
    eng.exchange(2); eng.sweep_exchange(1, 1)
    refused()
    eng.set_tracking(False)                                    # off already: nothing to do
    eng.set_ladder(0)
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*no ladder"):
        eng.set_tracking(True)
    refused()
    eng.close()


def test_labels_round_trip_and_refusals_leave_them_alone(gpu):
    R, L = 4, 33
    eng, tw = make_pair(gpu, R, L, beta=1.25)
    eng.exchange(3); tw.exchange(3)
    compare_tracking(eng, tw)
    w, d = eng.labels()
    assert w.dtype == d.dtype == np.uint8
    eng.set_labels(w, d)                                       # set_labels(labels()) changes nothing
    compare_tracking(eng, tw)
    trips = eng.tracking_counters()

    def bad(c, what, **change):
        w2, d2 = w.astype(np.int64), d.astype(np.int64)
        for k, v in change.items():
            (w2 if k == "w" else d2)[c] = v
        with pytest.raises(gpu.AmcError, match=r"amc error -1.*chain %d\b.*%s" % (c, what)):
            eng.set_labels(w2, d2)
        assert np.array_equal(raw_labels(eng), tw.lab) and eng.tracking_counters() == trips

    bad(6, "walker id 4 >= n_rungs", w=4)
    bad(9, "direction 3", d=3)
    bad(8, "rung 0", d=2)
    bad(8, "rung 0", d=0)
    bad(11, "rung 3", d=1)
    w2 = w.copy()
    w2[13] = w2[12]                                            # ladder 3 = chains 12 .. 15: the id of chain 12 a second time
    with pytest.raises(gpu.AmcError, match=r"amc error -1.*chain 13\b.*permutation"):
        eng.set_labels(w2, d)
    assert np.array_equal(raw_labels(eng), tw.lab) and eng.tracking_counters() == trips
    with pytest.raises(gpu.AmcError, match="one walker id and one direction per local chain"):
        eng.set_labels(w[:-1], d[:-1])
    with pytest.raises(gpu.AmcError, match=r"amc error -1"):
        eng.set_tracking_counters(-1, 0)
    # a valid upload is taken: the identity labels again, other counters
    eng.set_labels(*[a.astype(np.uint8) for a in (T.initial_labels(R * L, R) & 63, T.initial_labels(R * L, R) >> 6)])
    eng.set_tracking_counters(7, 11)
    tw.set_tracking(True); tw.round_trips, tw.up_trips = 7, 11
    eng.exchange(2); tw.exchange(2)
    compare_tracking(eng, tw)
    eng.close()


def test_set_ladder_turns_tracking_off_and_upload_state_leaves_labels_alone(gpu):
    eng, tw = make_pair(gpu, 3, 171)
    eng.sweep(1); eng.exchange(2); tw.sweep(1); tw.exchange(2)
    x, beta = start_state(3, 513)
    eng.upload_state(x, beta); tw.state.put(x, tw.pot)
    compare_tracking(eng, tw)                                  # new positions, the labels and counters as they were
    eng.exchange(1); tw.exchange(1)
    compare_tracking(eng, tw)
    for R in (3, 0):                                           # the same ladder again, and none
        eng.set_tracking(True)
        eng.set_ladder(R)
        with pytest.raises(gpu.AmcError, match=r"amc error -5.*tracking is off"):
            eng.labels()
    eng.set_ladder(9)                                          # 513 = 9 x 57
    eng.set_tracking(True)
    assert np.array_equal(raw_labels(eng), T.initial_labels(513, 9)) and eng.tracking_counters() == (0, 0)
    assert eng.flow_rungs().tolist() == [[0, 57, 0]] + [[57, 0, 0]] * 7 + [[0, 0, 57]]
    eng.close()


def test_checkpoint_after_an_odd_number_of_exchange_steps(gpu, tmp_path):
    def build(path, steps):
        chains = ma.ParticleChains.ladder(171, [0.5, 0.7, 1.0], x=start_state(3, 513)[0], potential="double_well")
        pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
        al = [dict(algorithm=ma.Metropolis, pool=pool, seed=4, per_chain_counters=True),
              dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), track=True)]
        return ma.Simulation(chains, al, steps, path=str(path))
    whole = build(tmp_path / "w", 22)
    ma.run(whole)
    first = build(tmp_path / "a", 14)
    ma.run(first)
    assert first.algorithms[0].engine.exchange_step == 7
    ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    second = build(tmp_path / "b", 8)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    e1, e2 = whole.algorithms[0].engine, second.algorithms[0].engine
    assert np.array_equal(bits(whole.chains.x), bits(second.chains.x))
    assert e1.exchange_step == e2.exchange_step == 11
    assert np.array_equal(raw_labels(e1), raw_labels(e2)) and np.array_equal(e1.flow_rungs(), e2.flow_rungs())
    assert e1.tracking_counters() == e2.tracking_counters() and e1.tracking_counters()[0] > 0
    f, trips = whole.algorithms[1].flow(), whole.algorithms[1].round_trips()
    assert f[0] == 1.0 and f[2] == 0.0 and 0.0 < f[1] < 1.0 and trips.tolist() == list(e1.tracking_counters())
