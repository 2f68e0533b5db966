"""Choosing the next beta on the device (DESIGN.md section 3.14 "Choosing the next beta"; include/amc.h amc_anneal_next_beta) against
its host twin (tests/anneal_search_twin.py), bit for bit: beta_new, the eight diag words and the whole trace of integer sums.  Shapes
are the smallest at which the kernels take another path: one chain, wave (64) and block (256) boundaries, several blocks, odd sizes,
and one ensemble that walks a one-block-per-CU grid more than once."""
import math

import numpy as np
import pytest

from montecarlo_amd.system import CustomPotential

import anneal_search_twin as S
import anneal_twin as A
import oracle_lib as O

pytestmark = pytest.mark.gpu
CUSTOM = "x*x*x*x - 2.0*x*x + 0.25*x"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def start_x(M):
    ids = np.arange(M)
    return 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)


def make_pair(gpu, M, *, x=None, beta=0.5, potential="harmonic", dtype="f64", families=False, seed=23):
    """(HipEngine, AnnealTwin over the matching OracleSim), both holding the same start state at the same shared beta."""
    x = start_x(M) if x is None else np.asarray(x, dtype=np.float64)
    if dtype == "f32":
        x = x.astype(np.float32).astype(np.float64)
    eng = gpu.HipEngine(n_chains=M, potential=potential, beta=beta, sigma=[0.5], weight=[1.0], seed=seed, dtype=dtype, per_chain_counters=True)
    eng.upload_state(x)
    sim = O.OracleSim(M, potential=potential, beta=beta, sigma=[0.5], weight=[1.0], seed=seed, dtype=dtype)
    sim.set_x(x)
    tw = A.AnnealTwin(sim, beta, seed=seed, potential=potential, f32=dtype == "f32", families=families)
    if families:
        eng.set_anneal_families(True)
    return eng, tw


def search(eng, tw, limit, target, rounds):
    """One search on both; beta_new, diag and the trace compared bit for bit.  Returns the device's answer."""
    b, diag, trace = eng.anneal_next_beta(limit, target, rounds)
    bo, do, to = S.twin_next_beta(tw, limit, target, rounds)
    assert np.array_equal(trace, to), ("the sums differ from the twin", np.argwhere(trace != to)[:6].tolist())
    assert diag.tolist() == do.tolist(), ("diag differs from the twin", diag.tolist(), do.tolist())
    assert A.f64_bits(b) == A.f64_bits(bo)
    assert eng.beta == tw.beta                                      # a search moves nothing
    return b, diag, trace


def compare(eng, tw):
    """(test_gpu_anneal.py's helper) positions, energies, beta, the step index, the records, the families, the counters."""
    x, e = eng.download_state()
    xo, eo = tw.sim.state()
    assert np.array_equal(bits(x), bits(xo)), ("positions differ from the twin", np.flatnonzero(bits(x) != bits(xo))[:8])
    assert np.array_equal(bits(e), bits(eo)), "energies differ from the twin"
    assert eng.beta == tw.beta and eng.anneal_step == tw.t_a
    rec = eng.anneal_records()
    assert np.array_equal(rec, tw.records_array()), ("records differ from the twin", rec.tolist(), tw.records)
    if tw.fam is not None:
        assert np.array_equal(eng.download_families(), tw.fam), "families differ from the twin"
        assert eng.anneal_family_stats() == tw.family_stats()
    ao, to = tw.sim.counters()
    acc, tot = eng.download_counters()
    assert np.array_equal(acc, ao) and np.array_equal(tot, to), "Move counters differ from the twin"
    assert eng.step == tw.sim.step


def cool_and_heat(eng, tw, rounds=3):
    """A sweep, a search towards a cold limit, the step taken, a search back towards a hot one."""
    for o in (eng, tw):
        o.sweep(1)
    b, diag, _ = search(eng, tw, 6.0, 0.8, rounds)
    for o in (eng, tw):
        o.anneal(b)
    search(eng, tw, 0.125, 0.6, 2)
    return diag


@pytest.mark.parametrize("potential", ["harmonic", "double_well"])
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 3075])
def test_search_matches_the_twin(gpu, M, potential):
    eng, tw = make_pair(gpu, M, potential=potential)
    diag = cool_and_heat(eng, tw)
    print(f"M = {M}, {potential}: status {int(diag[0])}, step {A.bits_f64(diag[2])!r}")
    assert diag[0] == (S.LIMIT if M == 1 else S.OK) or M == 2
    compare(eng, tw)
    eng.close()


@pytest.mark.parametrize("potential", ["harmonic", "double_well", CustomPotential(CUSTOM)])
def test_search_with_float32_state(gpu, potential):
    eng, tw = make_pair(gpu, 1025, potential=potential, dtype="f32")
    cool_and_heat(eng, tw)
    b, diag, _ = search(eng, tw, 0.7, 0.9, 6)                       # six rounds: the candidates are rounded to Float32
    assert float(np.float32(A.bits_f64(diag[2]))) == A.bits_f64(diag[2]) and float(np.float32(b)) == b
    eng.close()


def test_search_with_a_custom_potential(gpu):
    eng, tw = make_pair(gpu, 1025, potential=CustomPotential(CUSTOM))
    cool_and_heat(eng, tw, rounds=6)
    eng.close()


def test_a_grid_walked_twice_and_grid_independence(gpu, monkeypatch):
    """70 001 chains: with one block per CU (256 blocks x 256 threads) the chain passes walk their grid more than once.  The same bits
    under two AMC_BLOCKS_PER_CU settings, and those of the twin."""
    M = 70001
    out = []
    for bpc in ("1", "3"):
        monkeypatch.setenv("AMC_BLOCKS_PER_CU", bpc)
        eng, tw = make_pair(gpu, M, potential="double_well")
        monkeypatch.delenv("AMC_BLOCKS_PER_CU")
        eng.sweep(1)
        if bpc == "1":
            tw.sweep(1)
            out.append(search(eng, tw, 4.0, 0.9, 2))
        else:
            out.append(eng.anneal_next_beta(4.0, 0.9, 2))
        eng.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert out[0][1][0] == S.OK


def test_nan_positions_and_all_nan(gpu):
    M = 1030
    x = start_x(M)
    x[[5, 300, 1029]] = np.nan
    eng, tw = make_pair(gpu, M, x=x)
    b, diag, trace = search(eng, tw, 3.0, 0.8, 3)
    assert diag[0] == S.OK and 0.5 < b < 3.0
    search(eng, tw, 0.1, 0.8, 3)
    eng.close()
    eng, tw = make_pair(gpu, M, x=np.full(M, np.nan), beta=1.0)
    b, diag, trace = search(eng, tw, 2.0, 0.8, 3)
    assert b == 2.0 and diag[0] == S.ALL_NAN and diag[6] == diag[7] == S.NAN_BITS and not trace.any()
    for o in (eng, tw):
        o.anneal(b)                                                 # records its own status and leaves x alone
    compare(eng, tw)
    assert eng.anneal_records()[0].tolist()[0] == A.ALL_NAN
    eng.close()


def test_infinite_energies(gpu):
    M = 300
    x = start_x(M)
    x[3] = np.inf                                                   # e = +Inf: heating gives it a = +Inf, cooling no weight
    eng, tw = make_pair(gpu, M, x=x, beta=2.0)
    b, diag, _ = search(eng, tw, 1.0, 0.8, 2)
    assert b == 1.0 and diag[0] == S.INF
    b, diag, _ = search(eng, tw, 5.0, 0.8, 2)
    assert diag[0] == S.OK
    eng.close()
    eng, tw = make_pair(gpu, 6, x=np.full(6, np.inf), beta=1.0)
    b, diag, _ = search(eng, tw, 2.0, 0.8, 2)
    assert b == 2.0 and diag[0] == S.NO_WEIGHT
    eng.close()


@pytest.mark.parametrize("where", [0, 2499, 1300])
def test_one_dominant_chain(gpu, where):
    """e = 900 against e = 0: every candidate of every round fails, and the smallest step resolved is taken."""
    M = 2500
    x = np.full(M, 30.0)
    x[where] = 0.0
    eng, tw = make_pair(gpu, M, x=x)
    b, diag, trace = search(eng, tw, 2.0, 0.5, 2)
    assert diag[0] == S.BELOW_RESOLUTION and b == 0.5 + 1.5 / 64.0 and A.bits_f64(diag[3]) == 1.0
    assert np.all(trace[:, :, 0] == 2 ** 30)                        # the one chain's weight and nothing else
    eng.close()


def test_limit_in_one_step_and_an_empty_span(gpu):
    eng, tw = make_pair(gpu, 1025, potential="double_well")
    b, diag, trace = search(eng, tw, 3.0, 1.0e-6, 4)                # a target small enough for the whole span
    assert b == 3.0 and diag[0] == S.LIMIT and diag[1] == 1 and trace[0].all() and not trace[1:].any()
    b, diag, trace = search(eng, tw, 0.5, 0.9, 4)                   # D = 0: nothing is launched
    assert b == 0.5 and diag.tolist() == [S.LIMIT, 0, 0, 0, 0, 0, 0, 0] and not trace.any()
    eng.close()


@pytest.mark.parametrize("dtype,potential", [("f64", "double_well"), ("f32", "harmonic")])
def test_a_whole_adaptive_run(gpu, dtype, potential):
    """[sweep(2); next_beta; anneal] until the limit, on both."""
    eng, tw = make_pair(gpu, 1025, potential=potential, dtype=dtype, families=True)
    steps = 0
    while eng.beta != 2.5:
        for o in (eng, tw):
            o.sweep(2)
        b, diag, _ = search(eng, tw, 2.5, 0.9, 3)
        assert diag[0] in (S.OK, S.LIMIT) and A.bits_f64(diag[3]) >= 0.9
        for o in (eng, tw):
            o.anneal(b)
        steps += 1
        assert steps < 40
    compare(eng, tw)
    assert steps > 2 and A.f64_bits(eng.beta) == A.f64_bits(2.5) and eng.anneal_records()[-1].tolist()[2] == A.f64_bits(2.5)
    eng.close()


def test_refusals_leave_the_handle_as_it_was(gpu):
    kw = dict(potential="harmonic", sigma=[0.5], weight=[1.0], seed=23)
    M = 300
    x = start_x(M)
    with_beta = gpu.HipEngine(n_chains=M, beta=1.0, **kw)
    with_beta.upload_state(x, np.full(M, 1.0))
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*amc_anneal_next_beta.*per-chain beta"):
        with_beta.anneal_next_beta(2.0, 0.5)
    with_beta.set_ladder(3)
    with pytest.raises(gpu.AmcError, match=r"amc error -5.*amc_anneal_next_beta"):
        with_beta.anneal_next_beta(2.0, 0.5)
    with_beta.close()
    for off, glob in [(0, M + 2), (2, M + 2)]:
        part = gpu.HipEngine(n_chains=M, chain_offset=off, n_chains_global=glob, beta=1.0, **kw)
        part.upload_state(x)
        with pytest.raises(gpu.AmcError, match=r"amc error -5.*whole ensemble"):
            part.anneal_next_beta(2.0, 0.5)
        part.close()
    eng, tw = make_pair(gpu, M, beta=1.0)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(gpu.AmcError, match=r"amc error -1.*beta_limit = .* is not finite"):
            eng.anneal_next_beta(bad, 0.5)
    for bad in (0.0, 1.0, -0.5, 1.5, math.nan):
        with pytest.raises(gpu.AmcError, match=r"amc error -1.*target = .* strictly between 0 and 1"):
            eng.anneal_next_beta(2.0, bad)
    for bad in (0, -1, 17):
        with pytest.raises(gpu.AmcError, match=r"amc error -1.*rounds = .* must lie in \[1, 16\]"):
            eng.anneal_next_beta(2.0, 0.5, bad)
    import ctypes as C
    assert gpu.load().amc_anneal_next_beta(eng._h, 2.0, 0.5, 6, None, None, None) == -1
    out = C.c_double(0.0)
    assert gpu.load().amc_anneal_next_beta(eng._h, 2.0, 0.5, 16, C.byref(out), None, None) == 0 and 1.0 < out.value <= 2.0      # diag and trace are optional
    assert eng.beta == 1.0 and eng.anneal_step == 0 and eng.anneal_records().shape == (0, 8)
    # the refused handle still sweeps, searches and anneals, and matches the twin
    for o in (eng, tw):
        o.sweep(2)
    b, _, _ = search(eng, tw, 2.0, 0.7, 16)
    for o in (eng, tw):
        o.anneal(b); o.sweep(1)
    compare(eng, tw)
    eng.close()
