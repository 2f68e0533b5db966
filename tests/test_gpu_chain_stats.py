"""Convergence sums on the device (include/amc.h amc_chain_stats_accumulate .. amc_chain_stats_clear) against
their host twin (tests/chain_stats_twin.py), bit for bit: the downloaded sums per chain AND all 12 words of every fetched record -- no
tolerance anywhere.  The twin is fed its own O(x) (the oracle's potential) of the positions downloaded right behind each sample.
Shapes are the smallest at which a kernel takes another path: one chain, two, a block and its neighbours; a grid of one block per CU (65 536 threads) walked four times with 1, 2 and
3 chains behind the four-in-flight loop; with a ladder odd R, R = 8, R = 64 with two ladders (most blocks hold no chain of most
groups), R = 3 with a ladder count that is no multiple of the ladders per trip.  No lane-cap case, for the reason
test_gpu_rung_sums.py gives: the cap is first reached at 2^28 chains."""
import ctypes as C

import numpy as np
import pytest

from montecarlo_amd.system import CustomPotential

import chain_stats_twin as T

pytestmark = pytest.mark.gpu
CUSTOM = "x*x*x*x - 2.0*x*x + 0.25*x"
LADDER = lambda R: 0.5 * 1.5 ** np.arange(R)
ERR_BAD_ARG, ERR_STATE = -1, -5
PARTS = (0, 0, 0, 1, 1, 0)                # three samples into part 0, two into part 1, one more into part 0
GRID1 = 65536                             # threads of a grid of one block per CU


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def start_state(M, R=0, offset=0):
    ids = np.arange(offset, offset + M)
    x = 1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids)
    return x, (LADDER(R)[ids % R] if R else None)


def make(gpu, M, R=0, *, potential="double_well", dtype="f64", offset=0, n_global=None, seed=23, env=None, **kw):
    mp = pytest.MonkeyPatch()
    for k, v in (env or {}).items():
        mp.setenv(k, v)
    try:
        eng = gpu.HipEngine(n_chains=M, chain_offset=offset, n_chains_global=n_global or offset + M, potential=potential, beta=1.0,
                            sigma=[0.5], weight=[1.0], seed=seed, dtype=dtype, **kw)
    finally:
        mp.undo()
    x, beta = start_state(M, R, offset)
    eng.upload_state(x, beta)
    if R:
        eng.set_ladder(R)
    eng.twin_model = (potential, dtype == "f32")
    return eng


def observe(eng, kind):
    """O(x) of every chain by the TWIN's potential (the oracle's, corr_twin.observable) from the downloaded positions: nothing of the
    engine's own evaluation of the potential or of its widening enters the reference."""
    potential, f32 = getattr(eng, "twin_model", ("double_well", False))
    return T.CT.observable(kind, potential, eng.download_state(want_e=False)[0], f32)


def same(eng, twin, what=""):
    """The engine's sums and records against the twin's; returns the records."""
    sums = eng.chain_stats_sums()
    if not np.array_equal(bits(sums), bits(twin.sums)):
        p, k, i = (int(v) for v in np.argwhere(bits(sums) != bits(twin.sums))[0])
        raise AssertionError(f"{what}: sums differ from the twin, first at part {p} {'SQ'[k]} chain {i}: {sums[p, k, i]!r} != {twin.sums[p, k, i]!r}")
    rec, n, obs = eng.chain_stats_fetch()
    want = twin.records()
    assert rec.shape == want.shape and n == tuple(twin.n) and obs == twin.observable, (what, rec.shape, n, obs)
    if not np.array_equal(bits(rec), bits(want)):
        g, c = (int(v) for v in np.argwhere(bits(rec) != bits(want))[0][:2])
        raise AssertionError(f"{what}: records differ from the twin, first at group {g} column {c}: {rec[g, c].tolist()} != {want[g, c].tolist()}")
    return rec


def sequence(eng, kind, R, parts=PARTS):
    """A sample per entry of ``parts`` with sweeps (and an exchange step) between them; the twin fed behind each."""
    twin = T.ChainStatsTwin(eng.n_chains, max(R, 1))
    for s, p in enumerate(parts):
        if s:
            eng.sweep(2)
            if R and s % 2:
                eng.exchange(1)
        eng.chain_stats_accumulate(kind, p)
        twin.accumulate(kind, observe(eng, kind), p)
    return twin


def check_sequence(eng, kind, R, what, parts=PARTS):
    twin = sequence(eng, kind, R, parts)
    rec = same(eng, twin, what)
    again = eng.chain_stats_fetch()
    assert np.array_equal(bits(again[0]), bits(rec)) and again[1] == tuple(twin.n)            # a fetch changes nothing
    assert np.array_equal(bits(eng.chain_stats_sums()), bits(twin.sums))
    return rec


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["energy", "x"])
@pytest.mark.parametrize("M", [1, 2, 255, 257])
def test_shapes_without_a_ladder(gpu, M, kind):
    eng = make(gpu, M)
    check_sequence(eng, kind, 0, f"M={M} {kind}")
    eng.close()


@pytest.mark.parametrize("kind", ["energy", "x"])
@pytest.mark.parametrize("R,L", [(3, 22), (8, 33), (64, 5), (64, 2)])
def test_shapes_with_a_ladder(gpu, R, L, kind):
    eng = make(gpu, R * L, R)
    check_sequence(eng, kind, R, f"R={R} L={L} {kind}")
    eng.close()


@pytest.mark.parametrize("M,R", [(4 * GRID1 + 7, 0), (5 * GRID1 + 7, 0), (6 * GRID1 + 7, 0), (3 * 100003, 3)])
def test_grid_stride_and_tails(gpu, M, R):
    """One block per CU: 4 x 65 536 + 7 chains leave the first lanes one chain behind the four-in-flight loop and the others none;
    one and two grids more leave 2 | 1 and 3 | 2.  R = 3: a trip is 21 845 ladders, 100 003 ladders are four trips and a ragged fifth,
    and the last thread of the grid holds no chain."""
    eng = make(gpu, M, R, env={"AMC_BLOCKS_PER_CU": "1"})
    check_sequence(eng, "x", R, f"M={M} R={R}", parts=(0, 1, 1))
    eng.close()


def test_two_grids_give_the_same_bits(gpu):
    M, out = 300011, []
    for env in ({"AMC_BLOCKS_PER_CU": "1"}, {}):
        eng = make(gpu, M, env=env)
        rec = check_sequence(eng, "x", 0, f"env={env}", parts=(0, 1))
        out.append((rec, eng.chain_stats_sums()))
        eng.close()
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))


# ---- 2. potentials and state types ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["energy", "x"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("potential", ["harmonic", "double_well", "custom"])
def test_potentials_and_state_types(gpu, potential, dtype, kind):
    pot = CustomPotential(CUSTOM) if potential == "custom" else potential
    for R, L in ((0, 257), (5, 103)):
        eng = make(gpu, L * max(R, 1), R, potential=pot, dtype=dtype)
        check_sequence(eng, kind, R, f"{potential} {dtype} R={R} {kind}")
        eng.close()


# ---- 3. flags ---------------------------------------------------------------------------------------------------------------------------
def test_flags_touch_their_own_columns_only(gpu):
    """A NaN sampled into part 0 of a chain of group 0 flags S0, S0S0, Q0 and S0S1 of that group; an Inf sampled into part 1 of a chain
    of group 1 flags S1, S1S1, Q1 and S0S1 of that group; groups 2 and 3 stay finite."""
    R, L = 4, 40
    x, beta = start_state(R * L, R)
    eng = gpu.HipEngine(n_chains=R * L, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=5)
    eng.twin_model = ("harmonic", False)
    twin = T.ChainStatsTwin(R * L, R)
    a = x.copy().reshape(L, R)
    a[3, 0] = np.nan
    eng.upload_state(a.reshape(-1), beta)
    eng.set_ladder(R)
    eng.chain_stats_accumulate("x", 0)
    twin.accumulate("x", observe(eng, "x"), 0)
    kept = eng.chain_stats_sums()
    b = x.copy().reshape(L, R)
    b[5, 1] = np.inf
    eng.upload_state(b.reshape(-1), beta)               # (through the checkpoint route: an upload clears the sums)
    eng.set_ladder(R)
    eng.set_chain_stats("x", (1, 0), kept)
    eng.chain_stats_accumulate("x", 1)
    twin.accumulate("x", observe(eng, "x"), 1)
    val = T.values(same(eng, twin, "flags"))
    nonfinite = ~np.isfinite(val)
    assert nonfinite[0].tolist() == [True, True, True, False, False, False, True]
    assert nonfinite[1].tolist() == [False, False, False, True, True, True, True]
    assert not nonfinite[2:].any()
    eng.close()


# ---- 4. shards --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 6])
def test_shard_invariance(gpu, R):
    M = 660
    whole = make(gpu, M, R)
    rec_w = check_sequence(whole, "energy", R, "whole")
    sums_w = whole.chain_stats_sums()
    whole.close()
    for split in ([0, 402, M], [0, 6, M]):
        merged, sums = None, []
        for a, b in zip(split, split[1:]):
            part = make(gpu, b - a, R, offset=a, n_global=M)
            sequence(part, "energy", R)
            rec = part.chain_stats_fetch()[0].reshape(-1, 12)
            merged = rec if merged is None else gpu.xsum_merge(merged, rec)
            sums.append(part.chain_stats_sums())
            part.close()
        assert np.array_equal(bits(merged), bits(rec_w.reshape(-1, 12))), (R, split)
        assert np.array_equal(bits(np.concatenate(sums, axis=2)), bits(sums_w)), (R, split)


# ---- 5. a random walk over the entries against the twin -------------------------------------------------------------------------------
WALK_OPS = ("sweep", "exchange", "acc", "fetch", "move", "clear", "ladder")
# every operation once in an order that means something -- sums held when the ladder changes, a move behind that change (the fresh
# handle takes betas of period 4 under a ladder of 2 rungs), a clear with sums held -- then draws with a fixed seed up to 40 operations
WALK_HEAD = ("acc", "sweep", "exchange", "acc", "fetch", "move", "acc", "ladder", "acc", "sweep", "acc", "move", "exchange", "acc", "clear",
             "acc", "ladder", "acc")


def test_random_walk_against_the_twin(gpu):
    """40 operations over {sweep, exchange, accumulate(p), fetch, download -> set on a fresh handle, clear, set_ladder}, the sums and
    the records compared with the twin behind EVERY one.  Only operations that apply are drawn (a move needs sums to move), so every
    one of the 40 runs; the walk asserts at its end that it held sums at a ladder change and moved behind one."""
    rng = np.random.default_rng(20241)
    R, L = 4, 37
    M = R * L
    eng = make(gpu, M, R)
    twin, G, done, held_at_ladder, moved_under = None, R, [], 0, set()
    for step in range(40):
        if step < len(WALK_HEAD):
            op = WALK_HEAD[step]
        else:
            op = str(rng.choice([o for o in WALK_OPS if o != "move" or twin is not None]))
        assert op != "move" or twin is not None
        done.append(op)
        if op == "sweep":
            eng.sweep(int(rng.integers(1, 4)))
        elif op == "exchange":
            eng.exchange(1)
        elif op == "acc":
            p = int(rng.integers(0, 2))
            eng.chain_stats_accumulate("energy", p)
            twin = twin or T.ChainStatsTwin(M, G)
            twin.accumulate("energy", observe(eng, "energy"), p)
        elif op == "fetch":
            eng.chain_stats_fetch()                     # (compared below, like everything else: a fetch changes nothing)
        elif op == "move":                              # download -> set on a fresh handle, which goes on from the same state
            sums, n = eng.chain_stats_sums(), eng.chain_stats_fetch()[1]
            x, t, tx = eng.download_state(want_e=False)[0], eng.step, eng.exchange_step
            eng.close()
            eng = gpu.HipEngine(n_chains=M, potential="double_well", beta=1.0, sigma=[0.5], weight=[1.0], seed=23)
            eng.upload_state(x, LADDER(R)[np.arange(M) % R])
            eng.set_ladder(G)
            eng.exchange_step = tx
            eng.step = t
            eng.set_chain_stats("energy", n, sums)
            moved_under.add(G)
        elif op == "clear":
            eng.chain_stats_clear()
            twin = None
        elif op == "ladder":
            held_at_ladder += twin is not None
            G = 2 if G == 4 else 4
            eng.set_ladder(G)
            twin = None
        if twin is None:
            rec, n, obs = eng.chain_stats_fetch()
            assert rec.shape == (G, 0, 12) and n == (0, 0) and obs == 0, (step, op)
        else:
            same(eng, twin, f"step {step} {op}")
    eng.close()
    assert len(done) == 40 and set(done) == set(WALK_OPS), sorted(set(WALK_OPS) - set(done))
    assert held_at_ladder >= 2 and moved_under == {2, 4}, (held_at_ladder, moved_under)


# ---- 6. refusals, lifetimes, no disturbance ---------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu):
    eng = make(gpu, 4 * 50, 4)
    lib, h = eng._lib, eng._h
    twin = sequence(eng, "energy", 4, parts=(0, 1))
    n, g, obs = (C.c_uint64 * 2)(), C.c_int(0), C.c_int(0)
    small = np.zeros(4 * 7 * 12 - 1)
    dp = small.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.amc_chain_stats_accumulate(h, 2, 0) == ERR_STATE and b"observable" in lib.amc_last_error()
    assert lib.amc_chain_stats_accumulate(h, 3, 0) == ERR_BAD_ARG and lib.amc_chain_stats_accumulate(h, 0, 0) == ERR_BAD_ARG
    assert lib.amc_chain_stats_accumulate(h, 1, 2) == ERR_BAD_ARG and lib.amc_chain_stats_accumulate(h, 1, -1) == ERR_BAD_ARG
    assert lib.amc_chain_stats_fetch(h, dp, small.size, n, C.byref(g), C.byref(obs)) == ERR_BAD_ARG and b"capacity" in lib.amc_last_error()
    assert lib.amc_chain_stats_fetch(h, dp, small.size, None, C.byref(g), C.byref(obs)) == ERR_BAD_ARG
    assert lib.amc_chain_stats_download(h, None) == ERR_BAD_ARG
    # (n = {0, 0} would clear: the sizes fill it first)
    assert lib.amc_chain_stats_fetch(h, None, 0, n, C.byref(g), C.byref(obs)) == 0 and (n[0], n[1], g.value, obs.value) == (1, 1, 4, 1)
    assert lib.amc_set_chain_stats(h, 7, n, dp) == ERR_BAD_ARG and b"observable" in lib.amc_last_error()
    same(eng, twin, "behind the refusals")
    eng.chain_stats_clear()
    assert lib.amc_chain_stats_download(h, dp) == ERR_STATE
    eng.chain_stats_accumulate("x", 1)                  # another observable after a clear
    assert eng.chain_stats_fetch()[1:] == ((0, 1), 2) and eng.chain_stats_counts() == ((0, 1), 2)
    eng.close()


def test_what_clears_the_sums_and_what_keeps_them(gpu):
    R, L = 3, 22
    x, beta = start_state(R * L, R)
    eng = make(gpu, R * L, R, per_chain_counters=True)
    twin = sequence(eng, "energy", R, parts=(0,))
    eng.sweep(1); eng.exchange(1); eng.reduce(); eng.reduce_rungs(); eng.bridge_accumulate(3); eng.corr_mark("x"); eng.corr_sample()
    eng.energy_histogram_accumulate(0.0, 2.0, 10); eng.set_blocks(2, 1)
    same(eng, twin, "kept")
    eng.respace_ladder("acceptance", 1.0, 0.01)         # kept ON PURPOSE: the caller clears when beta moves
    same(eng, twin, "behind a respacing")
    eng.set_ladder(R)
    assert eng.chain_stats_fetch()[2] == 0
    eng.chain_stats_accumulate("x", 0)
    eng.upload_state(x, beta)
    assert eng.chain_stats_fetch()[2] == 0
    eng.chain_stats_accumulate("x", 0)
    eng.init_uniform(-1.0, 1.0)
    assert eng.chain_stats_fetch()[2] == 0
    eng.close()
    flat = make(gpu, 130)
    twin = sequence(flat, "energy", 0, parts=(0, 1))
    flat.anneal(1.25)
    flat.beta = 1.5
    same(flat, twin, "behind anneal and set_beta")
    flat.close()


def snapshot_of_everything(eng):
    x, e = eng.download_state()
    acc, tot = eng.counter_totals()
    out = dict(x=x.copy(), e=e.copy(), acc=np.array(acc), tot=np.array(tot), step=eng.step, est=eng.estimator_step)
    if eng.n_rungs:
        out.update(xstep=eng.exchange_step, gaps=np.concatenate([np.ravel(v) for v in eng.exchange_counters()]),
                   bridge=eng.bridge_fetch()[0], corr=eng.corr_fetch()[0])
    return out


@pytest.mark.parametrize("R", [0, 4])
def test_a_handle_that_accumulates_ends_as_one_that_never_did(gpu, R):
    a, b = make(gpu, 4 * 129, R), make(gpu, 4 * 129, R)
    for i in range(3):
        for eng in (a, b):
            eng.sweep(3)
            if R:
                eng.exchange(1)
                eng.bridge_accumulate(3)
                eng.corr_mark("x") if i == 0 else eng.corr_sample()
        a.chain_stats_accumulate("energy", i % 2)
    a.chain_stats_fetch()
    for eng in (a, b):
        eng.sweep(2)
    sa, sb = snapshot_of_everything(a), snapshot_of_everything(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.asarray(sa[k]).tobytes() == np.asarray(sb[k]).tobytes(), k
    a.close()
    b.close()


def test_the_buffers_are_allocated_at_the_first_sample(gpu):
    """hipMemGetInfo around the first sample and the first fetch of a handle that has swept: the 32 bytes per chain appear at the first
    amc_chain_stats_accumulate, not at amc_create, and a clear followed by another first sample allocates nothing more -- a handle
    that never calls these entries never pays for them.  (Free memory of the whole device: another process allocating meanwhile only
    widens the first drop.)"""
    hip = C.CDLL(gpu.runtime_info()["hip_runtime"])
    free, total = C.c_size_t(0), C.c_size_t(0)

    def free_bytes():
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    M = 1 << 22
    eng = gpu.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=3, per_chain_counters=False)
    eng.init_uniform(-2.0, 2.0)
    eng.sweep(2); eng.reduce(); eng.sync()
    assert eng.chain_stats_fetch()[2] == 0              # asking allocates nothing either
    before = free_bytes()
    eng.chain_stats_accumulate("x", 0); eng.sync()
    after = free_bytes()
    print(f"free before the first sample {before}, after {after}: {before - after} bytes")
    assert before - after >= 32 * M
    eng.chain_stats_clear()
    eng.chain_stats_accumulate("energy", 1); eng.sync()
    # the memory is kept and zeroed: a second buffer would take 32 M bytes more.  (Whole-device figures again: only another
    # process taking that much between the two reads could be mistaken for it, and the handle's own state is checked beside it.)
    assert after - free_bytes() < 32 * M
    assert eng.chain_stats_sums()[0].tobytes() == bytes(16 * M)      # part 0 of the kept buffer was zeroed by the new first sample
    assert eng.chain_stats_fetch()[1] == (0, 1)
    eng.close()
