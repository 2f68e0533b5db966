"""The ladder respacing rule (DESIGN.md section 3.13 "Respacing") on its host twin (tests/respace_twin.py): cases worked by hand, every
status, the ends, damping and floor, R = 2, Float32 state, a property test, the rule run on the CPU by the product's own inline
function (tests/aux/respace_rule_host.cpp, under the address and undefined-behaviour sanitizers), the argument checks of the C ABI
that need no device, and the rule doing its job over a run of the twin.  The device side is tests/test_gpu_respace.py: the device is
bit-equal to this twin."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import respace_twin as RT

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "montecarlo_amd", "csrc")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def flow_counts(f_up, total=8):
    """n[R][3] with f(r) = f_up[r] exactly: `total` labels per rung that have visited an end, none that has not."""
    n = np.zeros((len(f_up), 3), dtype=np.int64)
    for r, f in enumerate(f_up):
        up = f * total
        assert up == int(up)
        n[r] = [0, int(up), total - int(up)]
    return n


# ---- worked by hand (every intermediate is a dyadic rational: the arithmetic is exact) --------------------------------------------
def test_acceptance_three_rungs_by_hand():
    # w = [2/4, 1/4] = [0.5, 0.25], W = 0.75, G = [0, 0.5, 0.75]; k = 1: t = 0.375 < G[1]: j = 0, frac = 0.375 / 0.5 = 0.75,
    # nb = 1 + (2 - 1) 0.75 = 1.75: the gap that rejects more gets narrower
    st, out = RT.respace_rule("acceptance", [1.0, 2.0, 4.0], ([4, 4], [2, 3]))
    assert st == 0 and out.tolist() == [1.0, 1.75, 4.0]
    # equal rejection: t = 0.25 is not below G[1] = 0.25: j = 1, frac = 0: nb = b[1]
    st, out = RT.respace_rule("acceptance", [1.0, 2.0, 4.0], ([4, 4], [3, 3]))
    assert st == 0 and out.tolist() == [1.0, 2.0, 4.0]


def test_acceptance_four_rungs_by_hand():
    # w = [1, 0.25, 0.25], W = 1.5, G = [0, 1, 1.25, 1.5]; k = 1: t = 0.5, j = 0, frac = 0.5, nb = 0.5 + 0.5 0.5 = 0.75;
    # k = 2: t = 1.0, G[1] = 1 is not above it, G[2] = 1.25 is: j = 1, frac = 0, nb = b[1] = 1
    st, out = RT.respace_rule("acceptance", [0.5, 1.0, 2.0, 4.0], ([4, 4, 4], [0, 3, 3]))
    assert st == 0 and out.tolist() == [0.5, 0.75, 1.0, 4.0]
    # a falling ladder, the weight in the last gap: w = [0.25, 0.25, 1], G = [0, 0.25, 0.5, 1.5]; k = 1: t = 0.5, only G[3] is above
    # it: j = 2, frac = 0, nb = b[2] = 1; k = 2: t = 1, j = 2, frac = 0.5, nb = 1 + (0.5 - 1) 0.5 = 0.75
    st, out = RT.respace_rule("acceptance", [4.0, 2.0, 1.0, 0.5], ([4, 4, 4], [3, 3, 0]))
    assert st == 0 and out.tolist() == [4.0, 1.0, 0.75, 0.5]


def test_flow_three_rungs_by_hand():
    # f = [1, 1, 0]: d = [0, 1], w = [0, 1], W = 1, G = [0, 0, 1]; t = 0.5: j = 1, frac = 0.5, nb = 2 + 2 0.5 = 3: the whole drop of f
    # lies in gap 1, so rung 1 moves into it
    n = [[0, 5, 0], [1, 4, 0], [0, 0, 5]]
    st, out = RT.respace_rule("flow", [1.0, 2.0, 4.0], n)
    assert st == 0 and out.tolist() == [1.0, 3.0, 4.0]
    # f = [1, 0.5, 0]: equal drops, sqrt(0.5) twice: t = W / 2 = G[1] exactly, j = 1, frac = 0
    st, out = RT.respace_rule("flow", [1.0, 2.0, 4.0], flow_counts([1.0, 0.5, 0.0]))
    assert st == 0 and out.tolist() == [1.0, 2.0, 4.0]


def test_flow_four_rungs_by_hand():
    # f = [1, 0, 0.25, 0]: d = [1, -0.25 -> 0, 0.25], w = [1, 0, 0.5], W = 1.5, G = [0, 1, 1, 1.5]; k = 1: t = 0.5, j = 0, frac = 0.5,
    # nb = 0.75; k = 2: t = 1, neither G[1] nor G[2] is above it, G[3] is: j = 2, frac = 0, nb = b[2]
    st, out = RT.respace_rule("flow", [0.5, 1.0, 2.0, 4.0], flow_counts([1.0, 0.0, 0.25, 0.0]))
    assert st == 0 and out.tolist() == [0.5, 0.75, 2.0, 4.0]


# ---- every non-zero status ------------------------------------------------------------------------------------------------------------
def test_status_2_no_counts():
    assert RT.respace_rule("acceptance", [1.0, 2.0, 4.0], ([0, 0], [0, 0]))[0] == 2
    assert RT.respace_rule("acceptance", [1.0, 2.0, 4.0], ([4, 0], [1, 0])) == (2, None)
    n = RT.T.flow_counts(RT.T.initial_labels(12, 4), 4)          # straight after set_tracking(True): the interior has no direction
    assert RT.respace_rule("flow", [0.5, 1.0, 2.0, 4.0], n) == (2, None)


def test_status_1_no_weight():
    assert RT.respace_rule("flow", [1.0, 2.0, 4.0], flow_counts([0.5, 0.5, 0.5])) == (1, None)      # equal flow everywhere: W = 0
    assert RT.respace_rule("acceptance", [1.0, 2.0, 4.0], ([4, 4], [4, 4])) == (1, None)            # nothing was ever rejected


@pytest.mark.parametrize("b", [[1.0, 4.0, 2.0], [1.0, 1.0, 2.0], [1.0, np.inf, 2.0], [np.nan, 1.0, 2.0], [4.0, 2.0, 3.0]])
def test_status_3_bad_ladder(b):
    assert RT.respace_rule("acceptance", b, ([4, 4], [2, 3])) == (3, None)


def test_status_4_collapse():
    # three neighbouring Float64s above 1 and all the weight in the last gap: both interior targets lie in (b[2], b[3]), a third and
    # two thirds of an ulp above b[2], and round to b[2] and to b[3]: out[2] == out[3]
    b = 1.0 + np.arange(4) * 2.0 ** -52
    assert RT.respace_rule("acceptance", b, ([4, 4, 4], [4, 4, 0])) == (4, None)
    assert RT.respace_rule("acceptance", b[::-1].copy(), ([4, 4, 4], [0, 4, 4])) == (4, None)


# ---- ends, damping, floor, R = 2, Float32 ------------------------------------------------------------------------------------------
def test_the_ends_keep_their_bits():
    b = np.array([0.1, 0.30000000000000004, 0.7, 1.9000000000000001, 5.1])
    st, out = RT.respace_rule("acceptance", b, ([97, 101, 89, 103], [11, 60, 33, 80]), gamma=0.7, eps=0.05)
    assert st == 0 and bits(out)[0] == bits(b)[0] and bits(out)[-1] == bits(b)[-1]
    assert not np.array_equal(out[1:-1], b[1:-1])


def test_gamma_halves_the_move():
    n = [[0, 5, 0], [1, 4, 0], [0, 0, 5]]
    assert RT.respace_rule("flow", [1.0, 2.0, 4.0], n, gamma=0.5)[1].tolist() == [1.0, 2.5, 4.0]
    assert RT.respace_rule("acceptance", [1.0, 2.0, 4.0], ([4, 4], [2, 3]), gamma=0.5)[1].tolist() == [1.0, 1.875, 4.0]


def test_eps_lifts_a_zero_weight():
    # w = [0, 1], eps = 0.5: m = 0.5 1 / 2 = 0.25, wf = [0.25, 1], G = [0, 0.25, 1.25]; t = 0.625, j = 1, frac = 0.375, nb = 2.75 (3 without)
    n = [[0, 5, 0], [1, 4, 0], [0, 0, 5]]
    assert RT.respace_rule("flow", [1.0, 2.0, 4.0], n, eps=0.5)[1].tolist() == [1.0, 2.75, 4.0]


def test_two_rungs():
    b = np.array([0.30000000000000004, 1.7])
    for rule, counts in (("acceptance", ([5], [2])), ("flow", [[0, 3, 0], [0, 0, 3]])):
        st, out = RT.respace_rule(rule, b, counts, gamma=0.3, eps=0.2)
        assert st == 0 and np.array_equal(bits(out), bits(b))
    assert RT.respace_rule("acceptance", b, ([0], [0]))[0] == 2 and RT.respace_rule("acceptance", b, ([5], [5]))[0] == 1


def make_twin(R, L, betas, *, dtype="f64", seed=5, potential="harmonic", track=False, x=None):
    M = R * L
    beta = np.tile(np.asarray(betas, dtype=np.float64), L)
    sim = O.OracleSim(M, potential=potential, beta=1.0, sigma=[0.5], weight=[1.0], seed=seed, dtype=dtype)
    sim.set_beta(beta)
    tw = RT.RespaceTwin(sim, beta, R, seed=seed, potential=potential, f32=dtype == "f32")
    if x is None:
        x = 1.6 * np.sin(0.731 * np.arange(M) + 0.2)
    tw.state.put(x.astype(np.float32).astype(np.float64) if dtype == "f32" else x, tw.pot)
    if track:
        tw.set_tracking(True)
    return tw


def test_float32_ladder_is_rounded_once():
    """The rule runs in Float64 on double(beta_r); the new ladder is rounded to Float32 when it is stored and nowhere before."""
    b = np.array([0.3, 0.7, 1.1, 4.9])
    tw = make_twin(4, 6, b, dtype="f32", track=True)
    b32 = b.astype(np.float32).astype(np.float64)
    assert np.array_equal(tw.ladder(), b32)
    tw.sweep_exchange(16, 1)
    counts = (tw.attempted.copy(), tw.accepted.copy())
    st, out = RT.respace_rule("acceptance", b32, counts, 0.9, 0.01)
    assert st == 0 and tw.respace("acceptance", 0.9, 0.01) == 0
    assert not np.array_equal(out, out.astype(np.float32).astype(np.float64))          # (the Float64 result is no Float32 value)
    assert np.array_equal(tw.ladder(), out.astype(np.float32).astype(np.float64))
    assert np.array_equal(tw.beta, np.tile(tw.ladder(), 6)) and tw.n_respaced == 1
    assert tw.attempted.sum() == 0 and tw.accepted.sum() == 0 and (tw.round_trips, tw.up_trips) == (0, 0)
    assert np.array_equal(tw.lab, RT.T.initial_labels(24, 4))


def test_a_refused_respacing_changes_nothing():
    tw = make_twin(4, 6, [0.3, 0.7, 1.1, 4.9], track=True)
    tw.sweep_exchange(9, 1)
    before = (tw.beta.copy(), tw.attempted.copy(), tw.accepted.copy(), tw.lab.copy(), tw.round_trips, tw.up_trips)
    tw.lab[1::4] &= 63          # a rung without a direction
    lab = tw.lab.copy()
    assert tw.respace("flow") == 2 and tw.n_respaced == 0
    assert np.array_equal(tw.beta, before[0]) and np.array_equal(tw.attempted, before[1]) and np.array_equal(tw.accepted, before[2])
    assert np.array_equal(tw.lab, lab) and (tw.round_trips, tw.up_trips) == before[4:]


# ---- property test ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["acceptance", "flow"])
def test_status_0_outputs_are_ladders(rule):
    rng = np.random.default_rng(2024)
    seen = {0: 0, 1: 0, 2: 0, 3: 0, 4: 0}
    for trial in range(600):
        R = int(rng.integers(2, 65)) if trial % 3 else int(rng.integers(2, 6))
        b = np.cumsum(rng.uniform(1e-3, 1.0, R) * 10.0 ** rng.integers(-3, 3)) + rng.uniform(-5, 5)
        if rng.random() < 0.5:
            b = b[::-1].copy()
        if rule == "acceptance":
            att = rng.integers(0 if trial % 50 == 0 else 1, 1000, R - 1)
            acc = (att * rng.choice([0.0, 0.5, 1.0, rng.random()], R - 1)).astype(np.int64)
            counts = (att, acc)
        else:
            counts = rng.integers(0 if trial % 50 == 0 else 1, 50, (R, 3))
            if trial % 7 == 0:
                counts[:, 1] = np.sort(counts[:, 1])[::-1]
        gamma, eps = rng.choice([1.0, 0.5, rng.uniform(0.01, 1.0)]), rng.choice([0.0, 0.01, rng.uniform(0.0, 0.99)])
        st, out = RT.respace_rule(rule, b, counts, gamma, eps)
        seen[st] += 1
        if st != 0:
            assert out is None
            continue
        assert np.all(np.isfinite(out)) and out.min() >= b.min() and out.max() <= b.max()
        d = np.diff(out)
        assert np.all(d > 0) if b[1] > b[0] else np.all(d < 0)
        assert bits(out)[0] == bits(b)[0] and bits(out)[-1] == bits(b)[-1]
    assert seen[0] > 300 and seen[3] == 0, seen


# ---- the product's own rule on the CPU, under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_host(tmp_path_factory):
    """run(rule, b, counts, gamma, eps) -> (status, out) of tests/aux/respace_rule_host.cpp, which calls amc_respace.h's respace_rule;
    built once, with -fsanitize=address,undefined: a stand-alone program, nothing is loaded into this process."""
    d = tmp_path_factory.mktemp("respace_rule")
    exe = str(d / "respace_rule_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "aux", "respace_rule_host.cpp"), "-o", exe], check=True, capture_output=True)

    def run(rule, b, counts, gamma=1.0, eps=0.0):
        b = np.asarray(b, dtype=np.float64)
        flat = np.concatenate([np.asarray(c, dtype=np.int64).reshape(-1) for c in counts]) if rule == "acceptance" else np.asarray(counts).reshape(-1)
        args = [exe, {"acceptance": "1", "flow": "2"}[rule], float(gamma).hex(), float(eps).hex()] + [float(v).hex() for v in b] + [str(int(c)) for c in flat]
        r = subprocess.run(args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        words = r.stdout.split()
        return int(words[0]), np.array([float.fromhex(w) for w in words[1:]])
    return run


def test_the_inline_rule_equals_the_twin_on_the_cpu(rule_host):
    rng = np.random.default_rng(77)
    cases = [("acceptance", [1.0, 2.0, 4.0], ([4, 4], [2, 3]), 1.0, 0.0),
             ("acceptance", [0.5, 1.0, 2.0, 4.0], ([4, 4, 4], [0, 3, 3]), 1.0, 0.0),
             ("flow", [1.0, 2.0, 4.0], [[0, 5, 0], [1, 4, 0], [0, 0, 5]], 0.5, 0.5),
             ("flow", [0.5, 1.0, 2.0, 4.0], flow_counts([1.0, 0.0, 0.25, 0.0]), 1.0, 0.0),
             ("acceptance", [1.0, 2.0, 4.0], ([4, 0], [1, 0]), 1.0, 0.0),
             ("flow", [1.0, 2.0, 4.0], flow_counts([0.5, 0.5, 0.5]), 1.0, 0.0),
             ("acceptance", [1.0, 4.0, 2.0], ([4, 4], [2, 3]), 1.0, 0.0),
             ("acceptance", 1.0 + np.arange(4) * 2.0 ** -52, ([4, 4, 4], [4, 4, 0]), 1.0, 0.0),
             ("acceptance", [0.3, 1.7], ([5], [2]), 0.3, 0.2)]
    for R in (2, 3, 7, 33, 64):
        for _ in range(3):
            b = np.cumsum(rng.uniform(0.01, 1.0, R))
            att = rng.integers(1, 5000, R - 1)
            cases.append(("acceptance", b, (att, (att * rng.random(R - 1)).astype(np.int64)), rng.uniform(0.1, 1.0), 0.01))
            cases.append(("flow", b[::-1].copy(), rng.integers(1, 90, (R, 3)), rng.uniform(0.1, 1.0), 0.01))
    statuses = set()
    for rule, b, counts, gamma, eps in cases:
        st, out = RT.respace_rule(rule, b, counts, gamma, eps)
        st_c, out_c = rule_host(rule, b, counts, gamma, eps)
        statuses.add(st)
        assert st_c == st, (rule, b, counts)
        if st == 0:
            assert np.array_equal(bits(out_c), bits(out)), (rule, b, counts, out, out_c)
    assert statuses == {0, 1, 2, 3, 4}


# ---- the C ABI's argument checks that come before any device --------------------------------------------------------------------------
def test_null_handles_are_refused(amc):
    lib = amc.load()
    assert lib.amc_respace_ladder(None, 1, 1.0, 0.0, None) == -1 and b"amc_respace_ladder" in lib.amc_last_error()
    assert lib.amc_respace_status(None, None, None) == -1 and lib.amc_get_ladder(None, None) == -1 and lib.amc_set_respaced(None, 0) == -1


# ---- the rule does its job ---------------------------------------------------------------------------------------------------------------
UNEVEN = [0.25, 0.3, 0.36, 0.45, 4.0, 4.6, 5.3, 6.0]


def test_respacing_evens_out_the_rejection_rate():
    """Harmonic potential, R = 8, 512 ladders, the uneven ladder above (three narrow gaps at either end, one gap of a factor 9 in
    between); four blocks of [200 x (1 sweep, 1 exchange); respace("acceptance", gamma = 1, eps = 0.01)].  The spread max - min of the
    per-gap rejection rate over a block, measured on the twin (the device is bit-equal to it):
        0.53627, 0.18969, 0.03717, 0.00461 in the four blocks: first 0.53627, last 0.00461
    -- a factor 116 (the ladder ends close to the geometric one, 0.25 x 1.575^r, which is the even one for this potential); asserted
    with half that margin, a factor 58."""
    R, L = 8, 512
    ids = np.arange(R * L)
    tw = make_twin(R, L, UNEVEN, seed=31, x=1.6 * np.sin(0.731 * ids + 0.2) + 0.3 * np.cos(0.0173 * ids))
    spreads = []
    for block in range(4):
        tw.sweep_exchange(200, 1)
        rej = (tw.attempted - tw.accepted) / tw.attempted
        spreads.append(float(rej.max() - rej.min()))
        assert tw.respace("acceptance", 1.0, 0.01) == 0
    first, last = spreads[0], spreads[-1]
    print("rejection-rate spread per block:", spreads, "ladder:", tw.ladder().tolist())
    assert tw.n_respaced == 4 and last < first
    assert 58.0 * last < first
