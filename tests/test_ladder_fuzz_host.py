"""The random ladder walks (tests/ladder_fuzz.py) on the host: that the cases are well formed and repeat, that the default case list
meets the combinations it is there for, and that the walk notices a reference with one deliberate defect -- the evidence that
tests/test_gpu_ladder_fuzz.py would notice the same kinds of error in a kernel, or in the host code that decides what a call resets
and what it leaves alone.  No GPU: both sides of the walk are reference objects."""
import collections

import numpy as np
import pytest

import exchange_twin as X
import ladder_fuzz as LF
import respace_twin as RP
import track_twin as T

N_CASES, SEED = LF.DEFAULT_CASES, LF.DEFAULT_SEED       # the list tests/test_gpu_ladder_fuzz.py walks on the device by default
EVENTS = [
    "table, tracking and exchange on one handle",
    "a table cleared, then set_parameters, then a sweep",
    "set_ladder to another R, then exchange steps",
    "exchange step index >= 2^32 with swaps attempted",
    "chain ids cross 2^32 inside the shard",
    "equal beta with tracking: a round trip and an up trip",
    "non-finite positions",
    "sliced route with a ladder, at least 2 slices",
    "exchange steps between sliced calls",
    "double well on the sliced route",
    "Float32 state on a handle with the slice knobs",
    "Float32 parameters with tracking",
    "counts cross 65 536 after an upload while a table is set",
    # the ladder tools: bridge sums, respacing, tuning and its window, time correlation, jackknife blocks
    "respacing taken with snapshots accumulated",
    "respacing not taken (status != 0) with snapshots accumulated",
    "respacing taken under a partition",
    "respacing with a mark standing, then a sample",
    "tuning with an inconsistent window",
    "tuning that clamps",
    "table rewritten between two tunings",
    "explicit counts on a shard that does not start at 0",
    "upload with a mark standing",
    "set_blocks with snapshots accumulated",
    "partition on a shard across 2^32",
    "Float32 ladder respaced",
]


@pytest.fixture(scope="module")
def default_walks(oracle):
    """The default case list walked once, reference against reference: [(case, info)]."""
    return [(case, LF.run_case(LF.LadderReference, case)) for case in LF.case_list(SEED, N_CASES)]


def test_same_seed_same_cases_and_operations(default_walks):
    again = LF.case_list(SEED, N_CASES)
    assert again == [case for case, _ in default_walks]
    assert LF.case_list(SEED + 1, 4, pinned=()) != LF.case_list(SEED, 4, pinned=())
    for index in (0, len(LF.PINNED), len(again) - 1):
        assert LF.run_case(LF.LadderReference, again[index])["ops"] == default_walks[index][1]["ops"]


def test_cases_meet_the_engines_preconditions():
    for case in LF.case_list(SEED, 300):
        LF.check_case(case)
        x0, beta = LF.make_state(case)
        assert x0.shape == beta.shape == (case["n_chains"],) and np.all(beta > 0)
        if case["dtype"] == "f32":
            with np.errstate(over="ignore"):
                assert LF.same_floats(x0, x0.astype(np.float32).astype(np.float64))
        assert bool(case["plant"]) == bool(np.sum(~np.isfinite(x0)) or np.any(np.abs(x0) > 1e100))


def test_scripts_of_the_pinned_cases_ask_only_what_their_handles_take(default_walks):
    for case, info in default_walks[:len(LF.PINNED)]:
        n = len(case["script"])
        assert [tuple(op) for op in case["script"]] == info["ops"][:n] and len(info["ops"]) == case["n_ops"]


def test_default_list_meets_every_combination(default_walks):
    ops, events = collections.Counter(), collections.Counter()
    for _, info in default_walks:
        ops.update(op[0] for op in info["ops"])
        events.update(info["events"])
    assert set(ops) <= set(LF.OPERATIONS)
    assert not [name for name in LF.OPERATIONS if ops[name] < 3], dict(ops)
    assert not [name for name in EVENTS if events[name] < 1], dict(events)
    # both forms of the per-rung histogram: LDS rows while R (bins + 3) <= 12 288 counters, one global atomic per chain beyond
    assert set(LF.NEW_OPERATIONS) <= set(LF.OPERATIONS)
    # at most 40 % of the operations observe, and every drawn walk takes at least 8 mutating operations
    n_observers = sum(ops[name] for name in LF.OBSERVERS)
    assert n_observers <= 0.4 * sum(ops.values()), (n_observers, sum(ops.values()))
    assert not [info["taken"] for _, info in default_walks[len(LF.PINNED):] if info["taken"] < LF.MIN_MUTATORS]
    # no walk goes past the room a blocked accumulator starts with more than once
    for _, info in default_walks:
        names = [op[0] for op in info["ops"]]
        assert names.count("bridge") <= LF.MAX_SNAPSHOTS and names.count("mark") + names.count("sample") <= LF.MAX_SAMPLES
    forms = {case["R"] * (op[1] + 3) <= 12_288 for case, info in default_walks for op in info["ops"] if op[0] == "rung_hist"}
    assert forms == {True, False}


# ---- the walk has teeth ----------------------------------------------------------------------------------------------------------------
class _Patched:
    """A module attribute replaced while a block runs."""

    def __init__(self, module, name, value):
        self.module, self.name, self.value = module, name, value

    def __enter__(self):
        self.saved = getattr(self.module, self.name)
        setattr(self.module, self.name, self.value)

    def __exit__(self, *exc):
        setattr(self.module, self.name, self.saved)


class ParityFromTheNextStep(LF.LadderReference):
    """1: the gap parity is taken from t_x + 1 (the draw still from t_x)."""

    def exchange(self, n=1):
        gaps = X.gaps_of_step
        with _Patched(X, "gaps_of_step", lambda R, t: gaps(R, t + 1)):
            super().exchange(n)


class DrawKeyedByLocalId(LF.LadderReference):
    """2: the exchange draw is keyed by the local chain id."""

    def exchange(self, n=1):
        draw, off = X.draw_uniform, self.offset
        with _Patched(X, "draw_uniform", lambda seed, chain, t: draw(seed, chain - off, t)):
            super().exchange(n)


class TableReadTransposed(LF.LadderReference):
    """3: the table entry of (move k, rung r) is read at r K + k."""

    def table_as_read(self):
        K, R = self.table.shape
        flat = self.table.reshape(-1)
        return np.array([[flat[r * K + k] for r in range(R)] for k in range(K)])


class _EndRuleOnTheLeavingLabel(RP.RespaceTwin):
    def _swapped(self, a, r):
        lab = self.lab
        if lab is None:
            return
        lab[a], lab[a + 1] = lab[a + 1], lab[a]
        if r == 0:                               # the label that left rung 0 sits at a + 1 now
            self.round_trips += int(lab[a + 1] >> 6 == T.DOWN)
            lab[a + 1] = (lab[a + 1] & 63) | (T.UP << 6)
        if r + 1 == self.R - 1:                  # the label that left rung R - 1 sits at a now
            self.up_trips += int(lab[a] >> 6 == T.UP)
            lab[a] = (lab[a] & 63) | (T.DOWN << 6)


class EndRuleOnTheLeavingLabel(LF.LadderReference):
    """4: the end rule is applied to the label that leaves the end rung."""
    ladder_class = _EndRuleOnTheLeavingLabel


class LadderKeepsGapCounters(LF.LadderReference):
    """5: set_ladder keeps the old gap counters."""

    def set_ladder(self, n_rungs):
        old = self.tw.counters() if self.tw is not None else None
        super().set_ladder(n_rungs)
        if old is not None:
            n = min(old[0].size, self.tw.accepted.size)
            self.tw.accepted[:n], self.tw.attempted[:n] = old[0][:n], old[1][:n]


class StepIndexOf32Bits(LF.LadderReference):
    """6: the step index of the exchange draw is truncated to 32 bits."""

    def exchange(self, n=1):
        draw = X.draw_uniform
        with _Patched(X, "draw_uniform", lambda seed, chain, t: draw(seed, chain, t & 0xFFFFFFFF)):
            super().exchange(n)


def _row_with_the_last_bin_open(x, lo, hi, n_bins):
    out = LF.hist_row(x, lo, hi, n_bins)
    nan = np.isnan(x)
    inside = ~(nan | (x < lo) | (x >= hi))
    over = int(np.sum(((x[inside] - lo) * (n_bins / (hi - lo))).astype(np.int64) == n_bins))
    out[n_bins - 1] -= np.uint64(over)
    out[n_bins + 1] += np.uint64(over)
    return out


class HistogramSpillsTheLastBin(LF.LadderReference):
    """7: a position whose bin index comes out as n_bins is counted as >= hi."""
    hist_row = staticmethod(_row_with_the_last_bin_open)


class RespacingLeavesTheBridgeRecords(LF.LadderReference):
    """8: a respacing that is taken leaves the bridge records and their count."""

    def _respaced(self):
        pass


class RespacingClearsTheMask(LF.LadderReference):
    """9: a respacing that is taken frees the column mask along with the records."""

    def _respaced(self):
        super()._respaced()
        self.bridge_mask = 0


class RefusedRespacingZeroesTheGaps(LF.LadderReference):
    """10: a respacing that is not taken (status != 0) zeroes the gap counters."""

    def respace_ladder(self, *a, **k):
        super().respace_ladder(*a, **k)
        if self.tw.status != 0:
            self.tw.accepted[:] = 0
            self.tw.attempted[:] = 0


class BlockRowsSurviveARespacing(LF.LadderReference):
    """11: a respacing that is taken zeroes the merged records and leaves the rows per block."""

    def _respaced(self):
        rows = self.bridge_blk
        super()._respaced()
        self.bridge_blk = rows


class BlockOfTheLocalLadder(LF.LadderReference):
    """12: the block of a ladder is formed from its local index."""

    def block_first(self):
        return 0


class WindowIgnoresTheBase(LF.LadderReference):
    """13: the tuning reads the counters since they began, not since the window's base."""

    def window_base_for_tuning(self):
        return np.zeros_like(self.base)


class TableDropsTheBase(LF.LadderReference):
    """14: set_rung_sigma drops the window base."""

    def set_rung_sigma(self, sigma):
        super().set_rung_sigma(sigma)
        if sigma is not None and self.n_rungs:
            self.base[:] = 0


class UploadKeepsTheMark(LF.LadderReference):
    """15: upload_state keeps the mark."""

    def upload_state(self, x, beta=None):
        mark = self.corr
        super().upload_state(x, beta)
        self.corr = mark


class StepsHoldTheExchangeIndex(LF.LadderReference):
    """16: steps[s] records the exchange step index."""

    def corr_steps_entry(self):
        return self.exchange_step


class GroupsFollowTheWalker(LF.LadderReference):
    """17: the correlation groups follow the walker, not the rung."""

    def _observe(self, kind):
        o = super()._observe(kind)
        if not self.tracking:
            return o
        R = self.n_rungs
        walker = (self.tw.lab & np.uint8(63)).astype(np.int64)
        out = o.copy()
        out[(np.arange(o.size) // R) * R + walker] = o
        return out


DEFECTS = [ParityFromTheNextStep, DrawKeyedByLocalId, TableReadTransposed, EndRuleOnTheLeavingLabel, LadderKeepsGapCounters,
           StepIndexOf32Bits, HistogramSpillsTheLastBin,
           RespacingLeavesTheBridgeRecords, RespacingClearsTheMask, RefusedRespacingZeroesTheGaps, BlockRowsSurviveARespacing,
           BlockOfTheLocalLadder, WindowIgnoresTheBase, TableDropsTheBase, UploadKeepsTheMark, StepsHoldTheExchangeIndex,
           GroupsFollowTheWalker]


@pytest.mark.parametrize("defect", DEFECTS, ids=[d.__name__ for d in DEFECTS])
def test_walk_notices_a_defective_side(oracle, defect):
    """The defective object stands where the engine stands on the device.  The list is walked until the first case that fails."""
    caught = None
    for index, case in enumerate(LF.case_list(SEED, N_CASES)):
        try:
            LF.run_case(defect, case)
        except AssertionError as exc:
            caught = (index, str(exc))
            break
    assert caught is not None, f"no case of the default list notices: {defect.__doc__}"
    assert "case = " in caught[1] and "operations = " in caught[1] and repr(case["seed"]) in caught[1]


def test_unaltered_sides_agree(default_walks):
    """(what the fixture has shown already: every walk of the default list ends without a difference)"""
    assert len(default_walks) == len(LF.PINNED) + N_CASES
