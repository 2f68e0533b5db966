"""The random walks over a handle with one shared beta (tests/population_fuzz.py) on the host: that the cases are well formed and
repeat, that the default case list meets the combinations it is there for, and that the walk notices a reference with one deliberate
defect -- the evidence that tests/test_gpu_population_fuzz.py would notice the same kinds of error in a kernel or in the host code that
orders the kernels.  No GPU: both sides of the walk are reference objects."""
import collections

import numpy as np
import pytest

import anneal_twin as A
import population_fuzz as PF

N_CASES, SEED = PF.DEFAULT_CASES, PF.DEFAULT_SEED       # the list tests/test_gpu_population_fuzz.py walks on the device by default
EVENTS = [
    "anneal with a mark standing",
    "anneal refused under a partition, then taken after blocks_off",
    "search whose status is not OK",
    "annealing step with status != 0",
    "anneal_step >= 2^32 then a step",
    "families uploaded between steps",
]


@pytest.fixture(scope="module")
def default_walks(oracle):
    """The default case list walked once, reference against reference: [(case, info)]."""
    return [(case, PF.run_case(PF.PopulationReference, case)) for case in PF.case_list(SEED, N_CASES)]


def test_same_seed_same_cases_and_operations(default_walks):
    again = PF.case_list(SEED, N_CASES)
    assert again == [case for case, _ in default_walks]
    assert PF.case_list(SEED + 1, 4, pinned=()) != PF.case_list(SEED, 4, pinned=())
    for index in (0, len(PF.PINNED), len(again) - 1):
        assert PF.run_case(PF.PopulationReference, again[index])["ops"] == default_walks[index][1]["ops"]


def test_cases_meet_the_engines_preconditions():
    sizes = set()
    for case in PF.case_list(SEED, 300):
        PF.check_case(case)
        x0 = PF.make_state(case)
        assert x0.shape == (case["n_chains"],)
        if case["dtype"] == "f32":
            with np.errstate(over="ignore"):
                assert PF.same_floats(x0, x0.astype(np.float32).astype(np.float64))
        sizes.add(case["n_chains"])
    assert sizes == set(PF.CHAINS)


def test_scripts_of_the_pinned_cases_ask_only_what_their_handles_take(default_walks):
    for case, info in default_walks[:len(PF.PINNED)]:
        n = len(case["script"])
        assert [tuple(op) for op in case["script"]] == info["ops"][:n] and len(info["ops"]) == case["n_ops"]


def test_default_list_meets_every_combination(default_walks):
    ops, events = collections.Counter(), collections.Counter()
    for _, info in default_walks:
        ops.update(op[0] for op in info["ops"])
        events.update(info["events"])
    assert set(ops) <= set(PF.OPERATIONS) | {"search"}
    assert not [name for name in PF.OPERATIONS if ops[name] < 3], dict(ops)
    assert not [name for name in EVENTS if events[name] < 1], dict(events)
    # at most 40 % of the operations observe, every drawn walk takes at least 8 mutating operations, none more than 20 samples
    n_observers = sum(ops[name] for name in PF.OBSERVERS)
    assert n_observers <= 0.4 * sum(ops.values()), (n_observers, sum(ops.values()))
    assert not [info["taken"] for _, info in default_walks[len(PF.PINNED):] if info["taken"] < PF.MIN_MUTATORS]
    for _, info in default_walks:
        names = [op[0] for op in info["ops"]]
        assert names.count("mark") + names.count("sample") <= PF.MAX_SAMPLES
    # every ensemble size of the list, both state types, every search depth
    assert {case["n_chains"] for case, _ in default_walks} == set(PF.CHAINS)
    assert {case["dtype"] for case, _ in default_walks} == {"f64", "f32"}
    assert {op[3] for _, info in default_walks for op in info["ops"] if op[0] == "search"} == {1, 3, 6}


# ---- the walk has teeth ----------------------------------------------------------------------------------------------------------------
class AnnealKeepsTheMark(PF.PopulationReference):
    """1: a queued anneal keeps the mark."""

    def anneal(self, beta_new):
        mark, series = self._corr, self.series
        super().anneal(beta_new)
        self._corr, self.series = mark, series


class OffsetDrawCountsItsOwnSteps(PF.PopulationReference):
    """2: the offset's draw is keyed by the steps this handle has done, whatever anneal_step was set to."""

    done = 0

    def anneal(self, beta_new):
        if self.partition is None:
            t = self.twin.t_a
            self.twin.t_a = self.done
            try:
                super().anneal(beta_new)
            finally:
                self.twin.t_a = t + 1
            self.done += 1
        else:
            super().anneal(beta_new)


class FamiliesGatheredWithoutParents(PF.PopulationReference):
    """3: a step whose status is not 0 gathers the families all the same (through parents that were never written: zeros)."""

    def anneal(self, beta_new):
        super().anneal(beta_new)
        if int(self.twin.records[-1][0]) != A.OK and self.twin.fam is not None:
            self.twin.fam = self.twin.fam[np.zeros(self.n_chains, dtype=np.int64)]


class RefusedAnnealMovesBeta(PF.PopulationReference):
    """4: an anneal that is refused under a partition has moved beta already."""

    def anneal(self, beta_new):
        if self.partition is not None:
            self.beta = beta_new
        super().anneal(beta_new)


DEFECTS = [AnnealKeepsTheMark, OffsetDrawCountsItsOwnSteps, FamiliesGatheredWithoutParents, RefusedAnnealMovesBeta]


@pytest.mark.parametrize("defect", DEFECTS, ids=[d.__name__ for d in DEFECTS])
def test_walk_notices_a_defective_side(oracle, defect):
    """The defective object stands where the engine stands on the device.  The list is walked until the first case that fails."""
    caught = None
    for index, case in enumerate(PF.case_list(SEED, N_CASES)):
        try:
            PF.run_case(defect, case)
        except AssertionError as exc:
            caught = (index, str(exc))
            break
    assert caught is not None, f"no case of the default list notices: {defect.__doc__}"
    assert "case = " in caught[1] and "operations = " in caught[1] and repr(case["seed"]) in caught[1]


def test_unaltered_sides_agree(default_walks):
    """(what the fixture has shown already: every walk of the default list ends without a difference)"""
    assert len(default_walks) == len(PF.PINNED) + N_CASES
