"""Random operation walks over a handle with ONE shared beta -- population annealing, the choice of the next beta, the time
correlation and the jackknife blocks of a handle without a ladder -- against the host twins composed into one reference object.  The
counterpart of tests/ladder_fuzz.py, whose helpers it uses.

    PopulationReference   the surface of montecarlo_amd._capi.HipEngine that the walk uses: corr_twin.CorrTwinEngine and
                          anneal_search_twin.AnnealSearchTwinEngine over anneal_twin.AnnealTwinEngine (oracle_lib.OracleEngine
                          underneath), plus the partition at G = 1 (blocks_twin) and the refusals of include/amc.h.  What a call resets
                          or keeps follows the header and DESIGN.md sections 3.14 to 3.16.  It shares no code with the product.
    draw_case, check_case, PINNED, run_walk, run_case   as in ladder_fuzz.

The engine side is anything with HipEngine's surface: the host tests run the walk with a second reference object in its place.
"""
import numpy as np

import anneal_search_twin as AS
import anneal_twin as A
import blocks_twin as BL
import corr_twin as CT
import ladder_fuzz as LF
from ladder_fuzz import Refused, fbits, is_state_error, same_floats, same_ints, same_words

DEFAULT_CASES, DEFAULT_SEED = 40, 20261020       # AMC_POPULATION_FUZZ_CASES, AMC_POPULATION_FUZZ_SEED
CHAINS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3075]     # the wave, block and prefix-tile edges of the annealing kernels
MAX_SAMPLES = 20
MIN_MUTATORS = 8
OBSERVER_SHARE = 0.36
TWO32 = 1 << 32
STEP_VALUES = [0, 1, TWO32 - 1, TWO32, 1 << 47]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
class PopulationReference(CT.CorrTwinEngine, AS.AnnealSearchTwinEngine):
    """HipEngine's surface for a handle that holds the whole ensemble at one beta.  Constructor arguments as HipEngine's."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.partition = None            # (B, C) while a partition is set
        self.series = None               # the observable at the mark and at every sample, while the mark was made by corr_mark

    sweep_launches = A.AnnealTwinEngine.sweep
    reduce_state_records = LF.LadderReference.reduce_state_records

    # -- annealing ------------------------------------------------------------------------------------------------------------------------
    def anneal(self, beta_new):
        """A queued anneal clears the mark; it is refused, and changes nothing, while a partition is set."""
        if self.partition is not None:
            raise Refused("annealing while a partition is set")
        super().anneal(beta_new)         # (CorrTwinEngine.anneal forgets the mark)
        self.series = None

    def _families(self):
        if self.twin.fam is None:
            raise Refused("families are off")

    def anneal_family_stats(self):
        self._families()
        return super().anneal_family_stats()

    def download_families(self):
        self._families()
        return super().download_families()

    def upload_families(self, families):
        self._families()
        super().upload_families(families)

    # -- time correlation, one group; per block blocks_twin ---------------------------------------------------------------------------------
    def corr_mark(self, kind="energy"):
        super().corr_mark(kind)
        self.series = [self._corr["origin"]]

    def corr_sample(self):
        if self._corr is None:
            raise Refused("no mark")
        super().corr_sample()
        if self.series is not None:
            self.series.append(self._observe(self._corr["observable"]))

    def corr_origin(self):
        if self._corr is None:
            raise Refused("no mark")
        return super().corr_origin()

    def corr_clear(self):
        super().corr_clear()
        self.series = None

    def upload_state(self, x, beta=None):
        assert beta is None              # a shared beta: no per-chain array
        super().upload_state(x)          # (CorrTwinEngine.upload_state forgets the mark)
        self.series = None

    def set_blocks(self, n_blocks, chunk=0):
        """Forgets the mark on every call that succeeds; without a ladder a "ladder" is one chain, and the default chunk 256."""
        B = int(n_blocks)
        assert B == 0 or 2 <= B <= 64
        self.partition = None if B == 0 else (B, int(chunk) if int(chunk) else 256)
        self._corr, self.series = None, None

    def corr_fetch_blocks(self):
        if self.partition is None:
            raise Refused("no partition")
        B, C = self.partition
        if self._corr is None:
            return np.zeros((B, 0, 1, CT.COLS, CT.WORDS)), np.zeros(0, dtype=np.uint64), 0
        return (BL.corr_records(self.series, 1, B, C, first=0), np.array(self._corr["steps"], dtype=np.uint64), self._corr["observable"])


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def draw_case(rng):
    M = int(rng.choice(CHAINS))
    K = int(rng.choice([1, 2, 3]))
    w = rng.dirichlet(np.ones(K))
    w = w / w.sum()
    return dict(
        n_chains=M, potential=str(rng.choice(["harmonic", "double_well"])),
        sigma=[float(np.exp(rng.uniform(np.log(1e-2), np.log(10.0)))) for _ in range(K)], weight=[float(v) for v in w],
        seed=int(rng.integers(0, 2 ** 63)), dtype=str(rng.choice(["f64", "f64", "f32"])), per_chain_counters=bool(K > 1 or rng.random() < 0.5),
        beta=float(rng.uniform(0.2, 2.0)), plant=bool(rng.random() < 0.25), dominant=bool(rng.random() < 0.2),
        state_seed=int(rng.integers(0, 2 ** 31)), walk_seed=int(rng.integers(0, 2 ** 31)), n_ops=int(rng.integers(14, 29)), script=[])


def make_state(case, rng=None):
    """x0: normal(0, 1.5), through Float32 for Float32 state; `dominant`: one chain at the bottom of the potential and the others far
    out, so that a cooling step gives it nearly every child; `plant`: a NaN, +Inf, -Inf and 1e200 where the ensemble has room."""
    rng = rng if rng is not None else np.random.default_rng([case["state_seed"], 78])
    M = case["n_chains"]
    x0 = rng.normal(0.0, 1.5, M)
    if case["dominant"] and M > 1:
        x0 = np.sign(x0) * (6.0 + np.abs(x0))
        x0[int(rng.integers(0, M))] = 1.0 if case["potential"] == "double_well" else 0.0
    if case["plant"] and M > 4:
        where = rng.choice(M, size=4, replace=False)
        x0[where] = [np.nan, np.inf, -np.inf, 1e200]
    if case["dtype"] == "f32":
        with np.errstate(over="ignore"):
            x0 = x0.astype(np.float32).astype(np.float64)
    return x0


def engine_kwargs(case):
    return dict(n_chains=case["n_chains"], potential=case["potential"], beta=case["beta"], sigma=case["sigma"], weight=case["weight"],
                seed=case["seed"], per_chain_counters=case["per_chain_counters"], dtype=case["dtype"])


def check_case(case):
    """The engine's preconditions."""
    K = len(case["sigma"])
    assert case["n_chains"] in CHAINS and K in (1, 2, 3) and len(case["weight"]) == K and abs(sum(case["weight"]) - 1.0) < 1e-12
    assert case["per_chain_counters"] or K == 1
    assert np.isfinite(case["beta"]) and 0 <= case["seed"] < 2 ** 63 and all(1e-100 <= s <= 1e100 for s in case["sigma"])


def pinned_case(M, script, **kw):
    case = dict(n_chains=M, potential="harmonic", sigma=[0.6], weight=[1.0], seed=20260311, dtype="f64", per_chain_counters=True, beta=0.5,
                plant=False, dominant=False, state_seed=M, walk_seed=M + 1, n_ops=len(script) + 6, script=[list(op) for op in script])
    case.update(kw)
    return case


PINNED = [
    # an anneal behind a standing mark forgets it; refused under a partition and taken once the partition is off; the refused call
    # leaves beta, the step index and the log where they were
    pinned_case(257, [("mark", "energy"), ("single", 2), ("sample",), ("anneal", "cool"), ("corr_fetch",), ("refused", "sample"),
                      ("blocks", 3, 5), ("mark", "x"), ("single", 1), ("sample",), ("refused", "anneal"), ("beta",), ("records",),
                      ("anneal_step",), ("corr_blocks",), ("blocks_off",), ("anneal", "cool"), ("records",), ("state",)]),
    # the offset draw at a step index of 2^32 and beyond; families uploaded between two steps; a heating step over planted infinities
    # (status 2): beta moves, the positions and the families stay
    pinned_case(1025, [("families_on",), ("set_step", TWO32 - 1), ("anneal", "cool"), ("anneal", "cool"), ("families",),
                       ("families_put",), ("anneal", "cool"), ("families",), ("upload",), ("anneal", "heat"), ("records",), ("families",),
                       ("state",), ("set_step", 1 << 47), ("anneal", "same"), ("records",)],
                potential="double_well", plant=True, sigma=[0.8, 0.11], weight=[0.625, 0.375]),
    # Float32 state, one dominant chain, a far beta that leaves most weights 0; searches of every round count
    pinned_case(3075, [("search", "cool", 0.8, 1), ("search", "far", 0.3, 3), ("search", "same", 0.8, 6), ("search", "heat", 0.999, 3),
                       ("anneal", "far"), ("records",), ("state",), ("reduce",)],
                dtype="f32", dominant=True, per_chain_counters=False),
    # the smallest ensembles
    pinned_case(1, [("families_on",), ("anneal", "cool"), ("search", "cool", 0.8, 3), ("families",), ("records",)]),
    pinned_case(2, [("mark", "x"), ("anneal", "heat"), ("search", "far", 0.3, 6), ("records",), ("corr_fetch",)], dominant=True),
]


def case_list(seed, n_cases, pinned=PINNED):
    return [dict(c) for c in pinned] + [draw_case(np.random.default_rng([seed, i])) for i in range(n_cases)]


# ---- the walk --------------------------------------------------------------------------------------------------------------------------
MUTATORS = ["single", "single", "multi", "launches", "anneal", "anneal", "anneal", "anneal", "search", "search", "search", "families_on",
            "families_on", "families_off", "families_put", "records_reset", "records_put", "set_step", "set_step", "set_beta", "mark", "mark",
            "sample", "sample", "sample", "corr_clear", "blocks", "blocks", "blocks_off", "blocks_off", "upload", "recount", "sigma",
            "refused", "refused"]
OBSERVERS = ["state", "counters", "records", "beta", "anneal_step", "families", "corr_fetch", "corr_blocks", "reduce"]
OPERATIONS = sorted(set(MUTATORS)) + OBSERVERS
REFUSALS = ["anneal", "sample", "family_stats", "download_families", "upload_families"]
ANNEAL_KINDS = ["cool", "cool", "heat", "same", "far"]


def new_context():
    return dict(samples=0, records=None)


def refusals(ref):
    out = []
    if ref.partition is not None:
        out.append("anneal")
    if ref._corr is None:
        out.append("sample")
    if ref.twin.fam is None:
        out += ["family_stats", "download_families", "upload_families"]
    return out


def possible(ref, name, ctx):
    if name == "anneal":
        return ref.partition is None
    if name in ("families_off", "families_put", "families"):
        return ref.twin.fam is not None
    if name == "sample":
        return ref._corr is not None and ctx["samples"] < MAX_SAMPLES
    if name == "mark":
        return ctx["samples"] < MAX_SAMPLES
    if name in ("blocks_off", "corr_blocks"):
        return ref.partition is not None
    if name == "recount":
        return ref.per_chain_counters
    if name == "refused":
        return bool(refusals(ref))
    return True


def target_beta(ref, kind):
    """The beta an anneal or a search of `kind` goes to, from the beta at hand (a deterministic function of the reference's state)."""
    b = ref.beta
    return dict(cool=b * 1.3 + 0.05, heat=b * 0.7 - 0.01, same=b, far=b + 1e6)[kind]


def draw_op(rng, ref, ctx, mutator=False):
    names = OBSERVERS if not mutator and rng.random() < OBSERVER_SHARE else MUTATORS      # the kind first: the share holds
    for _ in range(64):
        name = str(rng.choice(names))
        if not possible(ref, name, ctx):
            continue
        if name in ("single", "launches"):
            return (name, int(rng.integers(1, 6)))
        if name == "multi":
            return (name, int(rng.integers(2, 12)))
        if name == "anneal":
            return (name, str(rng.choice(ANNEAL_KINDS)))
        if name == "search":
            return (name, str(rng.choice(ANNEAL_KINDS)), float(rng.choice([0.3, 0.8, 0.999])), int(rng.choice([1, 3, 6])))
        if name == "set_step":              # (the observers "anneal_step" and "beta" read what these two write)
            return (name, int(rng.choice(STEP_VALUES)))
        if name == "set_beta":
            return (name, float(rng.uniform(0.2, 2.0)))
        if name == "mark":
            return (name, str(rng.choice(["energy", "x"])))
        if name == "blocks":
            return (name, int(rng.choice([2, 3, 32, 64])), int(rng.choice([0, 1, 5, ref.n_chains])))
        if name == "recount":
            return (name, int(rng.choice(LF.RECOUNT_STEPS)))
        if name == "refused":
            return (name, str(rng.choice(refusals(ref))))
        return (name,)
    return ("single", 1) if mutator else ("state",)


def apply_op(op, s, rng, ref, ctx, case):
    """Side `s` takes a mutating operation of a handle in the state `ref` is in; its arrays are drawn here from rng."""
    name = op[0]
    K, M = ref.n_moves, ref.n_chains
    if name == "single":
        for _ in range(op[1]):
            s.sweep(1)
    elif name == "multi":
        s.sweep(op[1])
    elif name == "launches":
        s.sweep_launches(op[1])
    elif name == "anneal":
        s.anneal(target_beta(ref, op[1]))
    elif name == "families_on":
        s.set_anneal_families(True)
    elif name == "families_off":
        s.set_anneal_families(False)
    elif name == "families_put":            # any ids below n_chains, repeated ones among them
        s.upload_families(rng.integers(0, M, M).astype(np.uint32))
    elif name == "records_reset":
        s.anneal_records(reset=True)
    elif name == "records_put":
        s.set_anneal_records(ctx["records"] if ctx["records"] is not None else np.zeros((0, 8), dtype=np.uint64))
    elif name == "set_step":
        s.anneal_step = op[1]
    elif name == "set_beta":
        s.beta = op[1]
    elif name == "mark":
        s.corr_mark(op[1])
    elif name == "sample":
        s.corr_sample()
    elif name == "corr_clear":
        s.corr_clear()
    elif name == "blocks":
        s.set_blocks(op[1], op[2])
    elif name == "blocks_off":
        s.set_blocks(0, 0)
    elif name == "upload":
        s.upload_state(make_state(case, rng))
    elif name == "recount":
        tot = rng.multinomial(op[1], case["weight"], size=M).T.astype(np.int64)
        s.upload_counters((tot * rng.uniform(0, 1, tot.shape)).astype(np.int64), tot)
    elif name == "sigma":
        s.set_parameters(int(rng.integers(0, K)), [float(np.exp(rng.uniform(np.log(1e-2), np.log(10.0))))])
    else:
        raise ValueError(op)


def refuse(which, side, ref):
    """The call `which` of the fixed list on `side`: the exception it raised, or None when the side took it."""
    try:
        if which == "anneal":
            side.anneal(target_beta(ref, "cool"))
        elif which == "sample":
            side.corr_sample()
        elif which == "family_stats":
            side.anneal_family_stats()
        elif which == "download_families":
            side.download_families()
        elif which == "upload_families":
            side.upload_families(np.arange(ref.n_chains, dtype=np.uint32))
        else:
            raise ValueError(which)
    except (AssertionError, ValueError):
        raise
    except Exception as exc:
        return exc
    return None


def observe(op, eng, ref, fail, ctx):
    name = op[0]
    if name == "state":
        (x, e), (xo, eo) = eng.download_state(), ref.download_state()
        if not same_floats(x, xo):
            fail("positions differ", np.flatnonzero(fbits(x) != fbits(xo))[:8])
        if not same_floats(e, eo):
            fail("energies differ", np.flatnonzero(fbits(e) != fbits(eo))[:8])
    elif name == "counters":
        if ref.per_chain_counters:
            (a, t), (ao, to) = eng.download_counters(), ref.download_counters()
        else:
            (a, t), (ao, to) = eng.counter_totals(), ref.counter_totals()
        if not (same_ints(a, ao) and same_ints(t, to)):
            fail("Move counters differ")
    elif name == "records":
        got, want = np.asarray(eng.anneal_records(), dtype=np.uint64), np.asarray(ref.anneal_records(), dtype=np.uint64)
        if got.shape != want.shape or not np.array_equal(got, want):
            fail("annealing records differ", (got, want))
        ctx["records"] = want.copy()
    elif name == "beta":
        if not same_floats(eng.beta, ref.beta):
            fail("the shared beta differs", (eng.beta, ref.beta))
    elif name == "anneal_step":
        if eng.anneal_step != ref.anneal_step:
            fail("annealing step index differs", (eng.anneal_step, ref.anneal_step))
    elif name == "families":
        if not same_ints(eng.download_families(), ref.download_families()):
            fail("family ids differ")
        if tuple(eng.anneal_family_stats()) != tuple(ref.anneal_family_stats()):
            fail("family statistics differ", (eng.anneal_family_stats(), ref.anneal_family_stats()))
    elif name == "corr_fetch":
        (rec, st, ob), (reco, sto, obo) = eng.corr_fetch(), ref.corr_fetch()
        if ob != obo or not same_ints(st, sto) or not same_words(rec, reco):
            fail("correlation records differ", (ob, obo, st, sto))
        if obo and not same_floats(eng.corr_origin(), ref.corr_origin()):
            fail("the origin differs")
    elif name == "corr_blocks":
        (blk, st, ob), (blko, sto, obo) = eng.corr_fetch_blocks(), ref.corr_fetch_blocks()
        if ob != obo or not same_ints(st, sto) or not same_words(blk, blko):
            fail("correlation records per block differ", (ob, obo, st, sto, np.shape(blk), np.shape(blko)))
        if len(sto) and not same_words(BL.merge_blocks(blk), eng.corr_fetch()[0]):
            fail("the merge over the blocks is not the merged correlation fetch")
    elif name == "reduce":
        got = eng.reduce_state_records() if hasattr(eng, "reduce_state_records") else np.asarray(eng.reduce_exact()[0])[:3]
        if not np.array_equal(fbits(got), fbits(ref.reduce_state_records())):
            fail("records of sum e, sum x, sum x^2 differ")
    else:
        raise ValueError(op)


def run_walk(engine, ref, rng, n_ops, case, script=()):
    """`script`, then operations drawn from rng until n_ops are done (and, in a drawn case, MIN_MUTATORS mutating ones are taken); the
    comparison of everything at the end.  Returns dict(ops, events, taken)."""
    ops, events = [], set()

    def fail(what, detail=None):
        raise AssertionError(f"after operation {len(ops) - 1} {ops[-1] if ops else ''}: {what}" + (f"\n{detail}" if detail is not None else "") +
                             f"\ncase = {case!r}\noperations = {ops!r}")

    ctx = new_context()
    taken, wanted = 0, 0 if script else MIN_MUTATORS
    refused_anneal = families_put = False
    queue = [tuple(op) for op in script]
    while len(ops) < max(n_ops, len(script)) or taken < wanted:
        op = queue.pop(0) if queue else draw_op(rng, ref, ctx, mutator=len(ops) >= max(n_ops, len(script)))
        name = op[0]
        ops.append(op)
        if name in OBSERVERS:
            if not possible(ref, name, ctx):
                fail("the script asks for an observation the handle cannot give")
            observe(op, engine, ref, fail, ctx)
            continue
        if name == "search":                   # compared at once, then an anneal to the result (refused under a partition)
            limit = target_beta(ref, op[1])
            try:
                got = engine.anneal_next_beta(limit, op[2], op[3])
            except Exception as exc:
                fail(f"the engine refused: {exc!r}")
            want = ref.anneal_next_beta(limit, op[2], op[3])
            if not same_floats(got[0], want[0]) or not same_ints(got[1], want[1]) or not same_ints(got[2], want[2]):
                fail("the search differs", (got, want))
            if int(want[1][0]) != AS.OK:
                events.add("search whose status is not OK")
            if ref.partition is not None:
                op = ("refused", "anneal")
            else:
                op = ("anneal", None, float(want[0]))
            name = op[0]
        elif not possible(ref, name, ctx) or (name == "refused" and op[1] not in refusals(ref)):
            fail("the script asks for an operation the handle cannot take")
        if name == "refused":                  # both sides refuse with AMC_ERR_STATE; the observers that follow show nothing moved
            for side, who in ((engine, "the engine"), (ref, "the reference")):
                exc = refuse(op[1], side, ref)
                if exc is None or not is_state_error(exc):
                    fail(f"{who} did not refuse with AMC_ERR_STATE: {exc!r}")
            refused_anneal = refused_anneal or op[1] == "anneal"
            continue
        taken += 1
        if name == "anneal":
            if ref._corr is not None:
                events.add("anneal with a mark standing")
            if refused_anneal:
                events.add("anneal refused under a partition, then taken after blocks_off")
            if ref.anneal_step >= TWO32:
                events.add("anneal_step >= 2^32 then a step")
            if families_put and ref.twin.fam is not None:
                events.add("families uploaded between steps")
        arrays = int(rng.integers(0, 2 ** 62))     # both sides draw the operation's arrays from generators with this one seed
        for side in (engine, ref):
            try:
                if name == "anneal" and op[1] is None:
                    side.anneal(op[2])
                else:
                    apply_op(op, side, np.random.default_rng(arrays), ref, ctx, case)
            except AssertionError:
                raise
            except Exception as exc:
                if side is ref:
                    raise
                fail(f"the engine refused: {exc!r}")
        if name == "anneal":
            if int(ref.twin.records[-1][0]) != A.OK:
                events.add("annealing step with status != 0")
        elif name in ("mark", "sample"):
            ctx["samples"] += 1
        elif name == "families_put":
            families_put = bool(ref.twin.records)      # between two steps: one has been taken already
        elif name in ("families_on", "families_off"):
            families_put = False
    ops.append(("end",))
    for name in OBSERVERS:
        if possible(ref, name, ctx):
            observe((name,), engine, ref, fail, ctx)
    if engine.step != ref.step:
        fail("step index differs", (engine.step, ref.step))
    return dict(ops=ops[:-1], events=events, taken=taken)


def run_case(factory, case, reference_factory=PopulationReference):
    """Engine and reference of `case`, the state, the walk; both closed whatever happens."""
    check_case(case)
    x0 = make_state(case)
    ref = reference_factory(**engine_kwargs(case))
    eng = None
    try:
        eng = factory(**engine_kwargs(case))
        for s in (eng, ref):
            s.upload_state(x0)
        rng = np.random.default_rng([case["walk_seed"], 6])
        return run_walk(eng, ref, rng, case["n_ops"], case, script=case.get("script", ()))
    finally:
        ref.close()
        if eng is not None:
            eng.close()
