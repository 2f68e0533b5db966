"""The host side of the moments per energy bin per jackknife block (DESIGN.md section 3.17 "Moments per block"), no GPU: the twin of
the blocked cells (tests/emom_blocks_twin.py) against explicit loops, ``jackknife.jackknife_integers`` / ``leave_one_out_integers``
against brute force in Python integers, their refusals, the reworded ``check_blocks`` message, and the ``EnergyHistogram`` surface
and the checkpoint sections over the engine double of the host tests (exchange_twin.TwinEngine) extended with the twin."""
import numpy as np
import pytest

import montecarlo_amd as ma
from montecarlo_amd.jackknife import block_counts, check_blocks, jackknife_integers, leave_one_out_integers

import emom_blocks_twin as EB
import emom_twin as E
import exchange_twin as X

ALL = E.X | E.XX | E.POS


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,L,B,chunk,first", [(1, 65, 2, 1, 0), (3, 22, 4, 3, 0), (7, 37, 5, 1, 11), (2, 3, 3, 1, 0), (3, 6, 4, 4, 8)])
def test_twin_is_the_rule_per_chain_composed_with_the_block_rule(G, L, B, chunk, first):
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.8, 1.8, G * L)
    x[::17] = np.nan
    e = (x * x - 1.0) ** 2
    lo, hi, n, bound = 0.125, 2.5, 23, 1.5
    counts, sums = EB.moments(e, x, lo, hi, n, ALL, bound, G, B, chunk, first)
    want_c, want_s = np.zeros((B, G, n + 4), dtype=np.uint64), np.zeros((B, G, 3, n), dtype=np.int64)
    for i in range(G * L):                                  # chain i: rung i mod G of local ladder i div G
        c1, s1 = E.moments(e[i:i + 1], x[i:i + 1], lo, hi, n, ALL, bound, 1)
        b = ((first + i // G) // chunk) % B
        want_c[b, i % G] += c1[0]
        want_s[b, i % G] += s1[0]
    assert np.array_equal(counts, want_c) and np.array_equal(sums, want_s)
    whole = E.moments(e, x, lo, hi, n, ALL, bound, G)
    assert np.array_equal(counts.sum(axis=0, dtype=np.uint64), whole[0]) and np.array_equal(sums.sum(axis=0), whole[1])
    per_block = block_counts(L, B, chunk, first)
    assert np.array_equal(counts.sum(axis=2), np.repeat(per_block.astype(np.uint64)[:, None], G, axis=1))
    assert counts[:, :, n + 3].sum() > 0 and counts[:, :, n + 2].sum() > 0


# ---- the jackknife over several integer arrays ---------------------------------------------------------------------------------------------
def _arrays(rng, B=7):
    counts = rng.integers(1, 40, size=(B, 3, 11)).astype(np.uint64)
    sums = rng.integers(-2 ** 40, 2 ** 40, size=(B, 3, 2, 11)).astype(np.int64)
    counts[3] += np.uint64(1) << np.uint64(60)              # beyond 2^53: a Float64 total would round
    sums[2] -= np.int64(1) << np.int64(59)
    sums[5] += (np.int64(1) << np.int64(59)) + np.int64(1)
    return counts, sums


def test_leave_one_out_totals_are_exact():
    rng = np.random.default_rng(21)
    counts, sums = _arrays(rng)
    totals, loo = leave_one_out_integers([counts, sums])
    B = counts.shape[0]
    for arr, tot, k in ((counts, totals[0], 0), (sums, totals[1], 1)):
        assert tot.dtype == arr.dtype and tot.shape == arr.shape[1:]
        flat = arr.reshape(B, -1)
        exact = [sum(int(flat[b, i]) for b in range(B)) for i in range(flat.shape[1])]          # Python integers: no width
        assert [int(v) for v in tot.reshape(-1)] == exact
        for b in range(B):
            assert loo[b][k].dtype == arr.dtype
            assert [int(v) for v in loo[b][k].reshape(-1)] == [exact[i] - int(flat[b, i]) for i in range(flat.shape[1])]


def test_jackknife_integers_against_brute_force():
    rng = np.random.default_rng(22)
    counts, sums = _arrays(rng)
    seen = []

    def fn(c, s):
        assert c.dtype == np.uint64 and s.dtype == np.int64
        seen.append((c.copy(), s.copy()))
        low = (c & np.uint64(0xFFFFFFFF)).astype(np.float64)
        return np.concatenate([(s[:, 0].astype(np.float64) / low).sum(axis=1), np.log(low[:, 0])])

    theta, se = jackknife_integers([counts, sums], fn)
    B = counts.shape[0]
    assert len(seen) == B + 1 and np.array_equal(seen[0][0], counts.sum(axis=0, dtype=np.uint64))          # the totals come first
    assert np.array_equal(theta, fn(counts.sum(axis=0, dtype=np.uint64), sums.sum(axis=0, dtype=np.int64)))
    reps = np.stack([fn(np.sum([counts[k] for k in range(B) if k != b], axis=0, dtype=np.uint64),
                        np.sum([sums[k] for k in range(B) if k != b], axis=0, dtype=np.int64)) for b in range(B)])
    want = np.sqrt((B - 1) / B * ((reps - reps.mean(axis=0)) ** 2).sum(axis=0))
    assert np.array_equal(se, want) and np.all(se > 0)
    # one array alone is jackknife_counts
    from montecarlo_amd.jackknife import jackknife_counts
    one = lambda c: (c & np.uint64(0xFFFFFFFF)).astype(np.float64).sum(axis=1)
    a, b = jackknife_integers([counts], one), jackknife_counts(counts, one)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_refusals_of_the_helper():
    rng = np.random.default_rng(23)
    counts, sums = _arrays(rng)
    fn = lambda c, s: c.sum(dtype=np.float64)
    with pytest.raises(ValueError, match="at least 2"):
        jackknife_integers([counts[:1], sums[:1]], fn)
    empty_c, empty_s = counts.copy(), sums.copy()
    empty_c[4] = 0
    empty_s[4] = 0
    with pytest.raises(ValueError, match="block 4 is empty"):
        jackknife_integers([empty_c, empty_s], fn)
    with pytest.raises(ValueError, match="uint64 or int64"):
        jackknife_integers([counts, sums.astype(np.float64)], fn)
    with pytest.raises(ValueError, match="one B"):
        jackknife_integers([counts, sums[:5]], fn)
    with pytest.raises(ValueError, match="no arrays"):
        jackknife_integers([], fn)


def test_the_reworded_message_of_check_blocks():
    with pytest.raises(ValueError, match="larger than the 3 chunks") as info:
        check_blocks("EnergyHistogram", 4, None, 131, 4)    # the default chunk 64 makes 3 chunks of 131 ladders
    assert "jackknife block" in str(info.value) and "would be empty" in str(info.value)
    with pytest.raises(ValueError, match="larger than the 1 chunks"):
        check_blocks("Autocorrelation", 2, None, 64, 1)
    assert check_blocks("EnergyHistogram", 4, 5, 131, 4) == (4, 5)


# ---- the EnergyHistogram surface over the engine double -----------------------------------------------------------------------------------
class EmomBlocksTwinEngine(X.TwinEngine):
    """exchange_twin.TwinEngine plus the partition and the moments' surface of montecarlo_amd._capi.HipEngine, plain and per block,
    computed by emom_blocks_twin.  The accumulator is kept per block whenever it is blocked; the plain fetch is its sum."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.potential = kw.get("potential", "harmonic")
        self.first = int(kw.get("chain_offset", 0))
        self.part, self._emom, self.calls = None, None, []

    def ladder(self):
        return np.array(self._beta[:self.n_rungs], dtype=np.float64)

    def energy_histogram_accumulate(self, lo, hi, n_bins):     # (EnergyHistogram asks for the attribute; with moments it is never called)
        raise AssertionError("the plain energy histograms are not part of this double")

    def set_blocks(self, n_blocks, chunk=0):
        self.calls.append(("blocks", int(n_blocks), int(chunk)))
        if self._emom is not None and self._emom["blocked"]:          # the fold
            m = self._emom
            m.update(counts=m["counts"].sum(axis=0, dtype=np.uint64)[None], sums=m["sums"].sum(axis=0, dtype=np.int64)[None], blocked=False)
        self.part = (int(n_blocks), int(chunk)) if n_blocks else None

    def _groups(self):
        return max(int(getattr(self, "n_rungs", 0) or 0), 1)

    def _accumulate(self, form, blocked):
        G = self._groups()
        part = self.part if blocked else (1, 1)
        if self._emom is None:
            cols = bin(form[3]).count("1")
            self._emom = dict(form=form, blocked=blocked, n=0, counts=np.zeros((part[0], G, form[2] + 4), dtype=np.uint64),
                              sums=np.zeros((part[0], G, cols, form[2]), dtype=np.int64))
        m = self._emom
        assert m["form"] == form and m["blocked"] == blocked
        c, s = EB.snapshot(self.potential, self.download_state(want_e=False)[0], *form, G, *part, self.first // G)
        m["counts"] += c
        m["sums"] += s
        m["n"] += 1

    def energy_moments_accumulate(self, lo, hi, n_bins, mask, x_bound):
        self._accumulate((float(lo), float(hi), int(n_bins), int(mask), float(x_bound)), False)

    def energy_moments_accumulate_blocks(self, lo, hi, n_bins, mask, x_bound):
        assert self.part is not None
        self._accumulate((float(lo), float(hi), int(n_bins), int(mask), float(x_bound)), True)

    def energy_moments_fetch(self, reset=False):
        m, G = self._emom, self._groups()
        if m is None:
            return np.zeros((G, 0), dtype=np.uint64), np.zeros((G, 0, 0), dtype=np.int64), 0, (0.0, 0.0, 0, 0, 0.0)
        if reset:
            self._emom = None
        return m["counts"].sum(axis=0, dtype=np.uint64), m["sums"].sum(axis=0, dtype=np.int64), m["n"], m["form"]

    def energy_moments_fetch_blocks(self, reset=False):
        m = self._emom
        if m is None or not m["blocked"]:
            raise ma.AmcError("no accumulator kept per jackknife block stands")
        if reset:
            self._emom = None
        return m["counts"].copy(), m["sums"].copy(), m["n"], m["form"]

    def set_energy_moments(self, lo=0.0, hi=0.0, n_bins=0, mask=0, x_bound=0.0, counts=None, sums=None, n_snapshots=0):
        self._emom = None if counts is None or not n_snapshots else dict(
            form=(float(lo), float(hi), int(n_bins), int(mask), float(x_bound)), blocked=False, n=int(n_snapshots),
            counts=np.array(counts, dtype=np.uint64)[None], sums=np.array(sums, dtype=np.int64)[None])

    def set_energy_moments_blocks(self, lo=0.0, hi=0.0, n_bins=0, mask=0, x_bound=0.0, counts=None, sums=None, n_snapshots=0):
        assert self.part is not None and np.shape(counts)[0] == self.part[0]
        self._emom = dict(form=(float(lo), float(hi), int(n_bins), int(mask), float(x_bound)), blocked=True, n=int(n_snapshots),
                          counts=np.array(counts, dtype=np.uint64), sums=np.array(sums, dtype=np.int64))


R, L = 3, 24
BETAS = 0.5 * 1.5 ** np.arange(R)
BINS = dict(lo=0.0, hi=40.0, n_bins=40)
MOMENTS, X_BOUND = ("x", "x2", "pos"), 3.0


def build(path, steps, scheduler, blocks=4, chunk=2, moments=MOMENTS):
    chains = ma.ParticleChains.ladder(L, BETAS, "double_well", x=np.linspace(-1.5, 1.5, R * L))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.6], 1.0),)
    extra = dict(moments=moments, x_bound=X_BOUND) if moments else {}
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=11, engine_factory=EmomBlocksTwinEngine),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), n_rungs=R),
          dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), scheduler=scheduler, blocks=blocks,
               block_chunk=chunk if blocks else None, **BINS, **extra)]
    return ma.Simulation(chains, al, steps, path=str(path))


def test_the_surface_with_error_bars(oracle, tmp_path):
    sim = build(tmp_path, 40, list(range(2, 41, 2)))
    ma.run(sim)
    eh, eng = sim.algorithms[-1], sim.algorithms[0].engine
    assert [c for c in eng.calls if c[0] == "blocks"] == [("blocks", 4, 2)]              # the partition is set once
    n = BINS["n_bins"]
    assert eh.n_snapshots == 20
    cb, sb = eh.counts_blocks(), eh.moment_sums_blocks()
    assert cb.shape == (4, R, n + 3) and cb.dtype == np.uint64 and sb.shape == (4, R, 3, n) and sb.dtype == np.float64
    assert np.array_equal(cb.sum(axis=0, dtype=np.uint64), eh.counts())
    assert np.array_equal(cb.sum(axis=2), np.uint64(20) * np.repeat(block_counts(L, 4, 2).astype(np.uint64)[:, None], R, axis=1))
    k = eng.energy_moments_fetch_blocks()[1]
    quanta = np.array([2.0 ** (2 - 32), 2.0 ** (4 - 32), 1.0])                            # x_bound = 3: eb = 2
    assert np.array_equal(sb, k.astype(np.float64) * quanta[None, None, :, None])
    assert np.array_equal(k.sum(axis=0).astype(np.float64) * quanta[None, :, None], eh.moment_sums())
    grid = np.linspace(BETAS[0], BETAS[-1], 5)
    plain = eh.reweight_moments(grid)
    pairs = eh.reweight_moments(grid, error=True)
    assert tuple(pairs) == MOMENTS
    for name in MOMENTS:
        value, se = pairs[name]
        assert np.array_equal(value, plain[name]) and se.shape == grid.shape and np.all(np.isfinite(se)) and np.all(se > 0), name
    # the replicates by hand: WHAM on the leave-one-out counts from the full solution, reweight_observable with its sums and counts
    from montecarlo_amd import reweighting as rw
    counts4, _, _, _ = eng.energy_moments_fetch_blocks()
    total_c, total_k = counts4.sum(axis=0, dtype=np.uint64), k.sum(axis=0)
    f = rw.wham(total_c[:, :n], BETAS, eh.energies())[1]
    reps = []
    for b in range(4):
        c, s = (total_c - counts4[b])[:, :n], (total_k - k[b]).astype(np.float64) * quanta[None, :, None]
        lg = rw.wham(c, BETAS, eh.energies(), f0=f)[0]
        reps.append(np.stack([rw.reweight_observable(lg, eh.energies(), grid, s[:, j], c) for j in range(3)]))
    reps = np.stack(reps)
    want = np.sqrt(3 / 4 * ((reps - reps.mean(axis=0)) ** 2).sum(axis=0))
    assert np.array_equal(np.stack([pairs[m][1] for m in MOMENTS]), want)
    # the counts' results take error=True from the same counts; the callback
    values, with_se = eh.reweight(grid), eh.reweight(grid, error=True)
    assert all(np.array_equal(p[0], v) and p[1].shape == v.shape for p, v in zip(with_se, values))
    fe, fe_se = eh.free_energies(error=True)
    assert np.array_equal(fe, eh.free_energies()) and fe_se[0] == 0.0 and np.all(fe_se[1:] > 0)
    assert eh.density_of_states(error=True)[1][1].shape == (n,)
    out = ma.callback_reweight_moments_error(sim)
    assert out.shape == (3, R) and np.all(out > 0)
    # without blocks: the same integers, and error=True is refused
    other = build(tmp_path / "p", 40, list(range(2, 41, 2)), blocks=None)
    ma.run(other)
    eo = other.algorithms[-1]
    assert np.array_equal(eo.counts(), eh.counts()) and np.array_equal(eo.moment_sums(), eh.moment_sums())
    assert all(np.array_equal(eo.reweight_moments(grid)[m], plain[m]) for m in MOMENTS)
    with pytest.raises(ValueError, match="needs blocks"):
        eo.reweight_moments(grid, error=True)
    with pytest.raises(ValueError, match="need blocks"):
        eo.moment_sums_blocks()
    eh.restart()
    assert eh.n_snapshots == 0 and not eh.counts_blocks().any() and not eh.moment_sums_blocks().any()


def test_refusals_of_the_surface(oracle, tmp_path):
    with pytest.raises(ValueError, match="jackknife block"):
        build(tmp_path, 2, [2], blocks=4, chunk=None)       # the default chunk 85 makes 1 chunk of 24 ladders
    chains = ma.ParticleChains.ladder(L, BETAS, "double_well", x=np.linspace(-1.5, 1.5, R * L))
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.6], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=11, engine_factory=EmomBlocksTwinEngine),
          dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), scheduler=[2], blocks=4, block_chunk=2, moments=MOMENTS, x_bound=X_BOUND, **BINS),
          dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=[3], betas=[1.5])]
    with pytest.raises(ValueError, match="PopulationAnnealing"):
        ma.run(ma.Simulation(chains, al, 4, path=str(tmp_path / "pa")))
    # _jackknife's refusals, on cells planted through the checkpoint entry: a replicate whose histograms no longer connect (without
    # block 0 rung 0 shares no bin with the others), and an empty block
    sim = build(tmp_path / "t", 2, [2])
    ma.run(sim)
    eh, eng = sim.algorithms[-1], sim.algorithms[0].engine
    n = BINS["n_bins"]
    counts, sums = np.zeros((4, R, n + 4), dtype=np.uint64), np.zeros((4, R, 3, n), dtype=np.int64)
    counts[:, :, 5] = 6                                    # six ladders per block, one snapshot
    counts[1:, 0, 5], counts[1:, 0, 30] = 0, 6
    form = (BINS["lo"], BINS["hi"], n, ALL, X_BOUND)
    eng.set_energy_moments_blocks(*form, counts, sums, 1)
    assert np.all(np.isfinite(eh.reweight_moments(BETAS)["x2"]))
    with pytest.raises(ValueError, match="without block 0 .*no longer connect"):
        eh.reweight_moments(BETAS, error=True)
    counts[:] = 0
    counts[[0, 1, 3], :, 5] = 6
    eng.set_energy_moments_blocks(*form, counts, sums, 1)
    with pytest.raises(ValueError, match="block 2 is empty"):
        eh.reweight_moments(BETAS, error=True)


def test_checkpoint_sections(oracle, tmp_path):
    sched = list(range(2, 21, 2))
    whole = build(tmp_path / "w", 24, sched + [22, 24])
    ma.run(whole)
    first = build(tmp_path / "a", 20, sched)
    ma.run(first)
    fn = ma.checkpoint(first.algorithms[0], str(tmp_path / "ck"))
    d = np.load(fn)
    n = BINS["n_bins"]
    assert np.array_equal(d["emom_blocks"], [4, 2]) and d["emom_block_counts"].shape == (4, R, n + 4)
    assert d["emom_block_sums"].shape == (4, R, 3, n) and d["emom_block_sums"].dtype == np.int64 and int(d["emom_block_snapshots"]) == 10
    assert np.array_equal(d["emom_block_counts"].sum(axis=0, dtype=np.uint64), d["emom_counts"])          # the merged section stays
    assert np.array_equal(d["emom_block_sums"].sum(axis=0), d["emom_sums"]) and "ehist_block_counts" not in d.files
    second = build(tmp_path / "b", 4, [2, 4])
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    a, b = second.algorithms[-1], whole.algorithms[-1]
    assert a.n_snapshots == b.n_snapshots == 12
    assert np.array_equal(a.counts_blocks(), b.counts_blocks()) and np.array_equal(a.moment_sums_blocks(), b.moment_sums_blocks())
    assert [c for c in second.algorithms[0].engine.calls if c[0] == "blocks"] == [("blocks", 4, 2)]
    # another partition is refused; a run without blocks goes on with the merged plain accumulator
    other = build(tmp_path / "c", 4, [2, 4], blocks=2, chunk=2)
    with pytest.raises(ValueError, match="under the partition"):
        ma.restore(other.algorithms[0], str(tmp_path / "ck"))
    plain = build(tmp_path / "d", 4, [2, 4], blocks=None)
    ma.restore(plain.algorithms[0], str(tmp_path / "ck"))
    ma.run(plain)
    p = plain.algorithms[-1]
    assert p.n_snapshots == 12 and np.array_equal(p.counts(), b.counts()) and np.array_equal(p.moment_sums(), b.moment_sums())
    assert plain.algorithms[0].engine.part is None          # (no partition was ever set)
    # a run with blocks cannot resume from a checkpoint that holds merged moments alone
    ma.checkpoint(plain.algorithms[0], str(tmp_path / "ckp"))
    assert "emom_block_counts" not in np.load(tmp_path / "ckp" / "checkpoint_rank0.npz").files
    blocked = build(tmp_path / "e", 4, [2, 4])
    with pytest.raises(ValueError, match="without cells per block"):
        ma.restore(blocked.algorithms[0], str(tmp_path / "ckp"))
