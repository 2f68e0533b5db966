"""Host twin of the population-annealing step, beside the oracle (oracle/ itself knows no annealing).

Written from the DESIGN text with the oracle's own primitives -- amo_potential (amo_potential_f32 and numpy float32 operations for
Float32 state), amo_exp, draw_words -- and Python integers for everything that crosses chains (the weights, their prefix, the 128-bit
comparisons of the systematic resampling).  It sits over oracle_lib.OracleSim like exchange_twin.ExchangeTwin and shares no code with
the product.  Numpy's elementwise * - on float64 / float32 scalars are single IEEE operations: nothing is contracted.
"""
import math
import struct

import numpy as np

import oracle_lib as O

STREAM_ANNEAL = 4
WEIGHT_BITS = 30
MAX_RECORDS = 4096
OK, ALL_NAN, INF, NO_WEIGHT = 0, 1, 2, 3


def f64_bits(v: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def bits_f64(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


def order_key(a: float) -> int:
    """A non-NaN Float64 as an integer whose order is the order of the values, -0 below +0."""
    b = f64_bits(a)
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def log_weights(pot: int, x, beta_from: float, beta_to: float, f32: bool):
    """a_i = Float64((-e_i) * delta), e_i = potential(x_i) and delta = T(beta_to) - T(beta_from), the product in T."""
    lib = O.load()
    T = np.float32 if f32 else np.float64
    with np.errstate(all="ignore"):
        delta = T(beta_to) - T(beta_from)
        out = []
        for v in x:
            e = T(lib.amo_potential_f32(pot, float(T(v)))) if f32 else T(lib.amo_potential(pot, float(v)))
            p = (-e) * delta
            assert p.dtype == T
            out.append(float(p))
    return out


def offset_draw(seed: int, t_a: int) -> int:
    """omega = w.x | (w.y << 32), w = Philox4x32-10 of draw (id 0, t = t_a, draw 0, stream 4)."""
    w = O.draw_words(int(seed) & 0xFFFFFFFFFFFFFFFF, 0, int(t_a), 0, STREAM_ANNEAL)
    return w[0] | (w[1] << 32)


def resample(a, seed: int, t_a: int):
    """(status, a_max bits, W, T_w, U, parents): the integer part of the step from the log-weights.  parents is None unless status == OK."""
    lib = O.load()
    M = len(a)
    keyed = [(order_key(v), v) for v in a if v == v]
    if not keyed:
        return ALL_NAN, 0x7FF8000000000000, None, 0, 0, None
    a_max = max(keyed)[1]                         # the maximum in the order of the keys: -0 below +0
    if a_max == math.inf:
        return INF, f64_bits(a_max), None, 0, 0, None
    if a_max == -math.inf:
        return NO_WEIGHT, f64_bits(a_max), None, 0, 0, None
    W = [0 if (v != v or v == -math.inf) else int(math.floor(2.0 ** WEIGHT_BITS * lib.amo_exp(v - a_max))) for v in a]
    T_w = sum(W)
    U = (offset_draw(seed, t_a) * T_w) >> 64
    assert 0 <= U < T_w
    parents, i, C = [], 0, W[0]                   # C = C_i, the inclusive prefix
    for j in range(M):
        while not (j * T_w + U < C * M):          # both sides exact integers
            i += 1
            C += W[i]
        parents.append(i)
    return OK, f64_bits(a_max), W, T_w, U, parents


class AnnealTwin:
    """The annealing state beside an OracleSim that runs at one shared beta: the annealing step index, the records, the families, and
    anneal() / sweep()."""

    def __init__(self, sim, beta: float, *, seed: int, potential="harmonic", f32: bool = False, families: bool = False):
        self.sim = sim
        self.M = sim.M
        self.beta = float(beta)
        self.seed = int(seed)
        self.f32 = bool(f32)
        self.pot = O._potential_id(potential)
        self.t_a = 0
        self.records = []
        self.fam = np.arange(self.M, dtype=np.uint32) if families else None

    def x(self):
        return self.sim.state()[0]

    def anneal(self, beta_new: float):
        assert len(self.records) < MAX_RECORDS
        beta_new = float(beta_new)
        x = self.x()
        a = log_weights(self.pot, x, self.beta, beta_new, self.f32)
        status, amax_bits, W, T_w, U, parents = resample(a, self.seed, self.t_a)
        n_parents = max_children = 0
        if status == OK:
            p = np.asarray(parents, dtype=np.int64)
            counts = np.bincount(p, minlength=self.M)
            n_parents, max_children = int((counts > 0).sum()), int(counts.max())
            self.sim.set_x(x[p])                 # recomputes e = potential(x) in the simulation's type; the bits of x are kept
            if self.fam is not None:
                self.fam = self.fam[p]
            self.last = dict(W=W, counts=counts, parents=p)
        self.records.append([status, f64_bits(self.beta), f64_bits(beta_new), amax_bits, T_w, U, n_parents, max_children])
        self.beta = beta_new
        b = np.float64(np.float32(beta_new)) if self.f32 else beta_new
        self.sim.set_beta(np.full(self.M, b))
        self.t_a += 1

    def sweep(self, n: int = 1):
        self.sim.make_steps(int(n))

    def records_array(self):
        return np.array(self.records, dtype=np.uint64).reshape(-1, 8)

    def family_stats(self):
        n = np.bincount(self.fam, minlength=self.M).astype(object)
        return int((n > 0).sum()), int((n * n).sum()), int(n.max())


def log_z_ratios(records, M: int):
    """log(Z(beta_to) / Z(beta_from)) per record: a_max + log T_w - log M - 30 log 2 (NaN for a step that did not resample)."""
    out = []
    for r in np.asarray(records, dtype=np.uint64).reshape(-1, 8):
        out.append(bits_f64(int(r[3])) + math.log(int(r[4])) - math.log(M) - WEIGHT_BITS * math.log(2.0) if int(r[0]) == OK else math.nan)
    return np.array(out)


class AnnealTwinEngine(O.OracleEngine):
    """oracle_lib.OracleEngine with the annealing surface of montecarlo_amd._capi.HipEngine, computed by AnnealTwin: the engine double
    of the host-logic tests (Metropolis(engine_factory=AnnealTwinEngine))."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.whole = kw.get("chain_offset", 0) == 0 and kw.get("n_chains_global") in (None, kw["n_chains"])
        self.twin = AnnealTwin(self.sim, kw.get("beta", 1.0), seed=kw.get("seed", 1), potential=kw.get("potential", "harmonic"),
                               f32=kw.get("dtype", "f64") == "f32")
        self._drained = 0

    def anneal(self, beta_new):
        assert self.whole, "the handle does not hold the whole ensemble"
        self.twin.anneal(beta_new)

    def anneal_records(self, reset=False):
        out = self.twin.records_array()[self._drained:]
        if reset:
            self._drained = len(self.twin.records)
        return out

    def set_anneal_records(self, records):
        rec = np.asarray(records, dtype=np.uint64).reshape(-1, 8)
        self.twin.records = [list(map(int, r)) for r in rec]
        self._drained = 0

    @property
    def anneal_step(self):
        return self.twin.t_a

    @anneal_step.setter
    def anneal_step(self, t):
        self.twin.t_a = int(t)

    @property
    def beta(self):
        return self.twin.beta

    @beta.setter
    def beta(self, b):
        self.twin.beta = float(b)
        self.sim.set_beta(np.full(self.n_chains, np.float64(np.float32(b)) if self.twin.f32 else float(b)))

    def set_anneal_families(self, on=True):
        self.twin.fam = np.arange(self.n_chains, dtype=np.uint32) if on else None

    def anneal_family_stats(self):
        return self.twin.family_stats()

    def download_families(self):
        return self.twin.fam.copy()

    def upload_families(self, families):
        self.twin.fam = np.asarray(families, dtype=np.uint32).copy()
