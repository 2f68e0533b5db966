"""Host twin of the replica-exchange step, beside the oracle (oracle/ itself knows no exchange move).

Written from the DESIGN text with the oracle's own primitives -- amo_counter, amo_philox4x32_10, amo_uniform_co, amo_exp,
amo_potential (amo_potential_f32 and numpy float32 operations for Float32 state) -- over any simulation object of the tests:
oracle_lib.OracleSim / OracleEngine (Float64 or Float32 state) and f32_param_twin.TwinSim (the all-Float32 model).  It shares no
code with the product.  Numpy's elementwise * + - on float64 / float32 scalars are single IEEE operations: nothing is contracted.
"""
import numpy as np

import oracle_lib as O

STREAM_EXCHANGE = 3


def gaps_of_step(n_rungs: int, step: int):
    """The gaps r attempted in every ladder at exchange step `step`: r mod 2 == step mod 2 and r + 1 < R."""
    return [r for r in range(n_rungs - 1) if r % 2 == step % 2]


def draw_uniform(seed: int, chain_a: int, step: int) -> float:
    """u of gap (a, a + 1): uniform_co(w.x, w.y), w = Philox4x32-10 of draw (id = global id of chain a, t = step, draw 0, stream 3)."""
    w = O.draw_words(int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_a), int(step), 0, STREAM_EXCHANGE)
    return float(O.load().amo_uniform_co(w[0], w[1]))


def swap_decision(pot: int, xa, xb, beta_a, beta_b, u: float, f32: bool = False) -> bool:
    """accept iff min(1, exp(delta)) > u with delta = (((-e_b) beta_a) + ((-e_a) beta_b)) - (((-e_a) beta_a) + ((-e_b) beta_b)) in the state's
    type, exp and u Float64; Julia's min keeps a NaN, and a NaN rejects."""
    lib = O.load()
    if f32:
        T = np.float32
        ea, eb = T(lib.amo_potential_f32(pot, float(T(xa)))), T(lib.amo_potential_f32(pot, float(T(xb))))
    else:
        T = np.float64
        ea, eb = T(lib.amo_potential(pot, float(xa))), T(lib.amo_potential(pot, float(xb)))
    ba, bb = T(beta_a), T(beta_b)
    with np.errstate(all="ignore"):
        nea, neb = -ea, -eb
        delta = ((neb * ba) + (nea * bb)) - ((nea * ba) + (neb * bb))
    assert delta.dtype == T
    ex = float(lib.amo_exp(float(delta)))
    alpha = ex if ex != ex else min(1.0, ex)
    return alpha > u


class _State:
    """x of a simulation object as a Float64 array, and the way back (e follows: e == potential(x) on this path)."""

    def __init__(self, sim):
        self.sim = getattr(sim, "sim", sim)            # OracleEngine wraps an OracleSim
        self.twin32 = not hasattr(self.sim, "set_x")   # f32_param_twin.TwinSim keeps numpy float32 arrays

    def get(self):
        if self.twin32:
            return self.sim.x.astype(np.float64)
        return self.sim.state()[0]

    def put(self, x, pot):
        if self.twin32:
            lib = O.load()
            self.sim.x[:] = x.astype(np.float32)
            self.sim.e[:] = [lib.amo_potential_f32(pot, float(v)) for v in self.sim.x]
        else:
            self.sim.set_x(x)          # recomputes e = potential(x) in the simulation's type; the bits of x are kept


class ExchangeTwin:
    """The ladder state beside a simulation object: exchange step index, gap counters, and exchange() / sweep() / sweep_exchange()."""

    def __init__(self, sim, beta, n_rungs: int, *, seed: int, potential="harmonic", chain_offset: int = 0, f32: bool = False):
        self.sim, self.state = sim, _State(sim)
        self.R = int(n_rungs)
        self.f32 = bool(f32)
        self.beta = np.asarray(beta, dtype=np.float64).copy()
        if self.f32:
            self.beta = self.beta.astype(np.float32).astype(np.float64)       # Particle{Float32}.beta
        assert self.beta.size % self.R == 0 and chain_offset % self.R == 0
        self.offset, self.seed = int(chain_offset), int(seed)
        self.pot = O._potential_id(potential)
        self.t_x = 0
        self.accepted = np.zeros(self.R - 1, dtype=np.int64)
        self.attempted = np.zeros(self.R - 1, dtype=np.int64)

    def exchange(self, n: int = 1):
        for _ in range(int(n)):
            x = self.state.get()
            for r in gaps_of_step(self.R, self.t_x):
                for a in range(r, x.size, self.R):
                    u = draw_uniform(self.seed, self.offset + a, self.t_x)
                    self.attempted[r] += 1
                    if swap_decision(self.pot, x[a], x[a + 1], self.beta[a], self.beta[a + 1], u, self.f32):
                        x[a], x[a + 1] = x[a + 1], x[a]
                        self.accepted[r] += 1
                        self._swapped(a, r)
            self.state.put(x, self.pot)
            self.t_x += 1

    def _swapped(self, a: int, r: int):
        """Called once per accepted swap of gap r, after x[a] and x[a + 1] have changed places (track_twin.TrackTwin: the labels)."""

    def sweep(self, n: int = 1):
        s = self.sim
        (s.sweep if hasattr(s, "sweep") else s.make_steps)(int(n))

    def sweep_exchange(self, n_rounds: int, sweeps_per_round: int = 1):
        for _ in range(int(n_rounds)):
            self.sweep(sweeps_per_round)
            self.exchange(1)

    def counters(self):
        return self.accepted.copy(), self.attempted.copy()


class TwinEngine(O.OracleEngine):
    """oracle_lib.OracleEngine with the exchange surface of montecarlo_amd._capi.HipEngine, computed by ExchangeTwin: the engine
    double of the host-logic tests (Metropolis(engine_factory=TwinEngine))."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self._kw = dict(seed=kw.get("seed", 1), potential=kw.get("potential", "harmonic"), chain_offset=kw.get("chain_offset", 0),
                        f32=kw.get("dtype", "f64") == "f32")
        self._beta = None
        self.twin = None

    def upload_state(self, x, beta=None):
        super().upload_state(x, beta)
        if beta is not None:
            self._beta = np.array(beta, dtype=np.float64)

    def set_ladder(self, n_rungs):
        assert self._beta is not None, "a ladder needs a per-chain beta array"
        self.twin = ExchangeTwin(self, self._beta, n_rungs, **self._kw)
        self.n_rungs = int(n_rungs)

    def exchange(self, n_steps=1):
        self.twin.exchange(n_steps)

    def sweep_exchange(self, n_rounds, sweeps_per_round=1):
        self.twin.sweep_exchange(n_rounds, sweeps_per_round)

    def exchange_counters(self):
        return self.twin.counters()

    def set_exchange_counters(self, accepted, attempted):
        self.twin.accepted[:] = np.asarray(accepted, dtype=np.int64)
        self.twin.attempted[:] = np.asarray(attempted, dtype=np.int64)

    @property
    def exchange_step(self):
        return self.twin.t_x

    @exchange_step.setter
    def exchange_step(self, t):
        self.twin.t_x = int(t)
