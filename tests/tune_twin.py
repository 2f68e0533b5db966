"""Host twin of tuning the widths per rung (DESIGN.md section 3.13 "Tuning the widths"), written from the DESIGN text in numpy Float64
scalars -- single IEEE operations, nothing contracted; the rule needs no transcendental -- and composed with tests/rung_sigma_twin.py
inside tests/exchange_twin.py for the chains.  It shares no code with the product."""
import numpy as np

import exchange_twin as X
import rung_sigma_twin as RS

OK, FEW_CALLS, INCONSISTENT, CLAMPED = 0, 1, 2, 3


def tune_rule(s, A, T, target=0.44, gamma=1.0, min_calls=1000, lo=1e-100, hi=1e100, inconsistent=False):
    """(status, new width) of one entry: s the width at hand, A and T the accepted and total calls of the window (Python integers)."""
    f = np.float64
    s, target, gamma, lo, hi = f(s), f(target), f(gamma), f(lo), f(hi)
    A, T = int(A), int(T)
    if inconsistent or A > T:
        return INCONSISTENT, s
    if T < int(min_calls):
        return FEW_CALLS, s
    a = f(float(A)) / f(float(T))                # (int -> Float64 rounds to nearest, as the conversion of a 64-bit integer does)
    q = a / target
    q = f(0.5) if q < 0.5 else (f(2.0) if q > 2.0 else q)
    v = s + gamma * ((s * q) - s)
    st = OK
    if v < lo:
        v, st = lo, CLAMPED
    if v > hi:
        v, st = hi, CLAMPED
    return st, v


def harmonic_acceptance(sigma, beta):
    """The acceptance of the Gaussian walk of width sigma on V = x^2 at inverse temperature beta, in equilibrium:
    (2 / pi) atan(c / sigma) with c = sqrt(2 / beta) (DESIGN.md section 3.13 "Tuning the widths")."""
    return (2.0 / np.pi) * np.arctan(np.sqrt(2.0 / np.asarray(beta, dtype=np.float64)) / np.asarray(sigma, dtype=np.float64))


class TuneTwin(X.ExchangeTwin):
    """ExchangeTwin over a RungSigmaTwin, plus the window base, the tuning and its record."""

    def __init__(self, n_chains, table, beta, n_rungs, *, seed, potential="harmonic", chain_offset=0, weight=(1.0,), dtype="f64", **kw):
        self._sim_kw = dict(chain_offset=chain_offset, potential=potential, beta=1.0, weight=weight, seed=seed, dtype=dtype, **kw)
        sim = RS.RungSigmaTwin(n_chains, table, **self._sim_kw)
        sim.set_beta(np.asarray(beta, dtype=np.float64))
        super().__init__(sim, beta, n_rungs, seed=seed, potential=potential, chain_offset=chain_offset, f32=dtype == "f32")
        self.table = np.array(sim.sigma, dtype=np.float64)
        self.K = self.table.shape[0]
        self.base = np.zeros((2, self.K, self.R), dtype=np.int64)
        self.status = np.zeros((self.K, self.R), dtype=np.int64)
        self.n_tuned = 0

    def rung_totals(self):
        acc, tot = self.sim.counters()
        return (np.array([[acc[k, r::self.R].sum() for r in range(self.R)] for k in range(self.K)], dtype=np.int64),
                np.array([[tot[k, r::self.R].sum() for r in range(self.R)] for k in range(self.K)], dtype=np.int64))

    def window_counts(self):
        """(accepted, total, inconsistent)"""
        acc, tot = self.rung_totals()
        bad = (acc < self.base[0]) | (tot < self.base[1])
        return np.where(bad, -1, acc - self.base[0]), np.where(bad, -1, tot - self.base[1]), bad

    def restart(self):
        self.base[0], self.base[1] = self.rung_totals()

    def retable(self, table):
        """The chains go on under another table: new strided sims from the same x, beta, step index; the counters stay."""
        old = self.sim
        x = old.state()[0]
        sim = RS.RungSigmaTwin(old.M, table, **self._sim_kw)
        sim.set_beta(self.beta)
        sim.acc, sim.tot = old.acc, old.tot
        sim.step = old.step
        old.close()
        self.sim, self.state = sim, X._State(sim)
        self.state.put(x, self.pot)
        self.table = np.array(sim.sigma, dtype=np.float64)

    def tune(self, target=0.44, gamma=1.0, min_calls=1000, lo=1e-100, hi=1e100, counts=None):
        """counts: the GLOBAL window (accepted, total), or None for this twin's own.  Returns the status array."""
        if counts is None:
            A, T, bad = self.window_counts()
        else:
            A, T = np.asarray(counts[0]).reshape(self.K, self.R), np.asarray(counts[1]).reshape(self.K, self.R)
            bad = np.zeros((self.K, self.R), dtype=bool)
        new = self.table.copy()
        for k in range(self.K):
            for r in range(self.R):
                self.status[k, r], new[k, r] = tune_rule(self.table[k, r], A[k, r], T[k, r], target, gamma, min_calls, lo, hi, bool(bad[k, r]))
        if np.any((self.status == OK) | (self.status == CLAMPED)):
            self.n_tuned += 1
        self.restart()
        if not np.array_equal(new.view(np.uint64), self.table.view(np.uint64)):
            self.retable(new)
        return self.status.copy()
