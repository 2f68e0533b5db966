"""Host twin of proposal widths per rung (DESIGN.md section 3.13 "Widths per rung"): a simulation object with OracleSim's interface
made of R OracleSims over the whole shard.  Sim r has the pool sigma_k = sigma[k][r]; a sweep call runs on all R from the same x and
step index, and chain c is taken from sim (offset + c) mod R -- the Philox counter is keyed by global chain id and step, so that IS
chain c stepped with the widths of its rung.  Plugs into exchange_twin.ExchangeTwin where an OracleSim goes.
ArrayExchangeTwin is that ExchangeTwin with the exchange step written over arrays, for the statistical run at 4096 ladders."""
import numpy as np

import exchange_twin as X
import oracle_lib as O


class RungSigmaTwin:
    def __init__(self, n_chains, rung_sigma, *, chain_offset=0, weight=(1.0,), threads=1, **kw):
        self.threads = int(threads)                # of every sweep call (the results do not depend on it)
        self.sigma = np.array(rung_sigma, dtype=np.float64)
        if self.sigma.ndim == 1:
            self.sigma = self.sigma.reshape(1, -1)
        self.K, self.R = self.sigma.shape
        self.M, self.offset = int(n_chains), int(chain_offset)
        self.sims = [O.OracleSim(self.M, chain_offset=self.offset, sigma=[float(s) for s in self.sigma[:, r]], weight=weight, **kw)
                     for r in range(self.R)]
        self.rung = (self.offset + np.arange(self.M)) % self.R
        self.acc = np.zeros((self.K, self.M), dtype=np.int64)
        self.tot = np.zeros((self.K, self.M), dtype=np.int64)

    def set_x(self, x):
        for s in self.sims:
            s.set_x(x)

    def set_beta(self, b):
        for s in self.sims:
            s.set_beta(b)

    def state(self):
        x, e = np.empty(self.M), np.empty(self.M)
        for r, s in enumerate(self.sims):
            xs, es = s.state()
            mine = self.rung == r
            x[mine], e[mine] = xs[mine], es[mine]
        return x, e

    def counters(self):
        return self.acc.copy(), self.tot.copy()

    def make_steps(self, n=1, threads=None):
        threads = threads or self.threads
        before = [s.counters() for s in self.sims]
        for s in self.sims:
            s.make_steps(n, threads)
        for r, s in enumerate(self.sims):
            a, t = s.counters()
            mine = self.rung == r
            self.acc[:, mine] += (a - before[r][0])[:, mine]
            self.tot[:, mine] += (t - before[r][1])[:, mine]
        self.set_x(self.state()[0])            # every sim goes on from the chains as their own rungs left them

    @property
    def step(self):
        return self.sims[0].step

    @step.setter
    def step(self, t):
        for s in self.sims:
            s.step = t

    def close(self):
        for s in self.sims:
            s.close()


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """oracle/amc_oracle.c amo_philox4x32_10 over numpy arrays of counters (uint64 arrays holding 32-bit words)."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & m32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


class ArrayExchangeTwin(X.ExchangeTwin):
    """ExchangeTwin whose exchange step works on all ladders at once in numpy, for ensembles where a Python loop over the ladders
    takes minutes: built-in potentials, Float64 state.  The same draws (Philox counter of amo_counter, amo_uniform_co's 52 bits) and
    the same order of operations in delta; exp is numpy's, which may differ from amo_exp in the last bit, so a decision can differ
    from ExchangeTwin's only where exp(delta) and u agree to that bit."""

    def exchange(self, n=1):
        assert not self.f32 and self.pot in (O.POTENTIALS["harmonic"], O.POTENTIALS["double_well"])
        key = self.seed & 0xFFFFFFFFFFFFFFFF
        for _ in range(int(n)):
            x = self.state.get()
            for r in X.gaps_of_step(self.R, self.t_x):
                a = np.arange(r, x.size, self.R)
                g, t = (self.offset + a).astype(np.uint64), self.t_x
                w = philox4x32_10(np.full(a.size, t & 0xFFFFFFFF), np.full(a.size, ((t >> 32) & 0xFFFF) | (X.STREAM_EXCHANGE << 28)),
                                  g, g >> np.uint64(32), key & 0xFFFFFFFF, key >> 32)
                u = ((((w[1] << np.uint64(32)) | w[0]) >> np.uint64(12)) | np.uint64(0x3FF0000000000000)).view(np.float64) - 1.0
                xa, xb = x[a], x[a + 1]
                if self.pot == O.POTENTIALS["harmonic"]:
                    ea, eb = xa * xa, xb * xb
                else:
                    qa, qb = xa * xa - 1.0, xb * xb - 1.0
                    ea, eb = qa * qa, qb * qb
                ba, bb = self.beta[a], self.beta[a + 1]
                with np.errstate(all="ignore"):
                    delta = (((-eb) * ba) + ((-ea) * bb)) - (((-ea) * ba) + ((-eb) * bb))
                    ex = np.exp(delta)
                    yes = np.where(np.isnan(ex), False, np.minimum(1.0, ex) > u)
                x[a], x[a + 1] = np.where(yes, xb, xa), np.where(yes, xa, xb)
                self.attempted[r] += a.size
                self.accepted[r] += int(yes.sum())
            self.state.put(x, self.pot)
            self.t_x += 1
