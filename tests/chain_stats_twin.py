"""Host twin of the convergence sums (include/amc.h amc_chain_stats_accumulate .. amc_chain_stats_fetch), written
from that text with the oracle's own pieces -- corr_twin.observable for O(x), oracle_lib.xsum_r per strided slice, oracle_lib.xsum_merge
over shards -- and sharing no code with the product.

Per chain i and part p the twin keeps S[p][i] and Q[p][i]; a sample o does S <- S + o and Q <- Q + (o * o), numpy's elementwise
operations on float64 arrays: one IEEE multiplication, then one IEEE addition, nothing contracted.  The columns of group g (the chains
l G + g) are the kind-R sums of
    S0  S[0]   S0S0  S[0] * S[0]   Q0  Q[0]   S1  S[1]   S1S1  S[1] * S[1]   Q1  Q[1]   S0S1  S[0] * S[1]
each a record of xsum_r over the slice of its own group and column: its level is that of its own summands, and a NaN or an infinity
flags its own record alone.
"""
import numpy as np

import oracle_lib as O

import corr_twin as CT
import exchange_twin as X

WORDS = O.XS_WORDS
PARTS, COLS = 2, 7
S0, S0S0, Q0, S1, S1S1, Q1, S0S1 = range(COLS)


class ChainStatsTwin:
    """The sums of M chains in G groups."""

    def __init__(self, n_chains: int, n_groups: int = 1):
        self.G = int(n_groups)
        self.sums = np.zeros((PARTS, 2, int(n_chains)))
        self.n = [0, 0]
        self.observable = 0

    def accumulate(self, kind, values, part: int):
        assert self.observable in (0, CT.OBSERVABLES[kind]) and part in (0, 1)
        o = np.asarray(values, dtype=np.float64)
        with np.errstate(all="ignore"):
            sq = o * o                                     # rounded once ...
            self.sums[part, 0] = self.sums[part, 0] + o
            self.sums[part, 1] = self.sums[part, 1] + sq   # ... then added
        self.n[part] += 1
        self.observable = CT.OBSERVABLES[kind]

    def records(self) -> np.ndarray:
        return records(self.sums, self.G)


def records(sums, n_groups: int = 1) -> np.ndarray:
    """records[G][7][12] from sums[2][2][M], chain i in group i mod G."""
    G = int(n_groups)
    s = np.asarray(sums, dtype=np.float64)
    a, qa, b, qb = (s[p, k].reshape(-1, G) for p in range(PARTS) for k in range(2))
    with np.errstate(all="ignore"):
        cols = [a, a * a, qa, b, b * b, qb, a * b]
    out = np.zeros((G, COLS, WORDS))
    for g in range(G):
        for c in range(COLS):
            out[g, c] = O.xsum_r(np.ascontiguousarray(cols[c][:, g]))
    return out


merge, values = CT.merge, CT.values


# ---- engine doubles with the chain-statistics surface of montecarlo_amd._capi.HipEngine ---------------------------------------------

class ChainStatsSurface:
    """chain_stats_accumulate .. chain_stats_clear computed by this twin over whatever engine double it is mixed into, and a log of
    the accumulate calls with the MH step index each was made at."""

    def _cs_reset(self):
        self._cs = None

    def _cs_groups(self):
        return max(int(getattr(self, "n_rungs", 0) or 0), 1)

    def chain_stats_accumulate(self, kind="energy", part=0):
        if not hasattr(self, "cs_calls"):
            self.cs_calls = []
        x = self.download_state(want_e=False)[0]
        if getattr(self, "_cs", None) is None:
            self._cs = ChainStatsTwin(len(x), self._cs_groups())
        self.cs_calls.append(("accumulate", int(part), self.step))
        self._cs.accumulate(kind, CT.observable(kind, self._cs_potential(), x, self._cs_f32()), int(part))

    def _cs_potential(self):
        return getattr(self, "potential", None) or getattr(self, "_kw", {}).get("potential", "harmonic")

    def _cs_f32(self):
        return bool(getattr(self, "f32", False) or getattr(self, "_kw", {}).get("f32", False))

    def chain_stats_fetch(self):
        self.cs_fetches = getattr(self, "cs_fetches", 0) + 1
        cs = getattr(self, "_cs", None)
        if cs is None:
            return np.zeros((self._cs_groups(), 0, WORDS)), (0, 0), 0
        return cs.records(), (cs.n[0], cs.n[1]), cs.observable

    def chain_stats_counts(self):
        cs = getattr(self, "_cs", None)
        return ((0, 0), 0) if cs is None else ((cs.n[0], cs.n[1]), cs.observable)

    def chain_stats_sums(self):
        return self._cs.sums.copy()

    def set_chain_stats(self, kind=0, n=(0, 0), sums=None):
        if sums is None or not any(int(v) for v in n):
            self._cs = None
            return
        s = np.array(sums, dtype=np.float64).reshape(PARTS, 2, -1)
        self._cs = ChainStatsTwin(s.shape[2], self._cs_groups())
        self._cs.sums, self._cs.n, self._cs.observable = s, [int(n[0]), int(n[1])], CT.OBSERVABLES[kind]

    def chain_stats_clear(self):
        self._cs = None

    def upload_state(self, x, beta=None):
        super().upload_state(x, beta)
        self._cs = None

    def init_uniform(self, lo, hi):
        super().init_uniform(lo, hi)
        self._cs = None


class ChainStatsTwinEngine(ChainStatsSurface, CT.CorrTwinEngine):
    """No ladder (one group); anneals (the annealing leaves the sums alone, as the engine does)."""


class ChainStatsLadderEngine(ChainStatsSurface, X.TwinEngine):
    """With the exchange surface: one group per rung."""

    def set_ladder(self, n_rungs):
        super().set_ladder(n_rungs)
        self._cs = None
