"""Host twin of the time correlation (include/amc.h amc_corr_mark .. amc_corr_fetch), written from that text
with the oracle's own pieces -- amo_potential / amo_potential_f32 through bridge_twin.energies, oracle_lib.xsum_r per strided slice,
oracle_lib.xsum_merge over shards and origins -- and sharing no code with the product.

With a_i = O(x_i) at the mark and o_i = O(x_i) at a sample, O(x) = double(potential_T(x)) ("energy") or double(x) ("x"), the columns of
group g (the chains l G + g) are the kind-R sums of
    O   o_i          OO  fl(o_i * o_i)          AO  fl(a_i * o_i)
Numpy's elementwise * on float64 arrays is one IEEE multiplication: nothing is contracted.  A record is xsum_r over the slice of one
group and column, so its level is that of its own summands and a NaN or an infinity flags its own record alone.
"""
import numpy as np

import oracle_lib as O

import anneal_twin as A
import bridge_twin as B

WORDS = O.XS_WORDS
COLS = 3
E, X = 1, 2
OBSERVABLES = {"energy": E, "x": X, E: E, X: X}


def observable(kind, potential, x, f32: bool = False) -> np.ndarray:
    """O(x) per chain as Float64; ``x``: the positions as download_state returns them (exact images of the state type's values)."""
    if OBSERVABLES[kind] == X:
        return np.asarray(x, dtype=np.float64).copy()
    return B.energies(potential, x, f32)


def sample_records(origin, values, n_groups: int = 1) -> np.ndarray:
    """records[G][3][12] of one sample: ``origin`` = a, ``values`` = o, chain i in group i mod G."""
    G = int(n_groups)
    a = np.asarray(origin, dtype=np.float64).reshape(-1, G)
    o = np.asarray(values, dtype=np.float64).reshape(-1, G)
    with np.errstate(all="ignore"):
        cols = [o, o * o, a * o]
    out = np.zeros((G, COLS, WORDS))
    for g in range(G):
        for c in range(COLS):
            out[g, c] = O.xsum_r(np.ascontiguousarray(cols[c][:, g]))
    return out


def records(series, n_groups: int = 1) -> np.ndarray:
    """records[S][G][3][12] of a mark and its samples: ``series[0]`` the observable at the mark (sample 0), ``series[s]`` at sample s."""
    return np.stack([sample_records(series[0], s, n_groups) for s in series])


def merge(parts) -> np.ndarray:
    """Shards' or origins' records merged record by record (integers: any order)."""
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    tot = parts[0].reshape(-1, WORDS).copy()
    for p in parts[1:]:
        tot = O.xsum_merge(tot, p.reshape(-1, WORDS))
    return tot.reshape(parts[0].shape)


def values(rec) -> np.ndarray:
    """The Float64 of every record."""
    rec = np.asarray(rec, dtype=np.float64)
    return O.xsum_round(rec.reshape(-1, WORDS)).reshape(rec.shape[:-1])


# ---- an engine double with the time-correlation surface of montecarlo_amd._capi.HipEngine (no ladder: one group) ---------------------

class CorrTwinEngine(A.AnnealTwinEngine):
    """anneal_twin.AnnealTwinEngine plus corr_mark .. corr_clear computed by this twin, and a log of those calls with the MH step index
    each was made at: the engine double of the host-logic tests (Metropolis(engine_factory=CorrTwinEngine))."""

    MAX_LAGS = 256

    def __init__(self, **kw):
        super().__init__(**kw)
        self.potential = kw.get("potential", "harmonic")
        self.f32 = kw.get("dtype", "f64") == "f32"
        self.calls = []
        self._corr = None                 # dict(observable, origin, records [S][1][3][12], steps)

    def _observe(self, kind):
        return observable(kind, self.potential, self.download_state(want_e=False)[0], self.f32)

    def corr_mark(self, kind="energy"):
        self.calls.append(("mark", self.step))
        a = self._observe(kind)
        self._corr = dict(observable=OBSERVABLES[kind], origin=a, records=[sample_records(a, a)], steps=[self.step])

    def corr_sample(self):
        assert self._corr is not None and len(self._corr["steps"]) < self.MAX_LAGS
        self.calls.append(("sample", self.step))
        self._corr["records"].append(sample_records(self._corr["origin"], self._observe(self._corr["observable"])))
        self._corr["steps"].append(self.step)

    def corr_fetch(self):
        self.calls.append(("fetch", self.step))
        if self._corr is None:
            return np.zeros((0, 1, COLS, WORDS)), np.zeros(0, dtype=np.uint64), 0
        return np.stack(self._corr["records"]), np.array(self._corr["steps"], dtype=np.uint64), self._corr["observable"]

    def corr_origin(self):
        return self._corr["origin"].copy()

    def set_corr(self, kind, origin, records, steps):
        rec = np.asarray(records, dtype=np.float64).reshape(-1, 1, COLS, WORDS)
        self._corr = dict(observable=OBSERVABLES[kind], origin=np.array(origin, dtype=np.float64), records=list(rec),
                          steps=[int(s) for s in steps])

    def corr_clear(self):
        self.calls.append(("clear", self.step))
        self._corr = None

    def upload_state(self, x, beta=None):
        super().upload_state(x, beta)
        self._corr = None

    def anneal(self, beta_new):
        super().anneal(beta_new)
        self._corr = None
