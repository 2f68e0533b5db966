"""Host twin of the bridge sums (DESIGN.md section 3.13 "Bridge sums"; include/amc.h amc_bridge_accumulate .. amc_set_bridge), written
from that text with the oracle's own pieces -- amo_potential / amo_potential_f32, amo_exp, oracle_lib.xsum_r per strided slice,
oracle_lib.xsum_merge over snapshots and shards -- and sharing no code with the product.

For chain c = l R + r, e = potential_T(x_c) in the state type T and beta the per-chain array (T):
    E   double(e)                                   EE  fl(double(e) * double(e))
    WF  exp(double((-e) * (beta_(c+1) - beta_c)))   MF  min(1, WF), a NaN stays a NaN       r + 1 < R
    WB  exp(double((-e) * (beta_(c-1) - beta_c)))   MB  min(1, WB)                          r >= 1
Numpy's elementwise * and - on float64 / float32 arrays are single IEEE operations: nothing is contracted.  A record is xsum_r over
the slice of one rung and column; WF, MF at rung R - 1, WB, MB at rung 0 and every column outside the mask are all-zero records.
"""
import numpy as np

import oracle_lib as O

WORDS = O.XS_WORDS
E, EE, WF, WB, MF, MB, ALL = 1, 2, 4, 8, 16, 32, 63
ACCEPTANCE_SET = E | EE | MF | MB
COLS = 6


def energies(potential, x, f32: bool = False) -> np.ndarray:
    """double(potential_T(x)) per chain (built-in potentials, or whatever oracle_lib.install_custom_potential installed)."""
    lib, pot = O.load(), O._potential_id(potential)
    if f32:
        return np.array([lib.amo_potential_f32(pot, float(np.float32(v))) for v in np.asarray(x, dtype=np.float64)], dtype=np.float64)
    return np.array([lib.amo_potential(pot, float(v)) for v in np.asarray(x, dtype=np.float64)], dtype=np.float64)


def _exp(a) -> np.ndarray:
    lib = O.load()
    flat = np.asarray(a, dtype=np.float64).reshape(-1)
    return np.array([lib.amo_exp(float(v)) for v in flat], dtype=np.float64).reshape(np.shape(a))


def _min_one(w) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(w), w, np.minimum(1.0, w))


def summands(e, beta, n_rungs: int, f32: bool = False):
    """The six columns' summands as arrays of shape (L, R), NaN-free only where a slot has a summand: the caller slices by rung.
    ``e``: the energies in the state type (as Float64 values), ``beta``: the per-chain array."""
    R = int(n_rungs)
    T = np.float32 if f32 else np.float64
    eT = np.asarray(e, dtype=np.float64).astype(T).reshape(-1, R)
    bT = np.asarray(beta, dtype=np.float64).astype(T).reshape(-1, R)
    L = eT.shape[0]
    with np.errstate(all="ignore"):
        ed = eT.astype(np.float64)
        ee = ed * ed
        ne = -eT
        d_f = bT[:, 1:] - bT[:, :-1]                  # rung r < R - 1: beta_(c+1) - beta_c
        a_f = ne[:, :-1] * d_f
        d_b = bT[:, :-1] - bT[:, 1:]                  # rung r >= 1: beta_(c-1) - beta_c
        a_b = ne[:, 1:] * d_b
    assert a_f.dtype == T and a_b.dtype == T
    wf, wb = np.zeros((L, R)), np.zeros((L, R))
    wf[:, :-1] = _exp(a_f.astype(np.float64))
    wb[:, 1:] = _exp(a_b.astype(np.float64))
    return [ed, ee, wf, wb, _min_one(wf), _min_one(wb)]


def has_summand(c: int, r: int, n_rungs: int) -> bool:
    """Column index c (0 E, 1 EE, 2 WF, 3 WB, 4 MF, 5 MB) has a summand at rung r."""
    if c in (2, 4):
        return r + 1 < n_rungs
    if c in (3, 5):
        return r >= 1
    return True


def records(e, beta, n_rungs: int, columns: int = ALL, f32: bool = False) -> np.ndarray:
    """records[R][6][12] of one snapshot of whole ladders."""
    R = int(n_rungs)
    cols = summands(e, beta, R, f32)
    out = np.zeros((R, COLS, WORDS))
    for r in range(R):
        for c in range(COLS):
            if (columns >> c) & 1 and has_summand(c, r, R):
                out[r, c] = O.xsum_r(np.ascontiguousarray(cols[c][:, r]))
    return out


def merge(parts) -> np.ndarray:
    """Snapshots' or shards' records merged (integers: any order); an all-zero record merges as nothing."""
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    tot = parts[0].reshape(-1, WORDS).copy()
    for p in parts[1:]:
        q = p.reshape(-1, WORDS)
        for i in range(tot.shape[0]):
            if not q[i].any():
                continue
            tot[i] = q[i] if not tot[i].any() else O.xsum_merge(tot[i], q[i])[0]
    return tot.reshape(parts[0].shape)


def values(rec) -> np.ndarray:
    """The Float64 of every record, shape (R, 6); an all-zero record reads 0."""
    rec = np.asarray(rec, dtype=np.float64)
    return O.xsum_round(rec.reshape(-1, WORDS)).reshape(rec.shape[:-1])


# ---- the estimators (montecarlo_amd/exchange.py ReplicaExchange.log_z_ratios / heat_capacity), restated -------------------------------
def log_z_acceptance(rec) -> np.ndarray:
    """log(Z_(r+1) / Z_r) by Bennett's identity with the Metropolis function at C = 0: log S_MF[r] - log S_MB[r + 1]."""
    v = values(rec)
    with np.errstate(all="ignore"):
        return np.log(v[:-1, 4]) - np.log(v[1:, 5])


def log_z_exponential(rec, n: float) -> np.ndarray:
    v = values(rec)
    with np.errstate(all="ignore"):
        return np.stack([np.log(v[:-1, 2] / n), -np.log(v[1:, 3] / n)])


def log_z_ti(rec, n: float, betas) -> np.ndarray:
    v = values(rec)
    b = np.asarray(betas, dtype=np.float64)
    m = v[:, 0] / n
    return -0.5 * (m[:-1] + m[1:]) * (b[1:] - b[:-1])


def heat_capacity(rec, n: float, betas) -> np.ndarray:
    v = values(rec)
    b = np.asarray(betas, dtype=np.float64)
    m, m2 = v[:, 0] / n, v[:, 1] / n
    return b * b * (m2 - m * m)
