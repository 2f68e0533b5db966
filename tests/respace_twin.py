"""Host twin of the ladder respacing (DESIGN.md section 3.13 "Respacing"), beside the twins of the exchange step and of walker
tracking (exchange_twin.py, track_twin.py).

Written from the DESIGN text in numpy Float64 scalars: every + - * / and sqrt below is one IEEE operation on np.float64, in the order
the text gives, nothing contracted.  ``respace_rule`` is the rule; ``RespaceTwin`` wraps TrackTwin and applies what a status-0
respacing does to a handle.  It shares no code with the product."""
import numpy as np

import track_twin as T

ACCEPTANCE, FLOW = "acceptance", "flow"
F = np.float64


def respace_rule(rule, b, counts, gamma=1.0, eps=0.0):
    """(status, out): b the R beta values (Float64), counts the GLOBAL integers -- "acceptance": (attempted[R - 1], accepted[R - 1]);
    "flow": n[R][3].  out is None unless status == 0."""
    b = [F(v) for v in np.asarray(b, dtype=np.float64)]
    R = len(b)
    gamma, eps = F(gamma), F(eps)
    with np.errstate(all="ignore"):
        if rule == ACCEPTANCE:
            att, acc = (np.asarray(c, dtype=np.int64) for c in counts)
            if np.any(att[:R - 1] == 0):
                return 2, None
            w = [F(int(att[j]) - int(acc[j])) / F(int(att[j])) for j in range(R - 1)]
        elif rule == FLOW:
            n = np.asarray(counts, dtype=np.int64).reshape(R, 3)
            if np.any(n[:, 1] + n[:, 2] == 0):
                return 2, None
            f = [F(int(n[r, 1])) / F(int(n[r, 1]) + int(n[r, 2])) for r in range(R)]
            w = []
            for j in range(R - 1):
                d = f[j] - f[j + 1]
                w.append(np.sqrt(d if d > 0 else F(0.0)))
        else:
            raise ValueError(rule)
        up = b[1] > b[0]

        def monotone(v):
            return all(np.isfinite(x) for x in v) and all((v[r + 1] > v[r]) if up else (v[r + 1] < v[r]) for r in range(R - 1))
        if not monotone(b):
            return 3, None
        W = F(0.0)
        for j in range(R - 1):
            W = W + w[j]
        if not (W > 0) or not np.isfinite(W):
            return 1, None
        m = (eps * W) / F(R - 1)
        wf = [m if w[j] < m else w[j] for j in range(R - 1)]
        G = [F(0.0)]
        for j in range(R - 1):
            G.append(G[j] + wf[j])
        out = list(b)
        for k in range(1, R - 1):
            t = (F(k) * G[R - 1]) / F(R - 1)
            j = next((i for i in range(R - 1) if G[i + 1] > t), R - 2)
            frac = (t - G[j]) / wf[j]
            nb = b[j] + (b[j + 1] - b[j]) * frac
            out[k] = b[k] + gamma * (nb - b[k])
        if not monotone(out):
            return 4, None
    assert all(type(v) is np.float64 for v in out)
    return 0, np.array(out, dtype=np.float64)


class RespaceTwin(T.TrackTwin):
    """TrackTwin with respace(): the rule on this twin's own counts (or the counts given), and the effects of status 0 -- beta of
    every chain (rounded once for Float32 state), the gap counters zeroed, with tracking the labels and the trip counters reset."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.status, self.n_respaced = 0, 0

    def ladder(self):
        return self.beta[:self.R].copy()

    def respace(self, rule, gamma=1.0, eps=0.0, counts=None):
        if counts is None:
            counts = (self.attempted, self.accepted) if rule == ACCEPTANCE else self.flow_rungs()
        self.status, out = respace_rule(rule, self.ladder(), counts, gamma, eps)
        if self.status != 0:
            return self.status
        if self.f32:
            out = out.astype(np.float32).astype(np.float64)
        self.beta = np.tile(out, self.beta.size // self.R)
        _set_sim_beta(self.state.sim, self.beta)
        self.accepted[:] = 0
        self.attempted[:] = 0
        if self.lab is not None:
            self.set_tracking(True)
        self.n_respaced += 1
        return 0


def _set_sim_beta(sim, beta):
    """The per-chain beta of the simulation object the sweeps run on: oracle_lib.OracleSim (set_beta) or f32_param_twin.TwinSim."""
    if hasattr(sim, "set_beta"):
        sim.set_beta(beta)
    else:
        sim.beta[:] = beta.astype(np.float32)
