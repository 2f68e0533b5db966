"""Host twin of walker tracking (DESIGN.md section 3.13 "Walker tracking"), beside the twin of the exchange step (exchange_twin.py).

Written from the DESIGN text: one label per local chain, lab = w | (d << 6); an accepted swap of gap r exchanges the two labels along
with x, then the label now at rung 0 (r == 0) or at rung R - 1 (r + 1 == R - 1) counts a trip when it last visited the other end and
takes the direction of the end it arrived at.  The step and its decision are ExchangeTwin's; TrackTwin fills in its per-swap hook.
It shares no code with the product."""
import numpy as np

import exchange_twin as X

UP, DOWN = 1, 2


def initial_labels(n_chains: int, n_rungs: int) -> np.ndarray:
    r = np.arange(n_chains) % n_rungs
    d = np.where(r == 0, UP, np.where(r == n_rungs - 1, DOWN, 0))
    return (r | (d << 6)).astype(np.uint8)


def flow_counts(lab: np.ndarray, n_rungs: int) -> np.ndarray:
    """n[r][d]: chains at rung r whose label has direction d -- a pure function of the labels."""
    n = np.zeros((n_rungs, 3), dtype=np.int64)
    np.add.at(n, (np.arange(lab.size) % n_rungs, lab.astype(np.int64) >> 6), 1)
    return n


def check_labels(lab: np.ndarray, n_rungs: int) -> None:
    """What amc_upload_labels refuses: w >= R, d == 3, a wrong direction at an end, walker ids that are no permutation."""
    R = n_rungs
    w, d = (lab & 63).reshape(-1, R), (lab >> 6).reshape(-1, R)
    assert w.max() < R and d.max() < 3
    assert np.all(d[:, 0] == UP) and np.all(d[:, R - 1] == DOWN)
    assert np.array_equal(np.sort(w, axis=1), np.tile(np.arange(R), (w.shape[0], 1)))


class TrackTwin(X.ExchangeTwin):
    """ExchangeTwin that may carry labels: set_tracking(True) as amc_set_tracking, then exchange() moves them as the text says."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.lab = None
        self.round_trips = self.up_trips = 0

    def set_tracking(self, on=True):
        self.lab = initial_labels(self.beta.size, self.R) if on else None
        self.round_trips = self.up_trips = 0

    def _swapped(self, a: int, r: int):
        lab = self.lab
        if lab is None:
            return
        lab[a], lab[a + 1] = lab[a + 1], lab[a]
        if r == 0:
            self.round_trips += int(lab[a] >> 6 == DOWN)
            lab[a] = (lab[a] & 63) | (UP << 6)
        if r + 1 == self.R - 1:
            self.up_trips += int(lab[a + 1] >> 6 == UP)
            lab[a + 1] = (lab[a + 1] & 63) | (DOWN << 6)

    def flow_rungs(self):
        return flow_counts(self.lab, self.R)


class TrackEngine(X.TwinEngine):
    """exchange_twin.TwinEngine with the tracking surface of montecarlo_amd._capi.HipEngine, computed by TrackTwin."""

    def set_ladder(self, n_rungs):
        assert self._beta is not None, "a ladder needs a per-chain beta array"
        self.twin = TrackTwin(self, self._beta, n_rungs, **self._kw)       # (a new ladder: tracking is off)
        self.n_rungs = int(n_rungs)

    def _tracked(self):
        if self.twin is None or self.twin.lab is None:
            raise RuntimeError("tracking is off")
        return self.twin

    def set_tracking(self, on=True):
        assert self.twin is not None, "tracking needs a ladder"
        self.twin.set_tracking(on)

    def labels(self):
        lab = self._tracked().lab
        return lab & np.uint8(63), lab >> np.uint8(6)

    def set_labels(self, walker, direction):
        lab = (np.asarray(walker, dtype=np.int64) | (np.asarray(direction, dtype=np.int64) << 6)).astype(np.uint8)
        check_labels(lab, self.n_rungs)
        self._tracked().lab = lab

    def flow_rungs(self):
        return self._tracked().flow_rungs()

    def tracking_counters(self):
        t = self._tracked()
        return t.round_trips, t.up_trips

    def set_tracking_counters(self, round_trips, up_trips):
        t = self._tracked()
        t.round_trips, t.up_trips = int(round_trips), int(up_trips)
