"""Host twin of the weight sums per block of families (DESIGN.md section 3.14 "Error bars"; include/amc.h amc_set_anneal_blocks), over
anneal_twin unchanged: the partition "block of chain c = (fam[c] div chunk) mod B", the block record of every annealing step -- n_b, the
chains of block b before the resampling, and T_b, the sum of the same integer weights W_c the step resamples by -- in Python integers,
a brute-force delete-one-block jackknife of log Z that recomputes every replicate from the chains' own weights, and the energy
histogram per block of families over ehist_twin unchanged (its energies and its binning rule; the block of a chain chosen here).  It
shares no code with the product.
"""
import math

import numpy as np

import anneal_twin as A
import ehist_twin as E


def histogram_by_block(potential, x, fam, B: int, chunk: int, lo, hi, n_bins, f32=False) -> np.ndarray:
    """counts[B, n_bins + 3] (uint64): ehist_twin's cell of every chain's energy, counted in the row of the block of its family."""
    cell = E.cells(E.energies(potential, x, f32), lo, hi, n_bins)
    out = np.zeros((int(B), int(n_bins) + 3), dtype=np.uint64)
    np.add.at(out, (block_of(fam, B, chunk), cell), np.uint64(1))
    return out


def default_chunk(M: int, B: int) -> int:
    return -(-int(M) // int(B))


def block_of(fam, B: int, chunk: int):
    return (np.asarray(fam, dtype=np.int64) // int(chunk)) % int(B)


class AnnealBlocksTwin(A.AnnealTwin):
    """AnnealTwin with families on and the partition (B, chunk); set_blocks(0) turns it off.  ``weights`` keeps every step's
    (status, a_max bits, W, block of every chain, family of every chain -- both before the resampling) for the brute-force jackknife
    and for block records under any other partition (block_records_under)."""

    def __init__(self, sim, beta, *, blocks=0, chunk=0, **kw):
        kw["families"] = True
        super().__init__(sim, beta, **kw)
        self.potential = kw.get("potential", "harmonic")
        self.set_blocks(blocks, chunk)

    def set_blocks(self, B, chunk=0):
        self.B = int(B)
        self.chunk = (int(chunk) or default_chunk(self.M, B)) if self.B else 0
        self.block_records, self.weights = [], []

    def block_counts(self):
        return np.bincount(block_of(self.fam, self.B, self.chunk), minlength=self.B).astype(np.uint64)

    def anneal(self, beta_new):
        if not self.B:
            return super().anneal(beta_new)
        fam = self.fam.copy()
        blk = block_of(fam, self.B, self.chunk)               # of the chains BEFORE the resampling
        super().anneal(beta_new)
        status = self.records[-1][0]
        n, T = [0] * self.B, [0] * self.B
        W = self.last["W"] if status == A.OK else [0] * self.M
        for b, w in zip(blk.tolist(), W):
            n[b] += 1
            T[b] += int(w)
        assert sum(n) == self.M and sum(T) == self.records[-1][4]
        self.block_records.append([n, T])
        self.weights.append((status, self.records[-1][3], list(W), blk, fam))

    def histogram_by_block(self, lo, hi, n_bins):
        return histogram_by_block(self.potential, self.x(), self.fam, self.B, self.chunk, lo, hi, n_bins, self.f32)

    def block_records_array(self):
        return np.array(self.block_records, dtype=np.uint64).reshape(-1, 2, self.B)


def block_records_under(weights, B: int, chunk: int):
    """The block records [S, 2, B] the same steps give under the partition (B, chunk): the resampling does not depend on it."""
    out = []
    for status, _, W, _, fam in weights:
        n, T = [0] * B, [0] * B
        for b, w in zip(block_of(fam, B, chunk).tolist(), W):
            n[b] += 1
            T[b] += int(w)
        out.append([n, T])
    return np.array(out, dtype=np.uint64).reshape(-1, 2, B)


def brute_force_log_z(weights, M: int, B: int):
    """(value[S], se[S], replicates[S, B]) of the cumulative log Z by recomputing every replicate from the chains: replicate b of step
    s is a_max + log(sum of W over the chains NOT in block b) - log(their number) - 30 log 2, NaN where either is 0 or the step did not
    resample; cumulative sums; se^2 = (B' - 1) / B' sum (theta_b - mean)^2 over the blocks that hold a chain at the first step."""
    S = len(weights)
    value, rep = np.full(S, math.nan), np.full((S, B), math.nan)
    shift = A.WEIGHT_BITS * math.log(2.0)
    for s, (status, amax_bits, W, blk, _) in enumerate(weights):
        if status != A.OK:
            continue
        a_max = A.bits_f64(amax_bits)
        value[s] = a_max + math.log(sum(W)) - math.log(M) - shift
        for b in range(B):
            rest = [w for w, k in zip(W, blk.tolist()) if k != b]
            if rest and sum(rest):
                rep[s, b] = a_max + math.log(sum(rest)) - math.log(len(rest)) - shift
    value, rep = np.cumsum(value), np.cumsum(rep, axis=0)
    se = np.full(S, math.nan)
    if S:
        alive = np.bincount(weights[0][3], minlength=B) > 0
        k = int(alive.sum())
        if k >= 2:
            th = rep[:, alive]
            se = np.sqrt((k - 1) / k * ((th - th.mean(axis=1, keepdims=True)) ** 2).sum(axis=1))
    return value, se, rep


class AnnealBlocksTwinEngine(A.AnnealTwinEngine):
    """AnnealTwinEngine with the block surface of montecarlo_amd._capi.HipEngine (set_anneal_blocks .. anneal_block_counts)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        t = self.twin
        self.twin = AnnealBlocksTwin(self.sim, t.beta, seed=t.seed, potential=kw.get("potential", "harmonic"), f32=t.f32)
        self.twin.fam = None                                   # families off until set_anneal_families, as on the device
        self._blk_drained = 0

    def set_anneal_families(self, on=True):
        super().set_anneal_families(on)
        self.twin.set_blocks(0)
        self._blk_drained = 0

    def set_anneal_blocks(self, n_blocks, chunk=0):
        assert n_blocks == 0 or self.twin.fam is not None, "families are off"
        self.twin.set_blocks(n_blocks, chunk)
        self._blk_drained = 0

    def anneal_block_records(self, reset=False):
        assert self.twin.B, "no partition"
        out = self.twin.block_records_array()[self._blk_drained:]
        if reset:
            self._blk_drained = len(self.twin.block_records)
        return out

    def set_anneal_block_records(self, records):
        rec = np.asarray(records, dtype=np.uint64).reshape(-1, 2, self.twin.B)
        self.twin.block_records = [[list(map(int, r[0])), list(map(int, r[1]))] for r in rec]
        self._blk_drained = 0

    def anneal_block_counts(self):
        return self.twin.block_counts()

    # the energy histograms PopulationAnnealing takes: [accumulate; fetch with reset], plain or per block of families
    def energy_histogram_accumulate(self, lo, hi, n_bins):
        self._hist = (E.snapshot(self.twin.potential, self.twin.x(), lo, hi, n_bins, 1, self.twin.f32), (lo, hi, n_bins))

    def energy_histogram_fetch(self, reset=False):
        return self._hist[0], 1, self._hist[1]

    def energy_histogram_accumulate_blocks(self, lo, hi, n_bins):
        assert self.twin.B, "no partition"
        self._hist = (self.twin.histogram_by_block(lo, hi, n_bins)[:, None, :], (lo, hi, n_bins))

    def energy_histogram_fetch_blocks(self, reset=False):
        return self._hist[0], 1, self._hist[1]
