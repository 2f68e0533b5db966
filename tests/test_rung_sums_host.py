"""Per-rung reproducible sums (amc_reduce_rungs_exact) without a GPU: the entry through the C ABI, the host
twin's shard invariance (tests/rung_sums_twin.py, the oracle only), and ReplicaExchange.rung_sums' chunked all-reduce through an engine
double."""
import ctypes as C
import os

import numpy as np

import montecarlo_amd as ma
from montecarlo_amd import exchange as EX

import exchange_twin as X
import rung_sums_twin as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_declared_bound_and_refuses_a_null_handle(amc):
    name = "amc_reduce_rungs_exact"
    header = open(os.path.join(ROOT, "include", "amc.h")).read()
    assert "int  amc_reduce_rungs_exact(amc_handle *h, int columns, double *records);" in header
    lib = amc.load()
    assert name in amc.SIGNATURES
    res, args = amc.SIGNATURES[name]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    zeros = [None if (a is C.c_void_p or hasattr(a, "contents")) else a(0) for a in args]
    assert getattr(lib, name)(*zeros) == -1
    assert name.encode() in lib.amc_last_error()
    assert (amc.AMC_REDUCE_E, amc.AMC_REDUCE_X, amc.AMC_REDUCE_XX, amc.AMC_REDUCE_ALL) == (1, 2, 4, 7)
    assert hasattr(amc.HipEngine, "reduce_rungs") and callable(ma.callback_rung_energy) and callable(ma.callback_rung_moments)


def _state(M):
    """Positions over many levels, a function of the global chain id: magnitudes from 1e-30 to 1e30, both signs."""
    ids = np.arange(M)
    x = np.sin(0.731 * ids + 0.2) * 10.0 ** (((ids * 7) % 61) - 30.0)
    return x, x * x


def test_twin_records_do_not_depend_on_the_shard_split(oracle):
    R, L = 3, 342
    M = R * L
    x, e = _state(M)
    whole = RS.records(x, e, R)
    assert whole.shape == (R, 3, RS.WORDS) and np.all(whole[:, :, 0] == 2.0)          # kind R
    for split in ([0, 402, M], [0, 258, 264, M]):
        parts = [RS.records(x[a:b], e[a:b], R) for a, b in zip(split, split[1:])]
        got = RS.merge(parts)
        assert np.array_equal(got.view(np.uint64), whole.view(np.uint64))
        assert np.array_equal(RS.values(got).view(np.uint64), RS.values(whole).view(np.uint64))
    # the value is the sum: every summand is rounded to a multiple of q_(top - 1) <= 2^-49 max |v| (half a quantum of error each),
    # the integer total once more to 53 bits -- against Python's exact rational arithmetic
    from fractions import Fraction
    for r in range(R):
        exact = float(sum(Fraction(float(v)) for v in x[r::R]))
        assert abs(RS.values(whole)[r, 1] - exact) <= L * 2.0 ** -50 * np.max(np.abs(x[r::R])) + 2.0 ** -52 * abs(exact)
    # a level per rung: a huge value in rung 2 leaves the records of rungs 0 and 1 as they were
    y = x.copy()
    y[2::R] *= 1e200
    other = RS.records(y, e, R, RS.X)
    assert np.array_equal(other[:2, 1], whole[:2, 1]) and other[2, 1, 1] > whole[2, 1, 1]
    assert not other[:, 0].any() and not other[:, 2].any()                            # columns nobody asked for: all-zero records


class _ChunkRecorder(X.TwinEngine):
    """TwinEngine with reduce_rungs computed by the twin and an allreduce_xsum that refuses what amc_allreduce_xsum would refuse."""
    CAPACITY = 68              # records per call: (AMC_RED_HEADER + AMC_MAX_MOVES), what a communicator's buffers always hold

    def reduce_rungs(self, columns=7):
        x, e = self.download_state()
        return RS.records(x, e, self.n_rungs, int(columns))

    def allreduce_xsum(self, records):
        rec = np.asarray(records, dtype=np.float64).reshape(-1, RS.WORDS)
        if rec.shape[0] > self.CAPACITY:
            raise ma.AmcError(f"amc_allreduce_xsum: at most {self.CAPACITY} records")
        self.chunks.append(rec.shape[0])
        return rec.copy()


def test_rung_sums_chunk_their_all_reduce(oracle, tmp_path):
    assert EX.XSUM_CHUNK == _ChunkRecorder.CAPACITY
    for R, want in [(64, [68, 68, 56]), (3, [9]), (23, [68, 1])]:
        L = 2
        betas = list(0.5 * 1.05 ** np.arange(R))
        chains = ma.ParticleChains.ladder(L, betas, x=np.linspace(-1.5, 1.5, R * L), potential="double_well")
        pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 1.0),)
        al = [dict(algorithm=ma.Metropolis, pool=pool, seed=7, engine_factory=_ChunkRecorder),
              dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(2, 0, 1))]
        sim = ma.Simulation(chains, al, 2, path=str(tmp_path / str(R)))
        ma.run(sim)
        eng = sim.algorithms[0].engine
        eng.chunks = []
        eng.comm_connected = True                      # sharding.allreduce_xsum then goes through the engine's communicator
        got = sim.algorithms[1].rung_sums()
        assert eng.chunks == want
        x, e = eng.download_state()
        ref = RS.means(RS.records(x, e, R), L)
        assert got.shape == (R, 3) and np.array_equal(got.view(np.uint64), ref.view(np.uint64))
        eng.chunks = []
        assert np.array_equal(ma.callback_rung_energy(sim).view(np.uint64), ref[:, 0].copy().view(np.uint64))
        mom = ma.callback_rung_moments(sim)
        assert mom.shape == (2, R) and np.array_equal(mom.view(np.uint64), np.ascontiguousarray(ref[:, 1:].T).view(np.uint64))
        only_e = sim.algorithms[1].rung_sums(RS.E)
        assert np.array_equal(only_e[:, 0].copy().view(np.uint64), ref[:, 0].copy().view(np.uint64)) and np.isnan(only_e[:, 1:]).all()
        eng.comm_connected = False
