"""Host twin of the all-Float32 model (Float32 state and Float32 policy parameters).

tests/aux/f32_param_twin.c restates the new arithmetic in plain C floats and takes everything that does not change from the
oracle's exported functions; this module compiles it with the host compiler (-O2 -ffp-contract=off, the way oracle_lib builds
its expression libraries) and wraps it: the pieces of box_muller_f32, one mc_step!, and TwinSim -- the counterpart of
oracle_lib.OracleSim for a handle with param_dtype = "f32".
"""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "aux", "f32_param_twin.c")
INC = os.path.join(HERE, "aux", "f32_param_tables.inc")

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    O.load()                                             # builds the oracle if it is not there
    with open(SRC, "rb") as f, open(INC, "rb") as g:
        key = hashlib.sha1(f.read() + g.read()).hexdigest()[:16]
    d = os.path.join(tempfile.gettempdir(), f"amc_f32_twin_{os.getuid()}_{key}")
    so = os.path.join(d, "libf32_param_twin.so")
    if not os.path.exists(so):
        os.makedirs(d, exist_ok=True)
        tmp = so + f".{os.getpid()}.tmp"
        # -mfma only makes fmaf() an instruction (libm's is correctly rounded as well); no contraction of a*b+c anywhere
        subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-fno-math-errno", "-fopenmp",
                        "-I", os.path.join(HERE, "aux"), SRC, "-o", tmp, O.LIB_PATH, "-lm", f"-Wl,-rpath,{O.ORACLE_DIR}"],
                       check=True, capture_output=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    u32p, f32p, dp, i64p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    sig = {
        "twin_uniform_oc_f32": (C.c_float, [C.c_uint32, C.c_uint32]),
        "twin_neg2log_f32": (C.c_float, [C.c_float]),
        "twin_sincospi_f32": (None, [C.c_uint32, f32p, f32p]),
        "twin_box_muller_f32": (None, [u32p, f32p]),
        "twin_box_muller_words": (None, [C.c_int64, u32p, f32p, f32p]),
        "twin_normal_words": (None, [C.c_uint64, C.c_uint64, C.c_int64, C.c_uint64, u32p]),
        "twin_logq": (C.c_double, [C.c_float, C.c_float]),
        "twin_mc_step": (C.c_int, [C.c_int, C.c_float, C.c_float, C.c_float, C.c_double, f32p, f32p]),
        "twin_init_uniform": (None, [C.c_uint64, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_double, f32p, f32p]),
        "twin_sweep": (None, [C.c_uint64, C.c_int64, C.c_int64, C.c_int, f32p, C.c_int, f32p, dp, C.c_uint64, C.c_int64,
                              f32p, f32p, i64p, i64p, f32p, dp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def normal_words(seed: int, pair0: int, n: int, t: int) -> np.ndarray:
    """The NORMAL draws of n consecutive pairs at step t, shape (n, 4) uint32 (Philox through the oracle)."""
    w = np.empty((n, 4), dtype=np.uint32)
    load().twin_normal_words(int(seed), int(pair0), int(n), int(t), _p(w, C.c_uint32))
    return w


def box_muller_words(words: np.ndarray):
    """(z [n, 2] float32, u [n] float32) of words [n, 4] uint32."""
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 4)
    z = np.empty((len(words), 2), dtype=np.float32)
    u = np.empty(len(words), dtype=np.float32)
    load().twin_box_muller_words(len(words), _p(words, C.c_uint32), _p(z, C.c_float), _p(u, C.c_float))
    return z, u


def radius_uniform_reference(words: np.ndarray) -> np.ndarray:
    """The radius uniform of the specification restated with numpy: N = 2 ((y:x) >> 12) + 1, the high word exact, the low
    word and the sum rounded to Float32 (the sum of two Float32 values is formed exactly in Float64, then rounded once)."""
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 4)
    n52 = ((words[:, 1].astype(np.uint64) << np.uint64(32)) | words[:, 0].astype(np.uint64)) >> np.uint64(12)
    big = n52 * np.uint64(2) + np.uint64(1)
    hi = (big >> np.uint64(32)).astype(np.uint32).astype(np.float32)
    lo = (big & np.uint64(0xFFFFFFFF)).astype(np.uint32).astype(np.float32)
    return (hi.astype(np.float64) * 2.0 ** 32 + lo.astype(np.float64)).astype(np.float32) * np.float32(2.0 ** -53)


def box_muller_reference(words: np.ndarray, u: np.ndarray) -> np.ndarray:
    """The same formula in Float64 by numpy: sqrt(-2 log u) (sin, cos)(pi w) with u the Float32 radius uniform (its construction
    is part of the specification) and w = (2^24 - (word >> 8)) 2^-23 the exact angle."""
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 4)
    a = (np.int64(1 << 24) - (words[:, 3] >> np.uint32(8)).astype(np.int64)).astype(np.float64)
    # reduce the angle exactly before multiplying by pi (the sine of a large multiple of pi would lose the accuracy we measure)
    n = np.rint(a / 131072.0)
    r = (a - n * 131072.0) * 2.0 ** -23                      # in [-1/128, 1/128], exact
    th = np.pi * (n % 128) / 64.0
    s = np.sin(th) * np.cos(np.pi * r) + np.cos(th) * np.sin(np.pi * r)
    c = np.cos(th) * np.cos(np.pi * r) - np.sin(th) * np.sin(np.pi * r)
    rad = np.sqrt(-2.0 * np.log(u.astype(np.float64)))
    return np.stack([rad * s, rad * c], axis=1)


def mc_step(pot: int, beta, sigma, z, u, x, e):
    xx, ee = C.c_float(x), C.c_float(e)
    a = load().twin_mc_step(int(pot), float(beta), float(sigma), float(z), float(u), C.byref(xx), C.byref(ee))
    return a, np.float32(xx.value), np.float32(ee.value)


class TwinSim:
    """M chains of the all-Float32 model with global ids chain_offset .. (the interface of oracle_lib.OracleSim that the tests
    use).  potential: "harmonic", "double_well" or a CustomPotential-like object with .expr (installed into the oracle, whose
    amo_potential_f32 the twin calls)."""

    def __init__(self, n_chains, *, chain_offset=0, potential="harmonic", beta=1.0, sigma=(1.0,), weight=(1.0,), seed=1):
        self.lib = load()
        self.potential = potential
        expr = getattr(potential, "expr", None)
        if expr is not None:
            O.install_custom_potential(expr)
            self.pot = 2
        else:
            self.pot = {"harmonic": 0, "double_well": 1}[potential]
        self.M, self.offset, self.seed = int(n_chains), int(chain_offset), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.K = len(sigma)
        s32 = np.asarray(sigma, dtype=np.float32)
        assert np.array_equal(s32.astype(np.float64), np.asarray(sigma, dtype=np.float64)), "sigma must hold Float32 values"
        self.sigma = np.ascontiguousarray(s32)
        self.weight = np.ascontiguousarray(weight, dtype=np.float64)
        self.beta = np.full(self.M, np.float32(beta), dtype=np.float32)
        self.x = np.zeros(self.M, dtype=np.float32)
        self.e = np.zeros(self.M, dtype=np.float32)
        self.acc = np.zeros((self.K, self.M), dtype=np.int64)
        self.tot = np.zeros((self.K, self.M), dtype=np.int64)
        self.t = 0

    def init_uniform(self, lo, hi):
        self.lib.twin_init_uniform(self.seed, self.offset, self.M, self.pot, float(lo), float(hi), _p(self.x, C.c_float), _p(self.e, C.c_float))

    def set_sigma(self, k, s):
        assert float(np.float32(s)) == float(s)
        self.sigma[k] = np.float32(s)

    def make_steps(self, n=1, record=False):
        z = np.empty((n, self.M), dtype=np.float32) if record else None
        u = np.empty((n, self.M), dtype=np.float64) if record else None
        self.lib.twin_sweep(self.seed, self.offset, self.M, self.pot, _p(self.beta, C.c_float), self.K, _p(self.sigma, C.c_float),
                            _p(self.weight, C.c_double), self.t, int(n), _p(self.x, C.c_float), _p(self.e, C.c_float),
                            _p(self.acc, C.c_int64), _p(self.tot, C.c_int64), _p(z, C.c_float), _p(u, C.c_double))
        self.t += int(n)
        return z, u

    def state(self):
        """(x, e) widened to Float64 (exact): what HipEngine.download_state returns."""
        return self.x.astype(np.float64), self.e.astype(np.float64)

    def counters(self):
        return self.acc.copy(), self.tot.copy()

    def callback_records(self):
        """The callbacks' sums of the twin's state as records, (4 + K, XS_WORDS).  The sums are no new arithmetic: they are the
        oracle's, formed by a Float32-state OracleSim that is handed this state and these counters."""
        sim = O.OracleSim(self.M, chain_offset=self.offset, potential=self.potential, beta=float(self.beta[0]),
                          sigma=[float(s) for s in self.sigma], weight=list(self.weight), seed=self.seed, dtype="f32")
        sim.set_x(self.x.astype(np.float64))
        p = C.POINTER(C.c_int64)
        sim.lib.amo_set_counters(sim.h, np.ascontiguousarray(self.acc).ctypes.data_as(p), np.ascontiguousarray(self.tot).ctypes.data_as(p))
        rec = sim.callback_records()
        sim.close()
        return rec
