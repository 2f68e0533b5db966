"""numpy model of the harmonic sweeps' filter argument (amc_model.h: harmonic_filter_setup, harmonic_filter_y), operation for
operation, and the reference-ordered dlogp it stands in for.  Shared by test_filter_argument_bound.py (CPU) and
test_gpu_filter_argument.py (device values against this model)."""
import numpy as np

LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")


def _exponent(v):
    hi = int(np.float64(v).view(np.uint64)) >> 32
    return ((hi >> 20) & 0x7FF) - 1023, hi >> 31


def setup(beta, sigma):
    """(nbl, cs, l): the launch constants.  nbl is NaN where the launch decides everything by accept_exact."""
    eb, sign = _exponent(beta)
    es, _ = _exponent(sigma)
    l = (28 - max(eb, -64)) >> 1
    ok = sign == 0 and eb <= 24 and es + 5 <= l
    with np.errstate(all="ignore"):
        nbl = np.float32(-(np.float64(beta) * np.float64(LOG2E))) if ok else np.float32(np.nan)
    cs = np.uint32(((255 - l) << 23) & 0xFFFFFFFF).view(np.float32)      # (wraps like the device's 32-bit shift; read only where nbl is no NaN)
    return nbl, cs, l


def y_model(x, delta, beta, sigma):
    """y as a lane forms it: Float32, NaN outside the guard."""
    x = np.asarray(x, dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    nbl, cs, _ = setup(beta, sigma)
    with np.errstate(all="ignore"):
        xn = x + delta
        sf = (xn + x).astype(np.float32)
        df = delta.astype(np.float32)
        g = (sf * cs) * np.float32(0.0)
        w = df * nbl
        # fma(w, sf, g): the product of two Float32 is exact in Float64, g is a zero or NaN -- one rounding
        return (w.astype(np.float64) * sf.astype(np.float64) + g.astype(np.float64)).astype(np.float32)


def dlogp_reference(x, delta, beta):
    """delta_log_target in the reference's operation order (Float64; numpy fuses nothing)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        xn = x + np.asarray(delta, dtype=np.float64)
        e1 = x * x
        e2 = xn * xn
        return ((-e2) * beta) - ((-e1) * beta)
