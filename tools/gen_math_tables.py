#!/usr/bin/env python3
"""Generate the lookup tables of the arithmetic spec v2 for BOTH implementations.

Writes the SAME literal values (C99 hex floats, correctly rounded from 60-digit decimals) to
    oracle/amc_tables.inc                 (included by oracle/amc_oracle.c)
    montecarlo_amd/csrc/amc_tables.h      (included by the HIP kernels; AMC_MATH_TABLES_STAGED, the same values in the layout
                                           of a block's LDS, is what every block copies there)

  EXP2[32]      2^(j/32)
  LOG_INVC[129], LOG_LOGC[129]   indexed by idx - 53, idx = (low exponent bit : top 7 mantissa bits) of the centred
                significand m in [sqrt(2)/2, sqrt(2)): c = interval midpoint (c = 1 for the two
                intervals that touch 1, so log(1) = 0 exactly), INVC = 1/c rounded to 9 fractional
                bits (exact in f64), LOGC = RN(-log INVC)
  SINPI[128], COSPI[128]         sin/cos(pi * j / 64), exact 0 / +-1 where they are exact

Float32 policy parameters (box_muller_f32) read two tables of Float32 PAIRS, written to
    montecarlo_amd/csrc/amc_tables.h      (AMC_MATH_TABLES_F32, staged into LDS per block by the forms that use it)
    tests/aux/f32_param_tables.inc        (the host twin of the tests; it shares no header with csrc/)

  LOGF[129]     (INVC, RN_f32(2 log INVC)) on the same 129 intervals: INVC has 9 fractional bits, exact in Float32;
                (1, 0) for the two intervals that touch 1
  SINCOSF[128]  (RN_f32 sin, RN_f32 cos)(pi * j / 64), exact 0 / +-1 where they are exact
Every Float32 entry is rounded ONCE, from the 60-digit decimal (no detour through a double).
"""
import os
from decimal import Decimal, getcontext

getcontext().prec = 70
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899")


def dsin(x):
    x = Decimal(x)
    term, s, n = x, x, 1
    while abs(term) > Decimal(10) ** -68:
        term = -term * x * x / ((2 * n) * (2 * n + 1))
        s += term
        n += 1
    return s


def dcos(x):
    x = Decimal(x)
    term, s, n = Decimal(1), Decimal(1), 1
    while abs(term) > Decimal(10) ** -68:
        term = -term * x * x / ((2 * n - 1) * (2 * n))
        s += term
        n += 1
    return s


def hexf(d):
    return float(d).hex()


def exp2_table():
    ln2 = Decimal(2).ln()
    return [hexf((ln2 * Decimal(j) / 32).exp()) for j in range(32)]


def log_tables():
    invc, logc = [], []
    for idx in range(256):
        top, j = idx >> 7, idx & 127
        # high word pattern: exponent 0x3fe (top = 0, m in [0.5, 1)) or 0x3ff (top = 1, m in [1, 2))
        lo = (Decimal(1) + Decimal(j) / 128) * (Decimal(1) if top else Decimal("0.5"))
        width = (Decimal(1) / 128) * (Decimal(1) if top else Decimal("0.5"))
        c = lo + width / 2
        if (top == 1 and j == 0) or (top == 0 and j == 127):
            c = Decimal(1)                      # intervals touching 1: r = m - 1, log(1) == 0 exactly
        # INVC is 1/c rounded to 9 fractional bits, so m*INVC - 1 is one exactly-rounded fma of an exact
        # product (no reciprocal rounding error enters r); LOGC = -log(INVC) absorbs the difference.
        q = (Decimal(1) / c * 512).to_integral_value(rounding="ROUND_HALF_EVEN") / 512
        invc.append(hexf(q))
        logc.append(hexf(-q.ln()) if q != 1 else "0x0.0p+0")
    # only indices 53..181 can occur: m in [sqrt(2)/2, 1) has top = 0, j >= 53; m in [1, sqrt(2)) has top = 1, j <= 53
    return invc[LOG_IDX_MIN:LOG_IDX_MAX + 1], logc[LOG_IDX_MIN:LOG_IDX_MAX + 1]


LOG_IDX_MIN, LOG_IDX_MAX = 53, 181


def sincos_tables():
    sn, cs = [], []
    for j in range(128):
        q, r = divmod(j, 32)                    # quadrant, position inside it: angle = pi*(q/2 + r/64)
        if r == 0:
            s0, c0 = Decimal(0), Decimal(1)
        elif r == 16:
            s0 = c0 = Decimal(0.5).sqrt()       # sin(pi/4)
        elif r < 16:
            s0, c0 = dsin(PI * r / 64), dcos(PI * r / 64)
        else:                                   # reflect about pi/4 so sin/cos tables are exactly symmetric
            s0, c0 = dcos(PI * (32 - r) / 64), dsin(PI * (32 - r) / 64)
        s, c = [(s0, c0), (c0, -s0), (-s0, -c0), (-c0, s0)][q]
        sn.append(hexf(s))
        cs.append(hexf(c))
    return sn, cs


def rn_f32(d):
    """The Float32 nearest to the Decimal d (ties to even), as a C99 hex float.  |d| is 0 or a normal Float32."""
    d = Decimal(d)
    if d == 0:
        return "0x0.0p+0"
    sign, a = ("-" if d < 0 else ""), abs(d)
    e = a.adjusted() * 4 - 8                      # a power of two safely below a ...
    while Decimal(2) ** (e + 1) <= a:             # ... raised to floor(log2 a)
        e += 1
    q = int((a / Decimal(2) ** (e - 23)).to_integral_value(rounding="ROUND_HALF_EVEN"))     # 24-bit significand, 2^23 <= q <= 2^24
    if q == 1 << 24:
        q, e = 1 << 23, e + 1
    assert (1 << 23) <= q < (1 << 24) and -126 <= e <= 127
    return f"{sign}0x1.{(q - (1 << 23)) << 1:06x}p{e:+d}"


def f32_tables():
    """LOGF and SINCOSF as flat lists of pairs (see the module's head)."""
    logf, scf = [], []
    invc, _ = log_tables()
    for h in invc:
        q = Decimal(float.fromhex(h))             # 9 fractional bits: exact
        logf += [rn_f32(q), rn_f32(2 * q.ln()) if q != 1 else "0x0.0p+0"]
    for j in range(128):
        q, r = divmod(j, 32)
        if r == 0:
            s0, c0 = Decimal(0), Decimal(1)
        elif r == 16:
            s0 = c0 = Decimal(0.5).sqrt()
        elif r < 16:
            s0, c0 = dsin(PI * r / 64), dcos(PI * r / 64)
        else:
            s0, c0 = dcos(PI * (32 - r) / 64), dsin(PI * (32 - r) / 64)
        s, c = [(s0, c0), (c0, -s0), (-s0, -c0), (-c0, s0)][q]
        scf += [rn_f32(s), rn_f32(c)]
    return logf, scf


def staged_image(e2, invc, logc, sn, cs):
    """The 546 doubles as a block keeps them in LDS (amc_math.h, LDS_*): the order EXP2 | LOG_INVC | LOG_LOGC | SINPI | COSPI rotated by
    the length of the cosine table, so that it comes first, and the LOGC entries times -2 (exact: a power of two)."""
    logc2 = [(-2.0 * float.fromhex(v)).hex() for v in logc]
    return cs + e2 + invc + logc2 + sn


def emit(name, vals, per_line=4):
    out = [f"static const double {name}[{len(vals)}] = {{"]
    for i in range(0, len(vals), per_line):
        out.append("    " + ", ".join(vals[i:i + per_line]) + ",")
    out.append("};")
    return "\n".join(out)


def main():
    e2 = exp2_table()
    invc, logc = log_tables()
    sn, cs = sincos_tables()
    body = "\n".join([emit("AMC_TAB_EXP2", e2), emit("AMC_TAB_LOG_INVC", invc), emit("AMC_TAB_LOG_LOGC", logc),
                      emit("AMC_TAB_SINPI", sn), emit("AMC_TAB_COSPI", cs)])
    assert len(invc) == 129 and len(e2) + 2 * len(invc) + 2 * len(sn) == 546
    head = ("/* GENERATED by tools/gen_math_tables.py -- do not edit.  Lookup tables of the arithmetic spec v2\n"
            " * (DESIGN.md section 3.4); the oracle and the HIP kernels carry identical literals. */\n")
    with open(os.path.join(ROOT, "oracle", "amc_tables.inc"), "w") as f:
        f.write(head + "#define AMC_TAB_LOG_IDX_MIN 53\n" + body + "\n")
    allv = e2 + invc + logc + sn + cs
    dev = emit("AMC_MATH_TABLES", allv).replace("static const double", "__device__ const double")
    staged = staged_image(e2, invc, logc, sn, cs)
    assert len(staged) == len(allv)
    dev_staged = emit("AMC_MATH_TABLES_STAGED", staged).replace("static const double", "__device__ const double").replace(
        "[546]", "[546] __attribute__((aligned(16)))")
    logf, scf = f32_tables()
    assert len(logf) == 258 and len(scf) == 256
    suffix = lambda vals: [v + "f" for v in vals]
    devf = emit("AMC_MATH_TABLES_F32", suffix(logf + scf)).replace("static const double", "__device__ const float")
    with open(os.path.join(ROOT, "tests", "aux", "f32_param_tables.inc"), "w") as f:
        f.write("/* GENERATED by tools/gen_math_tables.py -- do not edit.  Float32 tables of box_muller_f32 (DESIGN.md section 3.12):\n"
                " * pairs (INVC, 2 log INVC) and (sin, cos)(pi j / 64), the literals the HIP kernels carry. */\n"
                "#define TWIN_LOG_IDX_MIN 53\n" + emit("TWIN_LOGF", suffix(logf)).replace("const double", "const float") + "\n" +
                emit("TWIN_SINCOSF", suffix(scf)).replace("const double", "const float") + "\n")
    with open(os.path.join(ROOT, "montecarlo_amd", "csrc", "amc_tables.h"), "w") as f:
        f.write(head + "#pragma once\n#ifndef __HIPCC_RTC__   /* hiprtc (custom potentials) predefines the device API */\n#include <hip/hip_runtime.h>\n#endif\nnamespace amc {\n"
                "// one array: EXP2[32] | LOG_INVC[129] | LOG_LOGC[129] | SINPI[128] | COSPI[128]; the log tables are\n"
                "// indexed by idx - TAB_LOG_IDX_MIN (only idx in [53, 181] can occur)\n"
                "enum { TAB_EXP2 = 0, TAB_LOG_INVC = 32, TAB_LOG_LOGC = 161, TAB_SINPI = 290, TAB_COSPI = 418,\n"
                "       TAB_DOUBLES = 546, TAB_LOG_IDX_MIN = 53 };\n" + dev + "\n"
                "// the same 546 doubles as a block's LDS holds them (amc_math.h, LDS_*): rotated so that COSPI comes first, the\n"
                "// LOG_LOGC entries times -2 (exact); stage_math_tables copies this image, 273 16-byte quads\n" + dev_staged + "\n"
                "// Float32 policy parameters (box_muller_f32): pairs -- LOGF[129] (INVC, 2 log INVC), same index as above;\n"
                "// SINCOSF[128] (sin, cos)(pi j / 64).  TABF_* count PAIRS.\n"
                "enum { TABF_LOG = 0, TABF_SINCOS = 129, TABF_PAIRS = 257 };\n" + devf + "\n}  // namespace amc\n")
    def jl(name, vals):
        dec = [repr(float.fromhex(v)) for v in vals]        # shortest round-trip decimals: exact when parsed
        return f"const {name} = Float64[\n    " + ",\n    ".join(", ".join(dec[i:i + 4]) for i in range(0, len(dec), 4)) + "]\n"
    os.makedirs(os.path.join(ROOT, "julia", "src"), exist_ok=True)
    with open(os.path.join(ROOT, "julia", "src", "amc_tables.jl"), "w") as f:
        f.write("# GENERATED by tools/gen_math_tables.py -- do not edit.  Same literals as oracle/amc_tables.inc.\n"
                "const AMC_TAB_LOG_IDX_MIN = 53\n" + jl("AMC_TAB_LOG_INVC", invc) + jl("AMC_TAB_LOG_LOGC", logc) +
                jl("AMC_TAB_SINPI", sn) + jl("AMC_TAB_COSPI", cs))
    print("EXP2[1] =", e2[1], " INVC[128-53] =", invc[75], " LOGC[129-53] =", logc[76], " SINPI[16] =", sn[16])


if __name__ == "__main__":
    main()
