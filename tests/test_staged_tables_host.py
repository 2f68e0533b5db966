"""The staged image of the math tables (AMC_MATH_TABLES_STAGED in montecarlo_amd/csrc/amc_tables.h, written by
tools/gen_math_tables.py) against the unrotated array beside it: the layout a block keeps in LDS (amc_math.h: the cosine table
first, the rest behind it in order) with the LOGC entries times -2.  No GPU."""
import os
import re
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "montecarlo_amd", "csrc", "amc_tables.h")
TAB = dict(EXP2=0, LOG_INVC=32, LOG_LOGC=161, SINPI=290, COSPI=418, DOUBLES=546)


def header_array(name):
    text = open(HEADER).read()
    m = re.search(r"const double %s\[(\d+)\][^=]*= \{(.*?)\};" % name, text, re.S)
    assert m, name
    vals = [v.strip() for v in m.group(2).split(",") if v.strip()]
    assert len(vals) == int(m.group(1))
    return vals


def word(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_header_offsets_are_the_ones_this_test_assumes():
    text = open(HEADER).read()
    for k, v in TAB.items():
        assert re.search(r"\bTAB_%s = %d\b" % (k, v), text), k


def test_staged_array_is_the_unrotated_one_rotated_and_scaled():
    plain = [float.fromhex(v) for v in header_array("AMC_MATH_TABLES")]
    staged = [float.fromhex(v) for v in header_array("AMC_MATH_TABLES_STAGED")]
    assert len(plain) == len(staged) == TAB["DOUBLES"]
    rot = TAB["DOUBLES"] - TAB["COSPI"]
    want = [None] * TAB["DOUBLES"]
    for i, v in enumerate(plain):
        scaled = -2.0 * v if TAB["LOG_LOGC"] <= i < TAB["SINPI"] else v
        want[i + rot if i < TAB["COSPI"] else i - TAB["COSPI"]] = scaled
    assert [word(v) for v in staged] == [word(v) for v in want]        # bits: log(1) = 0 is staged as -0.0, what -2.0 * 0.0 gives
    assert staged[:128] == plain[TAB["COSPI"]:] and staged[0] == 1.0   # the cosine table leads
    assert word(staged[rot + TAB["LOG_LOGC"] + 128 - 53]) == word(-0.0)


def test_staged_array_is_16_byte_aligned_whole_quads():
    text = open(HEADER).read()
    assert re.search(r"AMC_MATH_TABLES_STAGED\[546\] __attribute__\(\(aligned\(16\)\)\)", text)
    assert TAB["DOUBLES"] % 2 == 0


def test_header_is_what_the_generator_emits():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_math_tables as G
    finally:
        sys.path.pop(0)
    invc, logc = G.log_tables()
    sn, cs = G.sincos_tables()
    e2 = G.exp2_table()
    assert header_array("AMC_MATH_TABLES") == e2 + invc + logc + sn + cs
    assert header_array("AMC_MATH_TABLES_STAGED") == G.staged_image(e2, invc, logc, sn, cs)
