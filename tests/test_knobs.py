"""The environment variables of libamc.so: one table (AmcKnobs in amc_internal.h), one reader (amc_env / amc_knobs in amc_api.hip),
the same names in DESIGN.md section 9; handle knobs take effect when the handle is created; the run-time compiler's disk cache key
is spelt as it always was, so existing cache directories still hit."""
import os
import re
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo_amd", "csrc")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _sources():
    return {f: _read("montecarlo_amd", "csrc", f) for f in sorted(os.listdir(CSRC))
            if f.endswith((".hip", ".h", ".cpp")) and not f.endswith(".gen.h")}


def _table():
    """Names in the code table: the knobs of struct AmcKnobs and the process settings listed below it."""
    s = _read("montecarlo_amd", "csrc", "amc_internal.h")
    block = s[s.index("struct AmcKnobs {"):s.index("AMC_INTERNAL const char* amc_env(")]
    knobs = block[:block.index("};")]
    return set(re.findall(r"\bAMC_[A-Z0-9_]+\b", knobs)), set(re.findall(r"\bAMC_[A-Z0-9_]+\b", block[block.index("};"):]))


def test_every_variable_is_read_in_one_place():
    srcs = _sources()
    for name, text in srcs.items():
        if name == "amc_rtc_worker.cpp":            # a program of its own: its one test hook
            assert re.findall(r"getenv\(\"(\w+)\"", text) == ["AMC_RTC_WORKER_FAULT"]
        elif name == "amc_api.hip":                 # the reader: amc_env is the one getenv of the library
            assert text.count("getenv(") == 1 and "const char* amc_env(const char* name) { return std::getenv(name); }" in text
        else:
            assert "getenv(" not in text, name
    knobs, settings = _table()
    api = srcs["amc_api.hip"]
    reader = api[api.index("AmcKnobs amc_knobs()"):]
    reader = reader[:reader.index("\n}\n")]
    assert set(re.findall(r"\"(AMC_[A-Z0-9_]+)\"", reader)) == knobs          # amc_knobs reads every handle knob, nothing else
    # process settings: fetched through amc_env where they are used, and listed in the table
    used = set()
    for name, text in srcs.items():
        if name != "amc_rtc_worker.cpp":
            used |= set(re.findall(r"amc_env\(\"(AMC_[A-Z0-9_]+)\"\)", text.replace(reader, "")))
    assert used == settings


def test_design_lists_the_same_variables():
    design = _read("DESIGN.md")
    section = design[design.index("## 9."):]
    rows = re.findall(r"^\| `(AMC_[A-Z0-9_]+)` \| ([^|]+)\|", section, re.M)
    knobs, settings = _table()
    assert len(rows) == len(set(r[0] for r in rows))                           # each once
    assert set(r[0] for r in rows) == knobs | settings
    assert {r[0] for r in rows if r[1].startswith("process")} == settings


def _fnv1a(data, h=1469598103934665603):
    for c in data:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _hiprtc_version():
    import ctypes
    for n in ("libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"):
        try:
            lib = ctypes.CDLL(n)
            break
        except OSError:
            continue
    else:
        pytest.fail("libhiprtc cannot be loaded: the run-time compiler has nothing to run")
    major, minor = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.hiprtcVersion(ctypes.byref(major), ctypes.byref(minor)) == 0
    return major.value, minor.value


def _cache_name(expr, inst, arch, toolchain):
    """amc_rtc.hip rtc_cache_path, restated: FNV-1a over expression, instantiation, ISA, toolchain text and every kernel source."""
    mk = _read("montecarlo_amd", "csrc", "Makefile")
    headers = re.search(r"^KERNEL_HEADERS = (.*?)(?<!\\)\n", mk, re.M | re.S).group(1).replace("\\\n", " ").split()
    h = _fnv1a(expr.encode())
    h = _fnv1a(inst.encode(), h ^ 0x9E3779B97F4A7C15)
    h = _fnv1a(arch.encode(), h ^ 0xC2B2AE3D27D4EB4F)
    h = _fnv1a(toolchain.encode(), h)
    for f in headers:
        h = _fnv1a(open(os.path.join(CSRC, f), "rb").read(), h)
    return "amc_rtc_%016x.bin" % h


# (environment, the variant text the disk key has always carried for it; energy_kernel is no estimator form)
CACHE_CASES = [
    ({}, ""),
    ({"AMC_NO_SIGMA_MEMO": "1"}, " no-sigma-memo"),
    ({"AMC_NO_GAUSS_CLASS_ROWS": "", "AMC_RTC_WAVES": "3"}, " no-gauss-rows waves3"),
    ({"AMC_RTC_LICM": "all-off", "AMC_NO_SIGMA_MEMO": "0"}, " licm-off no-sigma-memo"),
    ({"AMC_RTC_LICM": "est-off"}, ""),
]


def test_disk_cache_key_is_unchanged(tmp_path):
    """A code object planted under the name the key has always had is found: amc_potential_check returns without compiling and
    writes no file of its own.  One process, the variables changed between calls: each call reads them afresh."""
    major, minor = _hiprtc_version()
    expr, inst = "x*x + 0.4375*x", "amc::energy_kernel<2>"
    dirs = []
    for i, (env, variant) in enumerate(CACHE_CASES):
        d = tmp_path / str(i)
        d.mkdir()
        name = _cache_name(expr, inst, "gfx950", "hiprtc %d.%d%s" % (major, minor, variant))
        lowered, code = b"planted", b"not a code object"
        (d / name).write_bytes(struct.pack("<3Q", 0x31435452434d41, len(lowered), len(code)) + lowered + code)
        dirs.append((str(d), env, name))
    script = """
import os, sys
sys.path.insert(0, %r)
from montecarlo_amd import _capi
for d, env, name in %r:
    for k in ("AMC_NO_SIGMA_MEMO", "AMC_NO_GAUSS_CLASS_ROWS", "AMC_RTC_WAVES", "AMC_RTC_LICM"):
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["AMC_RTC_CACHE_DIR"] = d
    assert _capi.potential_check(%r) == ""
    print(d, sorted(os.listdir(d)) == [name], flush=True)
""" % (ROOT, dirs, expr)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for (d, env, name), line in zip(dirs, r.stdout.splitlines()):
        assert line == d + " True", (env, sorted(os.listdir(d)), name)


def _model_text(sample, logq, dlogq=None, perform=None, invert=None, n_params=1, potential=None, reward=None, f32=False):
    """A script-defined model as the disk key has always spelt it, from _capi.model_check's arguments: the expressions in one
    string with a control character in front of each section (classes 1.. of a pool: every section, empty where not given)."""
    many = isinstance(sample, (list, tuple))
    n = len(sample) if many else 1
    col = lambda v: list(v) if many and v is not None else [v] + [None] * (n - 1)
    sample, logq, perform, invert = col(sample), col(logq), col(perform), col(invert)
    partials = list(dlogq) if n_params > 1 and dlogq is not None else None          # one policy with several parameters
    dlogq = col(dlogq) if partials is None else [partials[0]]
    t = ("\x02" if f32 else "") + (potential or "x*x") + ("\x01" + reward if reward else "")
    t += "\x04" + sample[0] + "\x05" + logq[0]
    if dlogq[0]:
        t += "\x06" + ("\x0b".join(partials) if partials else dlogq[0])
    if perform[0]:
        t += "\x07" + perform[0] + "\x08" + invert[0]
    if n_params > 1:
        t += "\x0e%d" % n_params
    if n > 1:
        t += "\x0f%d" % n
        for c in range(1, n):
            t += "\x10" + sample[c] + "\x11" + logq[c] + "\x12" + (dlogq[c] or "") + "\x13" + (perform[c] or "") + "\x14" + (invert[c] or "")
    return t


_LOGQ = "-(delta*delta)/(2.0*(sigma*sigma)) - amc_log(sigma)"
_DLOGQ = "(delta*delta)/(sigma*sigma*sigma) - 1.0/sigma"
_LOGQ2 = "-((delta - theta1*x)*(delta - theta1*x))/(2.0*(theta0*theta0)) - amc_log(theta0)"
_DLOGQ2 = ["((delta - theta1*x)*(delta - theta1*x))/(theta0*theta0*theta0) - 1.0/theta0", "x*(delta - theta1*x)/(theta0*theta0)"]
_FIRST = dict(sample="sigma*z", logq=_LOGQ, dlogq=_DLOGQ, potential="x*x*x*x - 2.0*x*x", reward="-delta*delta - 0.25*x")
# (_capi.model_check's arguments, environment, the variant text: the default instantiation is an estimator form, built without
# Machine LICM under AMC_RTC_LICM=est-off and for policies of several parameters)
MODEL_CACHE_CASES = [
    (_FIRST, {}, ""),
    (dict(sample="sigma*z", logq=_LOGQ), {}, ""),
    (dict(sample="sigma*z", logq=_LOGQ, dlogq=_DLOGQ, perform="x + 0.5*delta", invert="-delta"), {}, ""),
    (dict(sample="theta1*x + theta0*z", logq=_LOGQ2, dlogq=_DLOGQ2, n_params=2), {}, " licm-off"),
    (dict(sample="theta1*x + theta0*z", logq=_LOGQ2, n_params=2), {}, " licm-off"),
    (dict(sample=["sigma*z", "0.5*sigma*z", "sigma*z - 0.125*x"], logq=[_LOGQ, "-2.0*(delta*delta)/(sigma*sigma) - amc_log(sigma)", _LOGQ],
          dlogq=[_DLOGQ, None, _DLOGQ], perform=[None, None, "x + 0.5*delta"], invert=[None, None, "-delta"], reward="-delta*delta"), {}, ""),
    (_FIRST, {"AMC_MODEL_CHECK_F32": "1"}, ""),
    (_FIRST, {"AMC_RTC_LICM": "est-off"}, " licm-off"),
]


def test_disk_cache_key_of_script_models_is_unchanged(tmp_path):
    """The same for script-defined models (amc_model_check): one class with and without its derivative, with an action, several
    parameters, a pool of classes, Float32 state -- each found under the name its control-character spelling hashes to."""
    major, minor = _hiprtc_version()
    inst = "amc::pg_estimate_kernel<2,1,false,0,0,false>"
    dirs = []
    for i, (model, env, variant) in enumerate(MODEL_CACHE_CASES):
        d = tmp_path / str(i)
        d.mkdir()
        text = _model_text(f32=env.get("AMC_MODEL_CHECK_F32") == "1", **model)
        name = _cache_name(text, inst, "gfx950", "hiprtc %d.%d%s" % (major, minor, variant))
        lowered, code = b"planted", b"not a code object"
        (d / name).write_bytes(struct.pack("<3Q", 0x31435452434d41, len(lowered), len(code)) + lowered + code)
        dirs.append((str(d), env, name, model))
    script = """
import os, sys
sys.path.insert(0, %r)
from montecarlo_amd import _capi
for d, env, name, model in %r:
    for k in ("AMC_MODEL_CHECK_F32", "AMC_MODEL_CHECK_INST", "AMC_NO_SIGMA_MEMO", "AMC_NO_GAUSS_CLASS_ROWS", "AMC_RTC_WAVES", "AMC_RTC_LICM"):
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["AMC_RTC_CACHE_DIR"] = d
    assert _capi.model_check(**model) == ""
    print(d, sorted(os.listdir(d)) == [name], flush=True)
""" % (ROOT, dirs)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(dirs)
    for (d, env, name, model), line in zip(dirs, lines):
        assert line == d + " True", (model, env, sorted(os.listdir(d)), name)


@pytest.mark.gpu
def test_handle_knobs_are_read_at_create(gpu, monkeypatch):
    """AMC_NO_SWEEP_ESTIMATOR_FUSION counts as the handle found it: set after creation it changes nothing, set before it
    keeps the sweep out of the estimator launch (amc_pg_route: 2 fused, 1 not)."""
    kw = dict(n_chains=4099, potential="harmonic", beta=2.0, sigma=[0.2], weight=[1.0], seed=7)
    monkeypatch.delenv("AMC_NO_SWEEP_ESTIMATOR_FUSION", raising=False)
    e = gpu.HipEngine(device=0, **kw)
    monkeypatch.setenv("AMC_NO_SWEEP_ESTIMATOR_FUSION", "1")
    assert e.pg_route_code(1, 1, fused=True)[0] == 2
    e.close()
    e = gpu.HipEngine(device=0, **kw)
    assert e.pg_route_code(1, 1, fused=True)[0] == 1
    monkeypatch.delenv("AMC_NO_SWEEP_ESTIMATOR_FUSION")
    assert e.pg_route_code(1, 1, fused=True)[0] == 1
    e.close()
