"""The handle's grouped state (amc_internal.h): LadderState and AnnealState each have one release function that frees every device
pointer the struct declares, and amc_destroy calls both -- a buffer added to a struct later cannot be forgotten at destroy.  Reads
the sources only: no library, no device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo_amd", "csrc")

# (struct, its release function)
STATES = [("LadderState", "ladder_release"), ("AnnealState", "anneal_release")]


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _braces(text, start):
    """The text between the brace that opens at or after `start` and the one that closes it."""
    a = text.index("{", start)
    depth = 0
    for i in range(a, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[a + 1:i]
    raise AssertionError("unbalanced braces")


def _code(text):
    return re.sub(r"//[^\n]*", "", text)


def _device_pointers(struct):
    body = _code(_braces(_read("amc_internal.h"), _read("amc_internal.h").index("struct %s {" % struct)))
    return re.findall(r"\*\s*(d_\w+)\s*=\s*nullptr\s*;", body)


def _release_body(struct, release):
    header = _read("amc_internal.h")
    m = re.search(r"\bvoid %s\(%s& (\w+)\)" % (release, struct), header)
    assert m, "%s(%s&) is not in amc_internal.h" % (release, struct)
    return m.group(1), _code(_braces(header, m.end()))


@pytest.mark.parametrize("struct,release", STATES)
def test_release_frees_every_device_pointer(struct, release):
    pointers = _device_pointers(struct)
    assert len(pointers) >= 8, (struct, pointers)                  # the pattern above still finds the members
    assert len(pointers) == len(set(pointers))
    # ... and misses none: every d_* name in the struct is a pointer member it found
    body = _code(_braces(_read("amc_internal.h"), _read("amc_internal.h").index("struct %s {" % struct)))
    assert set(re.findall(r"\b(d_\w+)\s*=", body)) == set(pointers)
    arg, text = _release_body(struct, release)
    freed = re.findall(r"hipFree\(%s\.(\w+)\)" % arg, text)
    assert sorted(freed) == sorted(pointers), (struct, sorted(set(pointers) ^ set(freed)))


def test_destroy_calls_both_release_functions():
    header, api = _read("amc_internal.h"), _code(_read("amc_api.hip"))
    handle = _code(_braces(header, header.index("struct amc_handle {")))
    destroy = _braces(api, api.index("int amc_destroy(amc_handle* h)"))
    for struct, release in STATES:
        m = re.search(r"^\s*%s (\w+);" % struct, handle, re.M)
        assert m, "amc_handle holds no %s by value" % struct
        assert re.search(r"\b%s\(h->%s\);" % (release, m.group(1)), destroy), "amc_destroy does not call %s" % release
