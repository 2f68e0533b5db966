"""CorrState (amc_internal.h) under the rules tests/test_handle_state_static.py holds LadderState and AnnealState to: its one release
function frees every device pointer the struct declares, and amc_destroy calls it.  Reads the sources only: no library, no device."""
import re

from test_handle_state_static import _braces, _code, _device_pointers, _read, _release_body


def test_corr_release_frees_every_device_pointer():
    pointers = _device_pointers("CorrState")
    assert sorted(pointers) == ["d_corr", "d_origin"]
    arg, text = _release_body("CorrState", "corr_release")
    assert sorted(re.findall(r"hipFree\(%s\.(\w+)\)" % arg, text)) == sorted(pointers)


def test_destroy_releases_and_every_slot_reassignment_forgets():
    header, api = _read("amc_internal.h"), _code(_read("amc_api.hip"))
    assert re.search(r"^\s*CorrState corr;", _code(_braces(header, header.index("struct amc_handle {"))), re.M)
    assert "corr_release(h->corr);" in _braces(api, api.index("int amc_destroy(amc_handle* h)"))
    for unit, entry in (("amc_state.hip", "int amc_upload_state("), ("amc_state.hip", "int amc_init_uniform("),
                        ("amc_anneal.hip", "int amc_anneal("), ("amc_exchange.hip", "static int ladder_reset(")):
        text = _code(_read(unit))
        assert "corr_forget(h);" in _braces(text, text.index(entry)), entry
