"""examples/pt_double_well.py end to end on the device at reduced length (as tests/test_examples.py runs the other drivers)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def test_pt_double_well_example(gpu, tmp_path, capsys):
    import pt_double_well as ex
    sim, left, left_plain, accept = ex.main(["--ladders", "4096", "--steps", "600", "--path", str(tmp_path / "pt")])
    out = capsys.readouterr().out
    assert "swap acceptance per gap" in out and "coldest rung" in out
    # the hottest rung crosses the barrier with or without exchanges; the coldest one only with them
    assert abs(left[0] - 0.5) < 0.05 and abs(left_plain[0] - 0.5) < 0.05
    assert left[-1] > 0.3 and left_plain[-1] < 0.1
    assert np.all((accept > 0.05) & (accept < 0.95))
    text = open(tmp_path / "pt" / "exchange" / "summary.log").read()
    assert "ReplicaExchange\n\t\tCalls: 600\n\t\tRungs: 5\n\t\tLadders: 4096" in text
    rows = open(tmp_path / "pt" / "exchange" / "exchange_acceptance.dat").read().splitlines()
    assert rows[0] == "0 [NaN, NaN, NaN, NaN]" and rows[-1].startswith("600 [")
