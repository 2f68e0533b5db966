"""examples/pt_double_well.py --tune-sigma 0.5 end to end on the device at reduced length (as tests/test_examples_adapt.py runs
--adapt): the widths per rung are tuned during the first half and left alone afterwards."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def test_pt_double_well_tune_sigma(gpu, tmp_path, capsys):
    import pt_double_well as ex
    sim, left, left_plain, accept = ex.main(["--ladders", "2048", "--steps", "400", "--tune-sigma", "0.5", "--path", str(tmp_path / "pt")])
    out = capsys.readouterr().out
    met, tune = sim.algorithms[0], sim.algorithms[2]
    assert [t for t, _ in tune.statuses] == list(range(20, 201, 20)) and all(np.all(s == 0) for _, s in tune.statuses)
    row = lambda label: [float(v) for v in re.search(label + r"\s*:\s*(.*)", out).group(1).split()]
    table, window = row("width per rung, 10 tunings"), row("acceptance since the last one")
    assert len(table) == len(window) == len(ex.BETAS)
    assert np.allclose(table, met.rung_sigma[0], atol=5e-5) and np.all(np.diff(table) < 0)          # sigma falls as beta rises
    assert all(0.0 < a < 1.0 for a in window)
    # the window is the second half: 200 sweeps of 2048 ladders under the final table
    assert np.all(met.engine.rung_window_counts()[1] == 200 * 2048)
    text = open(tmp_path / "pt" / "exchange" / "summary.log").read()
    assert "TuneRungSigma\n\t\tCalls: 10\n\t\tTarget: 0.5" in text
    rows = open(tmp_path / "pt" / "exchange" / "rung_sigma.dat").read().splitlines()
    assert rows[0].startswith("0 ") and "0.3" in rows[0] and rows[-1].startswith("400 ")
