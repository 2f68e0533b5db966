"""examples/pt_double_well.py --rung-sigma end to end on the device at reduced length: the widths and the move's acceptance per rung are
printed beside the swap acceptance, and without the flag the output has neither line."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def numbers(out, label):
    rows = [ln for ln in out.splitlines() if ln.startswith(label)]
    assert len(rows) == 1, (label, out)
    return np.array([float(v) for v in rows[0].split(":")[1].split()])


def test_pt_double_well_example_with_widths_per_rung(gpu, tmp_path, capsys):
    import pt_double_well as ex
    sim, left, left_plain, accept = ex.main(["--ladders", "1024", "--steps", "200", "--path", str(tmp_path / "pt"), "--rung-sigma"])
    out = capsys.readouterr().out
    met = sim.algorithms[0]
    want = ex.SIGMA0 * np.sqrt(ex.BETAS[0] / np.array(ex.BETAS))
    assert np.array_equal(met.engine.rung_sigma(), want.reshape(1, -1))
    assert np.allclose(numbers(out, "proposal width per rung"), want, atol=5e-5)
    acc = numbers(out, "move acceptance per rung")
    assert np.allclose(acc, met.rung_acceptance()[0], atol=5e-5) and np.all((acc > 0.0) & (acc < 1.0))
    assert numbers(out, "swap acceptance per gap").shape == (4,) and accept.shape == (4,)
    ex.main(["--ladders", "1024", "--steps", "20", "--path", str(tmp_path / "plain")])
    out = capsys.readouterr().out
    assert "swap acceptance per gap" in out and "per rung  " not in out and "move acceptance" not in out
