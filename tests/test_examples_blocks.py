"""examples/pt_double_well.py --free-energy --blocks and examples/tau_double_well.py --blocks end to end on the device at reduced length:
every estimate is printed with a jackknife standard error, and the acceptance estimate lies within 5 of them of the quadrature."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
PAIR = r"(-?\d+\.\d+) \+- (\d+\.\d+)"


def test_pt_double_well_free_energy_with_blocks(gpu, tmp_path, capsys):
    import pt_double_well as ex
    ex.main(["--ladders", "4096", "--steps", "400", "--free-energy", "--blocks", "16", "--path", str(tmp_path / "pt")])
    out = capsys.readouterr().out
    rows = {line.split(":")[0].strip(): line for line in out.splitlines()}
    assert "jackknife se over 16 blocks" in out
    for label, n in (("acceptance (Bennett, C = 0)", 4), ("exponential, forward", 4), ("exponential, backward", 4), ("thermodynamic integration", 4),
                     ("log(Z_r / Z_0), acceptance", 5), ("heat capacity per rung", 5)):
        assert len(re.findall(PAIR, rows[label])) == n, rows[label]
    exact = np.array([float(v) for v in rows["quadrature"].split(":")[1].split()])
    got = np.array([[float(v), float(s)] for v, s in re.findall(PAIR, rows["acceptance (Bennett, C = 0)"])])
    assert np.all(got[:, 1] > 0) and np.all(np.abs(got[:, 0] - exact) <= 5.0 * got[:, 1] + 1e-4)      # (+ the last printed digit)


def test_tau_double_well_with_blocks(gpu, tmp_path, capsys):
    import tau_double_well as ex
    tau_x, tau_p = ex.main(["--ladders", "2048", "--burn", "100", "--lags", "30", "--origins", "1", "--blocks", "16", "--path", str(tmp_path / "tau")])
    out = capsys.readouterr().out
    se = [[float(v) for v in line.split(":")[1].split()] for line in out.splitlines() if "+- se (16 blocks)" in line]
    assert len(se) == 2 and all(len(r) == 5 for r in se) and np.all(np.array(se) > 0) and np.all(np.isfinite(tau_x))
    with pytest.raises(SystemExit):
        ex.main(["--anneal", "--blocks", "16"])
