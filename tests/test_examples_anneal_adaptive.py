"""examples/pa_double_well.py --adaptive end to end on the device at reduced length (as tests/test_examples_anneal.py runs the
scheduled form)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def test_pa_double_well_example_adaptive(gpu, tmp_path, capsys):
    import pa_double_well as ex
    ends, exact, tol, done = ex.main(["--chains", "8192", "--stages", "30", "--sweeps", "5", "--runs", "4", "--adaptive", "0.8",
                                      "--path", str(tmp_path / "pa")])
    out = capsys.readouterr().out
    print(out)
    assert "quadrature" in out and "ESS / M kept" in out and "rho_t" in out
    # log Z(8) / Z(0.5) within the tolerance the example prints (8 standard errors of its 4 runs)
    assert ends.shape == (4,) and abs(ends.mean() - exact) <= tol < 0.1, (ends, exact, tol)
    # the last run's own steps: cooling all the way to the end, in fewer steps than were allowed
    assert 3 <= len(done) < 30 and np.all(np.diff(np.concatenate([[0.5], done])) > 0.0) and done[-1] == 8.0
    text = open(tmp_path / "pa" / "run0" / "summary.log").read()
    assert "PopulationAnnealing\n\t\tCalls: 30\n\t\tBetas: adaptive, ESS / M >= 0.8 per step, to 8.0 (6 rounds)" in text
    rows = open(tmp_path / "pa" / "run3" / "anneal_beta.dat").read().splitlines()
    assert float(rows[-1].split()[-1]) == 8.0
