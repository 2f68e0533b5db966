"""examples/pa_double_well.py end to end on the device at reduced length (as tests/test_examples.py runs the other drivers)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def test_pa_double_well_example(gpu, tmp_path, capsys):
    import pa_double_well as ex
    mean, exact, tol, survival, rho, left = ex.main(["--chains", "8192", "--stages", "12", "--sweeps", "5", "--path", str(tmp_path / "pa")])
    out = capsys.readouterr().out
    print(out)
    assert "quadrature" in out and "rho_t" in out
    # log Z(beta) / Z(0.5) at every annealing temperature within the tolerance the example prints (8 standard errors of its 8 runs)
    assert mean.shape == exact.shape == (12,) and np.all(np.abs(mean - exact) <= tol), (mean - exact, tol)
    assert np.all(np.diff(exact) < 0.0) and np.all(tol < 0.05)
    assert np.all((survival > 0.3) & (survival <= 1.0)) and 1.0 <= rho < 8192 / 8
    assert 0.2 < left < 0.8                      # both wells stay populated down to beta = 8: the population was cooled, not quenched
    text = open(tmp_path / "pa" / "run0" / "summary.log").read()
    assert "PopulationAnnealing\n\t\tCalls: 12\n\t\tBetas: 12 from" in text and "Families: true" in text
    rows = open(tmp_path / "pa" / "run0" / "anneal_beta.dat").read().splitlines()
    assert len(rows) >= 12 and rows[-1].split()[0] == str(200 + 11 * 5) and float(rows[-1].split()[-1]) == 8.0
