"""examples/rhat_double_well.py end to end at a toy size on the twin engine (tests/chain_stats_twin.py): no GPU."""
import os
import sys

import numpy as np

import chain_stats_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def test_rhat_double_well_example(oracle, amc, tmp_path, capsys):
    import rhat_double_well as ex
    out = ex.main(["--ladders", "64", "--burn", "20", "--every", "2", "--samples", "16", "--path", str(tmp_path / "rhat")],
                  engine_factory=T.ChainStatsLadderEngine)
    text = capsys.readouterr().out
    assert "swap acceptance per gap" in text and "R-hat(x), without" in text and "R-hat(energy), with exchange" in text
    for key in ((True, "x"), (False, "x"), (True, "energy"), (False, "energy")):
        assert out[key].shape == (5,) and np.all(np.isfinite(out[key])) and np.all(out[key] > 0.9)
    # the coldest rung without exchange steps: the wells are 2 apart, a chain moves by about 1/8 around its own -- far from converged
    # in x, while its energy looks fine
    assert out[False, "x"][-1] > 2.0 and out[False, "energy"][-1] < 1.5
    assert out[False, "x"][-1] > out[False, "x"][0]
    log = open(tmp_path / "rhat" / "plain" / "x" / "summary.log").read()
    assert "Convergence\n\t\tCalls: 16\n\t\tObservable: x\n\t\tSamples: 16" in log
