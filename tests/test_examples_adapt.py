"""examples/pt_double_well.py --adapt flow end to end on the device at reduced length (as tests/test_examples_exchange.py runs the
plain example): the ladder is respaced during the first half and left alone afterwards."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def test_pt_double_well_adapt_flow(gpu, tmp_path, capsys):
    import pt_double_well as ex
    sim, left, left_plain, accept = ex.main(["--ladders", "2048", "--steps", "400", "--adapt", "flow", "--path", str(tmp_path / "pt")])
    out = capsys.readouterr().out
    assert "ladder after 5 respacings" in out and "flow fraction f(r)" in out and "round trips per ladder" in out
    rx, rl = sim.algorithms[1], sim.algorithms[2]
    assert [t for t, _ in rl.statuses] == [40, 80, 120, 160, 200] and all(s == 0 for _, s in rl.statuses)
    lad = rx.betas()
    assert lad[0] == ex.BETAS[0] and lad[-1] == ex.BETAS[-1] and np.all(np.diff(lad) > 0) and not np.array_equal(lad, ex.BETAS)
    assert np.array_equal(sim.chains.beta_array, np.tile(lad, 2048))
    # the counters were zeroed by the last respacing, at step 200: what is printed is the second half
    acc, att = rx.metropolis.engine.exchange_counters()
    assert att.tolist() == [100 * 2048] * 4 and np.array_equal(accept, acc / att) and np.all((accept > 0.0) & (accept <= 1.0))
    assert left[-1] > left_plain[-1] and left_plain[-1] < 0.1  # the coldest rung still crosses the barrier only with exchanges
    text = open(tmp_path / "pt" / "exchange" / "summary.log").read()
    assert "RespaceLadder\n\t\tCalls: 5\n\t\tRule: flow" in text
    rows = open(tmp_path / "pt" / "exchange" / "ladder.dat").read().splitlines()
    assert rows[0].startswith("0 [0.5, 1.0, 2.0, 4.0, 8.0]") and rows[-1].startswith("400 [0.5, ")
