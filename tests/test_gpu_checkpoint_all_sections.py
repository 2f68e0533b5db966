"""checkpoint / restore with every section of the file on at once, on the device: one handle with a ladder, widths per rung, a tuned
window, walker tracking, the bridge sums and one respacing.  The other resume tests turn these on one at a time; what this one adds
is the order restore applies them in (ladder, table, labels, window, bridge records, respacing count).  A second case resumes a
population annealing with families.

4 ladders of R = 4 (16 chains), K = 2 moves.  A round is 2 sweeps and 1 exchange step; 6 rounds with a tuning behind the second and a
respacing behind the fourth, checkpoint, restore into a fresh Metropolis, 6 more rounds: bit-equal to 12 uninterrupted rounds."""
import numpy as np
import pytest

import montecarlo_amd as ma

from test_gpu_exchange import bits, start_state

pytestmark = pytest.mark.gpu
R, L = 4, 4
START = [0.6, 0.7, 0.85, 2.4]
TAB = np.array([[0.9, 0.8, 0.7, 0.4], [0.3, 0.25, 0.2, 0.1]])
ROUND = 2                                  # time steps per round: a sweep at each, an exchange step at the second


def build(path, rounds, dtype, burn_in):
    chains = ma.ParticleChains.ladder(L, START, x=start_state(R, R * L)[0], potential="double_well", dtype=dtype)
    pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 0.625), ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.2], 0.375))
    steps = ROUND * rounds
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=4, rung_sigma=TAB),
          dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, ROUND), track=True,
               bridge=True)]
    if burn_in:                            # the first half's: a tuning behind round 2, a respacing behind round 4
        al += [dict(algorithm=ma.TuneRungSigma, dependencies=(ma.Metropolis,), scheduler=[2 * ROUND], target=0.5, gamma=0.5, min_calls=1),
               dict(algorithm=ma.RespaceLadder, dependencies=(ma.ReplicaExchange,), scheduler=[4 * ROUND], rule="acceptance", gamma=0.9,
                    eps=0.1)]
    return ma.Simulation(chains, al, steps, path=str(path))


def state(sim):
    met, rx = sim.algorithms[0], sim.algorithms[1]
    eng = met.engine
    x, e = eng.download_state()
    rec, n_snap = eng.bridge_fetch(reset=False)
    return [bits(sim.chains.x), bits(x), bits(e), *eng.download_counters(), *eng.exchange_counters(), *eng.labels(),
            np.array(eng.tracking_counters()), bits(eng.rung_sigma()), bits(met.rung_sigma), *eng.rung_window_base(),
            bits(eng.ladder()), bits(sim.chains.beta_array), bits(rec),
            np.array([n_snap, eng.exchange_step, eng.step, eng.tune_status()[1], *eng.respace_status()])]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def same_file(a, b):
    return sorted(a.files) == sorted(b.files) and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a.files)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_ladder_section_at_once(gpu, tmp_path, dtype):
    whole = build(tmp_path / "w", 12, dtype, True)
    ma.run(whole)
    first = build(tmp_path / "a", 6, dtype, True)
    ma.run(first)
    saved = np.load(ma.checkpoint(first.algorithms[0], str(tmp_path / "ck")))
    # every section is in the file, and each is in use: a tuned table, a ladder that moved, records behind the respacing
    assert {"n_rungs", "rung_sigma", "rung_window_accepted", "n_tuned", "walker", "trips", "bridge_records", "n_respaced"} <= set(saved.files)
    assert int(saved["n_tuned"]) == 1 and int(saved["n_respaced"]) == 1 and int(saved["bridge_snapshots"]) == 2
    assert not np.array_equal(saved["rung_sigma"], TAB) and not np.array_equal(saved["beta"][:R], START) and int(saved["exchange_step"]) == 6
    second = build(tmp_path / "b", 6, dtype, False)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    assert same(state(whole), state(second))
    assert same_file(np.load(ma.checkpoint(whole.algorithms[0], str(tmp_path / "ck_w"))),
                     np.load(ma.checkpoint(second.algorithms[0], str(tmp_path / "ck_b"))))


def test_annealing_with_families(gpu, tmp_path):
    betas = [0.5, 0.7, 1.0, 1.4, 2.0, 2.8, 4.0]

    def anneal(path, steps):
        chains = ma.ParticleChains.uniform(16, betas[0], potential="double_well")
        pool = (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 0.625), ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.2], 0.375))
        al = [dict(algorithm=ma.Metropolis, pool=pool, seed=4),
              dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), betas=betas[1:],
                   families=True)]
        return ma.Simulation(chains, al, steps, path=str(path))
    whole, first, second = anneal(tmp_path / "w", 12), anneal(tmp_path / "a", 6), anneal(tmp_path / "b", 6)
    ma.run(whole)
    ma.run(first)
    saved = np.load(ma.checkpoint(first.algorithms[0], str(tmp_path / "ck")))
    assert int(saved["anneal_step"]) == 3 and saved["anneal_records"].shape == (3, 8) and saved["families"].shape == (16,)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"))
    ma.run(second)
    e1, e2 = whole.algorithms[0].engine, second.algorithms[0].engine
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(e1.download_state(), e2.download_state()))
    assert np.array_equal(whole.algorithms[1].records(), second.algorithms[1].records()) and e1.anneal_step == e2.anneal_step == 6
    assert np.array_equal(e1.download_families(), e2.download_families()) and e1.beta == e2.beta == betas[6]
    assert same_file(np.load(ma.checkpoint(whole.algorithms[0], str(tmp_path / "ck_w"))),
                     np.load(ma.checkpoint(second.algorithms[0], str(tmp_path / "ck_b"))))
