"""The checkpoint file, section by section, on the engine doubles: which keys a configuration writes, with which dtype and shape; that
a file written before storage.py was split into sections restores and continues bit for bit; that the file written now holds the
same bits under every key.

Every configuration has 12 chains and K = 2 moves; the ladders have R = 3 rungs (4 ladders) and are checkpointed after 3 exchange
steps, so both gap parities have run.  Between them the configurations turn on every section a double offers: core, counters, ladder,
widths per rung, window (with and without a table), tracking, annealing (with and without families), estimator.  No double has the
bridge sums or the respacing: tests/test_gpu_checkpoint_all_sections.py resumes those on the device.

SCHEMA and tests/golden/checkpoints/<configuration>.npz were written by ``first_half`` below run against the commit before the split
(``python tests/test_checkpoint_schema.py <directory>`` with that commit's package first on the path writes both).
"""
import os
import shutil
import sys

import numpy as np
import pytest

import montecarlo_amd as ma

import anneal_twin as A
import exchange_twin as X
import track_twin as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "checkpoints")
N = 6                                      # time steps per half: an exchange / annealing step at every second one
TAB = np.array([[0.5, 0.4, 0.3], [0.2, 0.15, 0.1]])
BETAS = [0.5, 0.7, 1.0, 1.4, 2.0, 2.8, 4.0]


def _pool():
    return (ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.5], 0.625), ma.Move(ma.Displacement(), ma.StandardGaussian(), [0.2], 0.375))


class RestartWindow(ma.AriannaAlgorithm):
    def __init__(self, chains, dependencies=None, **extras):
        self.metropolis = dependencies[0]

    def make_step(self, simulation):
        self.metropolis.restart_rung_window()


def _ladder(factory, tab=None, track=False, tune=False, window=False):
    def build(path, steps, resumed):
        chains = ma.ParticleChains.ladder(4, [0.5, 1.0, 2.0], x=np.linspace(-1.5, 1.5, 12))
        al = [dict(algorithm=ma.Metropolis, pool=_pool(), seed=7, engine_factory=factory, rung_sigma=tab),
              dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), track=track)]
        if tune and not resumed:           # one tuning, in the first half
            al.append(dict(algorithm=ma.TuneRungSigma, dependencies=(ma.Metropolis,), scheduler=[3], target=0.5, min_calls=1))
        if window and not resumed:         # a window restart without a table: the window's base and no count of tunings
            al.append(dict(algorithm=RestartWindow, dependencies=(ma.Metropolis,), scheduler=[3]))
        return ma.Simulation(chains, al, steps, path=str(path)), None
    return build


def _anneal(families):
    def build(path, steps, resumed):
        chains = ma.ParticleChains.uniform(12, BETAS[0], potential="double_well")
        al = [dict(algorithm=ma.Metropolis, pool=_pool(), seed=4, engine_factory=A.AnnealTwinEngine),
              dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=ma.build_schedule(steps, 0, 2), betas=BETAS[1:],
                   families=families)]
        return ma.Simulation(chains, al, steps, path=str(path)), None
    return build


def _estimator(path, steps, resumed):
    import oracle_lib
    chains = ma.ParticleChains.uniform(12, 2.0)
    al = [dict(algorithm=ma.Metropolis, pool=_pool(), seed=11, engine_factory=oracle_lib.OracleEngine),
          dict(algorithm=ma.PolicyGradientEstimator, dependencies=(ma.Metropolis,), optimisers=(ma.Static(), ma.VPG(0.05))),
          dict(algorithm=ma.PolicyGradientUpdate, dependencies=(ma.PolicyGradientEstimator,))]
    sim = ma.Simulation(chains, al, steps, path=str(path))
    return sim, sim.algorithms[1]


def _configurations():
    from test_rung_sigma_host import TableEngine
    from test_tune_host import TuneEngine
    return {"estimator": _estimator, "ladder": _ladder(X.TwinEngine), "tracking": _ladder(T.TrackEngine, track=True),
            "widths": _ladder(TableEngine, tab=TAB), "tuned": _ladder(TuneEngine, tab=TAB, tune=True),
            "window": _ladder(TuneEngine, window=True), "annealing": _anneal(False), "families": _anneal(True)}


NAMES = ["estimator", "ladder", "tracking", "widths", "tuned", "window", "annealing", "families"]

_CORE = {"x": ("float64", (12,)), "shard": ("int64", (2,)), "n_chains_global": ("int64", ()), "seed": ("int64", ()),
         "sweepstep": ("int64", ()), "step": ("int64", ()), "estimator_step": ("int64", ()), "sigma": ("float64", (2,)),
         "weight": ("float64", (2,)), "param_dtype": ("<U3", ()), "accepted_total": ("int64", (2,)), "total_total": ("int64", (2,)),
         "accepted": ("int64", (2, 12)), "total": ("int64", (2, 12))}
_LADDER = dict(_CORE, beta=("float64", (12,)), n_rungs=("int64", ()), exchange_step=("int64", ()), exchange_accepted=("int64", (2,)),
               exchange_attempted=("int64", (2,)))
_WINDOW = {"rung_window_accepted": ("int64", (2, 3)), "rung_window_total": ("int64", (2, 3))}
_ANNEAL = dict(_CORE, anneal_beta=("float64", ()), anneal_step=("int64", ()), anneal_records=("uint64", (3, 8)))
SCHEMA = {
    "estimator": dict(_CORE, gd=("float64", (1, 5))),
    "ladder": _LADDER,
    "tracking": dict(_LADDER, walker=("uint8", (12,)), direction=("uint8", (12,)), trips=("int64", (2,))),
    "widths": dict(_LADDER, rung_sigma=("float64", (2, 3))),
    "tuned": dict(_LADDER, rung_sigma=("float64", (2, 3)), n_tuned=("int64", ()), **_WINDOW),
    "window": dict(_LADDER, **_WINDOW),
    "annealing": _ANNEAL,
    "families": dict(_ANNEAL, families=("uint32", (12,))),
}


def first_half(name, path):
    """N time steps of the configuration, then its checkpoint: the file's name."""
    sim, est = _configurations()[name](os.path.join(path, "a"), N, False)
    ma.run(sim)
    return ma.checkpoint(sim.algorithms[0], os.path.join(path, "ck"), estimator=est)


def schema(d):
    return {k: (str(d[k].dtype), tuple(d[k].shape)) for k in d.files}


def same_bits(a, b):
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def written(oracle, tmp_path_factory):
    """The checkpoint every configuration writes after its first half, made once."""
    return {name: first_half(name, str(tmp_path_factory.mktemp(name))) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_keys_dtypes_and_shapes(written, name):
    assert schema(np.load(written[name])) == SCHEMA[name]


@pytest.mark.parametrize("name", NAMES)
def test_the_file_holds_the_bits_it_held_before_the_split(written, name):
    same_bits(np.load(written[name]), np.load(os.path.join(GOLDEN, name + ".npz")))


@pytest.mark.parametrize("name", NAMES)
def test_a_file_from_before_the_split_restores_and_continues(oracle, tmp_path, name):
    build = _configurations()[name]
    whole, est_w = build(tmp_path / "w", 2 * N, False)
    ma.run(whole)
    os.makedirs(tmp_path / "ck")
    shutil.copy(os.path.join(GOLDEN, name + ".npz"), tmp_path / "ck" / "checkpoint_rank0.npz")
    second, est_s = build(tmp_path / "b", N, True)
    ma.restore(second.algorithms[0], str(tmp_path / "ck"), estimator=est_s)
    ma.run(second)
    # every field of state at the end, through the checkpoint both would write
    same_bits(np.load(ma.checkpoint(second.algorithms[0], str(tmp_path / "ck_b"), estimator=est_s)),
              np.load(ma.checkpoint(whole.algorithms[0], str(tmp_path / "ck_w"), estimator=est_w)))
    assert np.array_equal(second.chains.x.view(np.uint64), whole.chains.x.view(np.uint64))


if __name__ == "__main__":                 # regenerate the golden files and print the table (see the module's docstring)
    import tempfile
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    for name in NAMES:
        fn = first_half(name, tempfile.mkdtemp())
        shutil.copy(fn, os.path.join(out, name + ".npz"))
        print(name, schema(np.load(fn)))
