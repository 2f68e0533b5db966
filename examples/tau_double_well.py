#!/usr/bin/env python3
"""How fast does the energy decorrelate?  tau_int per rung of the double-well ladder, measured on the device.

The ladder of examples/pt_double_well.py, started in equilibrium-like conditions by a burn-in with exchange steps; then one time
origin is marked and the energy of every chain is correlated with its value at the origin over ``--lags`` lags ``--every`` MH steps
apart (Autocorrelation: one word per chain and one memory-bound pass per lag on the device, no position leaves it).  The same
schedule runs with and without exchange steps: the series of RUNG r decorrelates faster when replicas from hotter rungs pass through
it, and tau_int -- the number of MH steps between two samples that count as independent -- says by how much.

    python examples/tau_double_well.py [--ladders 16384] [--burn 500] [--every 2] [--lags 100] [--origins 2] [--path data/TAU/...]
                                       [--blocks 32]
    python examples/tau_double_well.py --anneal

--anneal: population annealing instead (examples/pa_double_well.py's schedule): the population is cooled to the last beta, then an
origin is marked and tau_int of the energy at that beta is printed -- what the sweeps between two annealing steps have to cover.

--blocks B keeps the sums per block of ladders (Autocorrelation(..., blocks=B)) and prints the standard error of every tau_int from a
delete-one-block jackknife over the B blocks, each replicate with its own automatic window.  Not with --anneal: resampling makes
copies of one parent share blocks.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlo_amd as ma   # noqa: E402

BETAS = (0.5, 1.0, 2.0, 4.0, 8.0)
SIGMA0 = 0.3


def corr_schedule(args):
    """One call per slot: a mark and ``lags`` samples per origin, the origins back to back behind the burn-in."""
    n = args.origins * (args.lags + 1)
    return [args.burn + args.every * (k + 1) for k in range(n)]


def ladder_run(args, path, exchange: bool):
    R, L = len(BETAS), args.ladders
    sched = corr_schedule(args)
    x0 = np.where(np.arange(R * L) // R % 2 == 0, 1.0, -1.0) * (0.8 + 0.4 * ((np.arange(R * L) * 0.6180339887498949) % 1.0))
    chains = ma.ParticleChains.ladder(L, BETAS, potential="double_well", x=x0)
    pool = (ma.Move(ma.Displacement(0.0), ma.StandardGaussian(), [SIGMA0], 1.0),)
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=args.seed)]
    # the burn-in always exchanges (both runs start from the same kind of ensemble); afterwards only the run that is asked to
    x_sched = range(1, sched[-1] + 1) if exchange else range(1, args.burn + 1)
    al.append(dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=list(x_sched)))
    al.append(dict(algorithm=ma.Autocorrelation, dependencies=(ma.Metropolis,), scheduler=sched, observable="energy", n_lags=args.lags,
                   origins=args.origins, blocks=args.blocks))
    sim = ma.Simulation(chains, al, sched[-1], path=path)
    ma.run(sim)
    return sim.algorithms[2]


def anneal_run(args, path):
    betas = list(np.linspace(0.5, 8.0, 31))
    sched = corr_schedule(args)
    chains = ma.ParticleChains.uniform(args.ladders * len(BETAS), betas[0], potential="double_well")
    pool = (ma.Move(ma.Displacement(0.0), ma.StandardGaussian(), [SIGMA0], 1.0),)
    every = max(1, args.burn // (len(betas) - 1))
    al = [dict(algorithm=ma.Metropolis, pool=pool, seed=args.seed),
          dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), betas=betas[1:],
               scheduler=[every * (k + 1) for k in range(len(betas) - 1)]),
          dict(algorithm=ma.Autocorrelation, dependencies=(ma.Metropolis,), scheduler=sched, observable="energy", n_lags=args.lags,
               origins=args.origins)]
    sim = ma.Simulation(chains, al, sched[-1], path=path)
    ma.run(sim)
    return sim.algorithms[2], sim.algorithms[1].beta


def row(label, values, fmt="{:9.2f}"):
    print(f"{label:34s}: " + "  ".join(fmt.format(v) for v in values))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ladders", type=int, default=16384)
    ap.add_argument("--burn", type=int, default=500, help="time steps before the first origin")
    ap.add_argument("--every", type=int, default=2, help="MH steps between two lags")
    ap.add_argument("--lags", type=int, default=100)
    ap.add_argument("--origins", type=int, default=2)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--path", default=None)
    ap.add_argument("--anneal", action="store_true", help="tau_int at the final beta of a population-annealing run instead")
    ap.add_argument("--blocks", type=int, default=None, metavar="B", help="print tau_int +- its jackknife standard error over B blocks of ladders")
    args = ap.parse_args(argv)
    if args.blocks is not None and args.anneal:
        ap.error("--blocks does not go with --anneal: resampling makes copies of one parent share blocks")
    path = args.path or f"data/TAU/particle_1d/DoubleWell/L{args.ladders}/seed{args.seed}"
    if args.anneal:
        ac, beta = anneal_run(args, os.path.join(path, "anneal"))
        tau, window, converged = ac.tau_int()
        print(f"population annealing to beta = {beta}: tau_int(energy) = {tau[0]:.2f} MH steps (window {window[0]} lags of {args.every} steps, "
              f"{'converged' if converged[0] else 'NOT converged: more lags'})")
        return tau
    with_x = ladder_run(args, os.path.join(path, "exchange"), True)
    without = ladder_run(args, os.path.join(path, "plain"), False)
    row("beta", BETAS)
    if args.blocks:
        tau_x, se_x, win_x, ok_x = with_x.tau_int(error=True)
        tau_p, se_p, win_p, ok_p = without.tau_int(error=True)
        row("tau_int(energy), with exchange", tau_x)
        row(f"  +- se ({args.blocks} blocks)", se_x)
        row("tau_int(energy), without", tau_p)
        row(f"  +- se ({args.blocks} blocks)", se_p)
    else:
        tau_x, win_x, ok_x = with_x.tau_int()
        tau_p, win_p, ok_p = without.tau_int()
        row("tau_int(energy), with exchange", tau_x)
        row("tau_int(energy), without", tau_p)
    row("window (lags), with / without", [f"{a}/{b}" for a, b in zip(win_x, win_p)], "{:>9s}")
    if not (ok_x.all() and ok_p.all()):
        print("(a window reached the last lag: that tau_int is a lower bound; run with more --lags or a larger --every)")
    return tau_x, tau_p


if __name__ == "__main__":
    main()
