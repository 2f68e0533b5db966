#!/usr/bin/env python3
"""Parallel tempering of the double well (x^2 - 1)^2 on one MI355X.

At beta = 8 a chain with a local Gaussian move stays in the well it starts in: <U> looks fine while the density is wrong.
A temperature ladder with neighbour swaps (ReplicaExchange) lets positions travel up to a rung that crosses the barrier and back
down.  Every chain starts in the right well; the script runs the same schedule with and without exchange steps and prints, per
rung, the fraction of chains left of the barrier, the mean energy and the swap acceptance of every gap.

    python examples/pt_double_well.py [--ladders 16384] [--steps 2000] [--path data/PT/...] [--track] [--rung-sigma] [--adapt flow|acceptance]
                                          [--tune-sigma TARGET] [--free-energy] [--reweight N] [--moments] [--blocks 32]

--track also follows every replica through the swaps and prints, at the end, the flow fraction f(r) -- of the replicas at rung r that
have been to an end of the ladder, the share that came from the hot end (rung 0) last -- and the round trips per ladder.

--rung-sigma gives every rung a proposal width of its own, sigma_r = sigma_0 sqrt(beta_0 / beta_r) (Metropolis(..., rung_sigma=...)): the
hot rungs then take the long steps they are there for.  The acceptance of the move per rung is printed beside the swap acceptance.

--adapt flow|acceptance respaces the ladder on the device during the first half of the run (RespaceLadder, five damped respacings, the
last at steps / 2; "flow" turns tracking on) and leaves it alone afterwards -- moving beta breaks detailed balance, so the first half is
burn-in.  A respacing zeroes the gap counters and restarts the tracking, so the swap acceptance per gap and the round trips printed at
the end are those of the second half, on the final ladder, which is printed too.

--tune-sigma TARGET tunes the proposal width of every rung on the device towards the acceptance TARGET during the first half of the run
(TuneRungSigma, ten tunings, the last at steps / 2; listed behind RespaceLadder, so with --adapt the widths follow the ladder as it moves)
and leaves the widths alone afterwards -- changing sigma breaks detailed balance across the change, so the first half is burn-in.  The
table starts from sigma_0 at every rung, or from the table of --rung-sigma.  The tuned table is printed, and beside it the acceptance
per rung over the window since the last tuning: the second half, under the final table.

--free-energy accumulates the bridge sums over the second half of the run and prints log(Z_(r+1) / Z_r) by three estimators beside a
quadrature, and the heat capacity per rung.  With --blocks B the sums are kept per block of ladders (ReplicaExchange(..., blocks=B)) and
every estimate comes with the standard error of a delete-one-block jackknife over the B blocks, value +- se; with --reweight N the
energy histograms are kept per block too (EnergyHistogram(..., blocks=B)) and every point of the curve is printed +- se.

--reweight N accumulates an energy histogram per rung on the device over the second half of the run (EnergyHistogram, 100 snapshots)
and prints <e>(beta), C(beta) and log(Z(beta) / Z(beta_0)) by multiple-histogram reweighting (WHAM) on an N-point grid between the end
rungs, each beside the quadrature -- the curve BETWEEN the simulated temperatures.  With --free-energy the WHAM free energies per rung
are printed beside the bridge estimates.

--moments (with --reweight N) runs the TILTED well x^4 - 2 x^2 + x / 4 instead (a potential compiled at run time), whose wells are
not equally deep, keeps the sums of x, x^2 and [x > 0] per energy bin on the device beside the counts
(EnergyHistogram(..., moments=("x", "x2", "pos"), x_bound=4)) and prints <x>(beta), <x^2>(beta) and the occupancy of the right-hand
well P(x > 0)(beta) on the same grid, each beside the quadrature: functions of the POSITION between the simulated temperatures.  With
--blocks B the sums per bin are kept per block of ladders as well, and the three curves are printed +- their jackknife standard error.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlo_amd as ma   # noqa: E402

BETAS = (0.5, 1.0, 2.0, 4.0, 8.0)
SIGMA0 = 0.3
TILTED = "x*x*x*x - 2.0*x*x + 0.25*x"                  # --moments: the left well (x ~ -1.03, U ~ -1.26) lies 0.5 below the right one
X_BOUND = 4.0                                          # |x| <= 4 for every binned chain: U(4) = 225 is far beyond the bins


def well(tilted: bool):
    """U(x) of the run as a numpy function."""
    return (lambda x: x * x * x * x - 2.0 * x * x + 0.25 * x) if tilted else (lambda x: (x * x - 1.0) ** 2)


class RestartBridge(ma.AriannaAlgorithm):
    """The bridge sums start again at the scheduled time: what was accumulated while the chains still left the right well is dropped."""

    def __init__(self, chains, dependencies=None, path=None, **extras):
        self.exchange = dependencies[0]

    def make_step(self, simulation) -> None:
        self.exchange.restart_bridge()


def log_z_by_quadrature():
    """log Z_r, Z_r = integral of exp(-beta_r (x^2 - 1)^2) dx, by the trapezoid rule on a fine grid (the integrand is below 1e-300 at the ends)."""
    x = np.linspace(-6.0, 6.0, 240001)
    return np.array([np.log(np.sum(np.exp(-b * (x * x - 1.0) ** 2)) * (x[1] - x[0])) for b in BETAS])


# the chance of e >= 60 at beta = 0.5 is below 1e-14: no sample of any run lands outside; 5 x 2403 cells: the per-block LDS path.  Energies sit at the bin centres, and
# the density of states diverges at e -> 0: at the cold end, where <e> ~ 1 / (2 beta) is a few bins wide, the curve shows that bias
HIST = dict(lo=0.0, hi=60.0, n_bins=2400)


def curve_by_quadrature(betas, tilted=False):
    """(log Z, <e>, C) at every beta of `betas` by the trapezoid rule on the same grid."""
    x = np.linspace(-6.0, 6.0, 240001)
    u = well(tilted)(x)
    out = []
    for b in betas:
        w = np.exp(-b * u)
        z, m1, m2 = np.sum(w), np.sum(w * u), np.sum(w * u * u)
        out.append((np.log(z * (x[1] - x[0])), m1 / z, b * b * (m2 / z - (m1 / z) ** 2)))
    return tuple(np.array(v) for v in zip(*out))


def moments_by_quadrature(betas):
    """(<x>, <x^2>, P(x > 0)) of the tilted well at every beta of `betas`, by the trapezoid rule on the same grid."""
    x = np.linspace(-6.0, 6.0, 240001)
    u = well(True)(x)
    out = []
    for b in betas:
        w = np.exp(-b * (u - u.min()))
        out.append((np.sum(w * x) / np.sum(w), np.sum(w * x * x) / np.sum(w), np.sum(w[x > 0]) / np.sum(w)))
    return tuple(np.array(v) for v in zip(*out))


def one_run(args, path, exchange: bool):
    R, L = len(BETAS), args.ladders
    x0 = 0.8 + 0.4 * ((np.arange(R * L) * 0.6180339887498949) % 1.0)          # every chain in the right well
    chains = ma.ParticleChains.ladder(L, BETAS, potential=ma.CustomPotential(TILTED) if args.moments else "double_well", x=x0)
    pool = (ma.Move(ma.Displacement(0.0), ma.StandardGaussian(), [SIGMA0], 1.0),)
    algorithm_list = [dict(algorithm=ma.Metropolis, pool=pool, seed=args.seed)]
    if exchange and args.rung_sigma:
        # sigma_0 is the width of the hottest rung; the equilibrium width of a well shrinks like 1 / sqrt(beta)
        algorithm_list[0]["rung_sigma"] = [SIGMA0 * np.sqrt(BETAS[0] / b) for b in BETAS]
    elif exchange and args.tune_sigma is not None:
        algorithm_list[0]["rung_sigma"] = [SIGMA0] * len(BETAS)
    callbacks = [ma.callback_energy]
    if exchange:
        track = args.track or args.adapt == "flow"
        bridge = ma.ReplicaExchange.BRIDGE_DEFAULT | 4 | 8 if args.free_energy else False          # ... and the two W columns
        blocks = args.blocks if args.free_energy else None
        algorithm_list.append(dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), track=track, bridge=bridge, blocks=blocks))   # every time step
        if args.free_energy:                           # measure over the second half of the run
            algorithm_list.append(dict(algorithm=RestartBridge, dependencies=(ma.ReplicaExchange,), scheduler=[max(1, args.steps // 2)]))
        callbacks.append(ma.callback_exchange_acceptance)
        if args.adapt:
            half = args.steps // 2
            every = max(1, half // 5)
            algorithm_list.append(dict(algorithm=ma.RespaceLadder, dependencies=(ma.ReplicaExchange,), rule=args.adapt, gamma=0.7, eps=0.01,
                                       scheduler=list(range(half - 4 * every, half + 1, every)), until=half))
            callbacks.append(ma.callback_ladder)
        if args.tune_sigma is not None:
            half = args.steps // 2
            every = max(1, half // 10)
            algorithm_list.append(dict(algorithm=ma.TuneRungSigma, dependencies=(ma.Metropolis,), target=args.tune_sigma, gamma=1.0, min_calls=1000,
                                       scheduler=list(range(half - 9 * every, half + 1, every)), until=half))
            callbacks.append(ma.callback_rung_sigma)
        if args.reweight:                              # measure over the second half of the run, behind every respacing and tuning
            half = args.steps // 2
            every = max(1, (args.steps - half) // 100)
            hist = dict(HIST, lo=-1.5, hi=58.5, moments=("x", "x2", "pos"), x_bound=X_BOUND) if args.moments else HIST      # (the tilted well reaches -1.26)
            algorithm_list.append(dict(algorithm=ma.EnergyHistogram, dependencies=(ma.Metropolis,), blocks=args.blocks,
                                       scheduler=list(range(half + every, args.steps + 1, every)), **hist))
    algorithm_list.append(dict(algorithm=ma.StoreCallbacks, callbacks=tuple(callbacks),
                               scheduler=ma.build_schedule(args.steps, 0, max(1, args.steps // 10))))
    simulation = ma.Simulation(chains, algorithm_list, args.steps, path=path)
    ma.run(simulation)
    x = simulation.chains.x.reshape(L, R)
    left = (x < 0.0).mean(axis=0)
    energy = well(args.moments)(x).mean(axis=0)
    accept = simulation.algorithms[1].acceptance() if exchange else None
    hist = simulation.algorithms[0].engine.histogram_rungs(-2.0, 2.0, 8) if exchange else None
    return simulation, left, energy, accept, hist


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ladders", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--path", default=None)
    ap.add_argument("--track", action="store_true", help="follow the replicas: print the flow fraction per rung and the round trips")
    ap.add_argument("--rung-sigma", action="store_true", help="a proposal width per rung, sigma_r = sigma_0 sqrt(beta_0 / beta_r); print the move's acceptance per rung")
    ap.add_argument("--adapt", choices=("flow", "acceptance"), default=None,
                    help="respace the ladder during the first half of the run; print the ladder, and the swap acceptance and round trips of the second half")
    ap.add_argument("--tune-sigma", type=float, default=None, metavar="TARGET",
                    help="tune the proposal width of every rung towards this acceptance during the first half of the run; print the table and the "
                         "acceptance per rung of the second half")
    ap.add_argument("--free-energy", action="store_true",
                    help="accumulate the bridge sums over the second half of the run; print log(Z_(r+1) / Z_r) by three estimators beside a "
                         "quadrature, and the heat capacity per rung")
    ap.add_argument("--reweight", type=int, default=0, metavar="N",
                    help="accumulate an energy histogram per rung over the second half of the run; print <e>, C and log Z on an N-point grid "
                         "of beta between the end rungs by multiple-histogram reweighting, beside the quadrature")
    ap.add_argument("--moments", action="store_true",
                    help="with --reweight: run the tilted well x^4 - 2 x^2 + x / 4, keep the sums of x, x^2 and [x > 0] per energy bin and print "
                         "<x>, <x^2> and P(x > 0) on the grid beside the quadrature")
    ap.add_argument("--blocks", type=int, default=None, metavar="B",
                    help="with --free-energy and / or --reweight: keep the bridge sums and the energy histograms per block of ladders and print "
                         "every estimate +- its jackknife standard error")
    args = ap.parse_args(argv)
    if args.blocks is not None and not (args.free_energy or args.reweight):
        ap.error("--blocks needs --free-energy or --reweight")
    if args.moments and not args.reweight:
        ap.error("--moments needs --reweight N")
    if args.moments and args.free_energy:
        ap.error("--moments: the quadrature beside --free-energy is the symmetric well's")
    path = args.path or f"data/PT/particle_1d/DoubleWell/L{args.ladders}/seed{args.seed}"
    sim, left, energy, accept, hist = one_run(args, os.path.join(path, "exchange"), True)
    _, left_plain, energy_plain, _, _ = one_run(args, os.path.join(path, "plain"), False)
    print("beta                          : " + "  ".join(f"{b:7.2f}" for b in BETAS))
    print("fraction x < 0, with exchange : " + "  ".join(f"{v:7.4f}" for v in left))
    print("fraction x < 0, without       : " + "  ".join(f"{v:7.4f}" for v in left_plain))
    print("mean energy, with exchange    : " + "  ".join(f"{v:7.4f}" for v in energy))
    print("mean energy, without          : " + "  ".join(f"{v:7.4f}" for v in energy_plain))
    print("swap acceptance per gap       : " + "  ".join(f"{v:7.4f}" for v in accept))
    if args.tune_sigma is not None:
        met = sim.algorithms[0]
        print(f"width per rung, {met.engine.tune_status()[1]:2d} tunings    : " + "  ".join(f"{v:7.4f}" for v in met.rung_sigma[0]))
        print("acceptance since the last one : " + "  ".join(f"{v:7.4f}" for v in met.rung_window_acceptance()[0]))
    elif args.rung_sigma:
        print("proposal width per rung       : " + "  ".join(f"{v:7.4f}" for v in sim.algorithms[0].rung_sigma[0]))
        print("move acceptance per rung      : " + "  ".join(f"{v:7.4f}" for v in ma.callback_rung_acceptance(sim)[0]))
    print("coldest rung, 8 bins of [-2, 2): " + " ".join(str(int(v)) for v in hist[-1][:8]))
    if args.free_energy:
        rx = sim.algorithms[1]
        exact = np.diff(log_z_by_quadrature())
        if args.blocks:                                 # (value, se) per estimate: the jackknife over the blocks of ladders
            def row(pair, i=None):
                value, se = pair if i is None else (pair[0][i], pair[1][i])
                return "  ".join(f"{v:7.4f} +- {s:6.4f}" for v, s in zip(value, se))
            expo = rx.log_z_ratios("exponential", error=True)
            print(f"log Z ratio per gap, {rx.bridge_sums()[1]:4d} snapshots of {args.ladders} ladders, +- jackknife se over {args.blocks} blocks")
            print("  quadrature                  : " + "  ".join(f"{v:7.4f}          " for v in exact))
            print("  acceptance (Bennett, C = 0) : " + row(rx.log_z_ratios("acceptance", error=True)))
            print("  exponential, forward        : " + row(expo, 0))
            print("  exponential, backward       : " + row(expo, 1))
            print("  thermodynamic integration   : " + row(rx.log_z_ratios("ti", error=True)) + "   (trapezoid: coarse on this ladder)")
            print("log(Z_r / Z_0), acceptance    : " + row(rx.log_z(error=True)))
            print("heat capacity per rung        : " + row(rx.heat_capacity(error=True)))
        else:
            expo = rx.log_z_ratios("exponential")
            print(f"log Z ratio per gap, {rx.bridge_sums()[1]:4d} snapshots of {args.ladders} ladders")
            print("  quadrature                  : " + "  ".join(f"{v:7.4f}" for v in exact))
            print("  acceptance (Bennett, C = 0) : " + "  ".join(f"{v:7.4f}" for v in rx.log_z_ratios("acceptance")))
            print("  exponential, forward        : " + "  ".join(f"{v:7.4f}" for v in expo[0]))
            print("  exponential, backward       : " + "  ".join(f"{v:7.4f}" for v in expo[1]))
            print("  thermodynamic integration   : " + "  ".join(f"{v:7.4f}" for v in rx.log_z_ratios("ti")) + "   (trapezoid: coarse on this ladder)")
            print("heat capacity per rung        : " + "  ".join(f"{v:7.4f}" for v in rx.heat_capacity()))
    if args.reweight:
        eh = next(a for a in sim.algorithms if isinstance(a, ma.EnergyHistogram))
        ladder = eh.betas()
        grid = np.exp(np.linspace(np.log(ladder[0]), np.log(ladder[-1]), max(2, args.reweight)))
        q_log_z, q_m1, q_c = curve_by_quadrature(grid, args.moments)
        q_log_z0 = curve_by_quadrature(ladder[:1], args.moments)[0][0]
        head = f"reweighted curve, {eh.n_snapshots} snapshots of {args.ladders} ladders, {eh.n_bins} bins of [{eh.lo:g}, {eh.hi:g})"
        if args.blocks:                                 # every point of the curve +- the jackknife over the blocks of ladders
            (log_z, z_se), (m1, m1_se), _, (c, c_se) = eh.reweight(grid, error=True)
            print(f"{head}: WHAM +- jackknife se over {args.blocks} blocks | quadrature")
            print("     beta       <e>                           C                             log(Z / Z_0)")
            for i, b in enumerate(grid):
                print(f"  {b:7.4f}   {m1[i]:7.4f} +- {m1_se[i]:6.4f} | {q_m1[i]:7.4f}   {c[i]:7.4f} +- {c_se[i]:6.4f} | {q_c[i]:7.4f}   "
                      f"{log_z[i]:8.4f} +- {z_se[i]:6.4f} | {q_log_z[i] - q_log_z0:8.4f}")
        else:
            log_z, m1, _, c = eh.reweight(grid)
            print(f"{head}: WHAM | quadrature")
            print("     beta       <e>               C                 log(Z / Z_0)")
            for b, e1, e2, c1, c2, z1, z2 in zip(grid, m1, q_m1, c, q_c, log_z, q_log_z - q_log_z0):
                print(f"  {b:7.4f}   {e1:7.4f} | {e2:7.4f}   {c1:7.4f} | {c2:7.4f}   {z1:8.4f} | {z2:8.4f}")
        if args.moments and args.blocks:               # the sums per bin are kept per block too: every moment +- its jackknife se
            mom = eh.reweight_moments(grid, error=True)
            q_x, q_x2, q_pos = moments_by_quadrature(grid)
            print(f"reweighted moments of the position, |x| <= {X_BOUND:g} ({int(eh.beyond_bound().sum())} binned samples beyond it): "
                  f"WHAM +- jackknife se over {args.blocks} blocks | quadrature")
            print("     beta       <x>                           <x^2>                         P(x > 0)")
            for i, b in enumerate(grid):
                print(f"  {b:7.4f}   " + "   ".join(f"{mom[k][0][i]:7.4f} +- {mom[k][1][i]:6.4f} | {q[i]:7.4f}" for k, q in (("x", q_x), ("x2", q_x2), ("pos", q_pos))))
        elif args.moments:
            mom = eh.reweight_moments(grid)
            q_x, q_x2, q_pos = moments_by_quadrature(grid)
            print(f"reweighted moments of the position, |x| <= {X_BOUND:g} ({int(eh.beyond_bound().sum())} binned samples beyond it): WHAM | quadrature")
            print("     beta       <x>               <x^2>             P(x > 0)")
            for b, x1, x2, s1, s2, p1, p2 in zip(grid, mom["x"], q_x, mom["x2"], q_x2, mom["pos"], q_pos):
                print(f"  {b:7.4f}   {x1:7.4f} | {x2:7.4f}   {s1:7.4f} | {s2:7.4f}   {p1:7.4f} | {p2:7.4f}")
        if args.free_energy:
            rx = sim.algorithms[1]
            print("log(Z_r / Z_0), WHAM (-f_r)   : " + "  ".join(f"{v:7.4f}" for v in -eh.free_energies()))
            print("log(Z_r / Z_0), bridge sums   : " + "  ".join(f"{v:7.4f}" for v in rx.log_z("acceptance")))
            print("log(Z_r / Z_0), quadrature    : " + "  ".join(f"{v:7.4f}" for v in curve_by_quadrature(ladder)[0] - q_log_z0))
    if args.adapt:
        rx = sim.algorithms[1]
        print(f"ladder after {rx.metropolis.engine.respace_status()[1]} respacings   : " + "  ".join(f"{b:7.4f}" for b in rx.betas()) + "   (second half: the lines above and below)")
    if args.track or args.adapt == "flow":
        rx = sim.algorithms[1]
        trips = rx.round_trips()
        print("flow fraction f(r)            : " + "  ".join(f"{v:7.4f}" for v in rx.flow()))
        print(f"round trips per ladder        : {trips[0] / args.ladders:7.4f}  (up trips {trips[1] / args.ladders:7.4f})")
    return sim, left, left_plain, accept


if __name__ == "__main__":
    main()
