#!/usr/bin/env python3
"""Population annealing of the double well (x^2 - 1)^2 on one MI355X: log Z(beta) along a whole cooling schedule from one run.

A population of chains is equilibrated at beta = 0.5, where a local Gaussian move crosses the barrier freely, and then cooled to
beta = 8 in geometric steps.  At each step the engine resamples the population in proportion to exp(-(beta' - beta) e)
(PopulationAnnealing, amc_anneal) and the sweeps behind it equilibrate the copies; the mean weight of the step estimates
Z(beta') / Z(beta).  The script prints log(Z(beta) / Z(0.5)) at every annealing temperature beside a quadrature, the share of the
population that survived each step, and rho_t, the mean size of the family a chain belongs to.

The run is repeated for --runs independent seeds; the figure printed is their mean, and the tolerance printed beside the largest
deviation is 8 standard errors of that mean (the spread of the runs themselves; Student's t with 7 degrees of freedom leaves less
than 1e-4 outside 8 standard errors, and the bias of one run, of the order of its variance, is far below that).

With --adaptive TARGET the list of beta values is not given: at each scheduled time the engine chooses the next beta itself, the
largest step towards beta = 8 whose reweighting keeps the effective-sample fraction ESS / M at or above TARGET
(PopulationAnnealing(adaptive=...), amc_anneal_next_beta), for at most --stages steps.  Every run then has its own list, so the script
prints log(Z(8) / Z(0.5)) of the runs beside the quadrature, and the steps the last run chose.

With --reweight N the energy histogram of the population is taken on the device in front of every annealing step and at the end
(PopulationAnnealing(energy_histogram=...)), and the last run prints <e>(beta), C(beta) and log(Z(beta) / Z(0.5)) by multiple-histogram
reweighting over the temperatures of the schedule on an N-point grid from 0.5 to the last beta, each beside the quadrature.

With --blocks B the families are partitioned into B blocks and the engine keeps the weight sums of every step per block
(PopulationAnnealing(blocks=B), amc_set_anneal_blocks): the last run prints log(Z(beta) / Z(0.5)) +- its own delete-one-block jackknife
standard error beside the quadrature -- an error bar from ONE run, where the tolerance above needs several.  Together with
--reweight N the histograms are kept per block of families and every point of the reweighted curve is printed +- its standard error.

    python examples/pa_double_well.py [--chains 65536] [--stages 24] [--sweeps 10] [--runs 8] [--path data/PA/...] [--adaptive TARGET]
                                      [--reweight N] [--blocks B]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlo_amd as ma   # noqa: E402

BETA_HOT, BETA_COLD = 0.5, 8.0
SIGMA = 0.4
BURN = 200


def log_z_by_quadrature(betas):
    """log Z(beta), Z = integral of exp(-beta (x^2 - 1)^2) dx, by the trapezoid rule on a fine grid (the integrand is below 1e-300 at the ends)."""
    x = np.linspace(-8.0, 8.0, 320001)
    return np.array([np.log(np.sum(np.exp(-b * (x * x - 1.0) ** 2)) * (x[1] - x[0])) for b in betas])


# the chance of e >= 60 at beta = 0.5 is below 1e-14: no sample of any run lands outside; one row of 6003 cells.  Energies sit at the bin centres, and
# the density of states diverges at e -> 0: at the cold end, where <e> ~ 1 / (2 beta) is a few bins wide, the curve shows that bias
HIST = dict(lo=0.0, hi=60.0, n_bins=6000)


def curve_by_quadrature(betas):
    """(log Z, <e>, C) at every beta of `betas` by the trapezoid rule on the same grid."""
    x = np.linspace(-8.0, 8.0, 320001)
    u = (x * x - 1.0) ** 2
    out = []
    for b in betas:
        w = np.exp(-b * u)
        z, m1, m2 = np.sum(w), np.sum(w * u), np.sum(w * u * u)
        out.append((np.log(z * (x[1] - x[0])), m1 / z, b * b * (m2 / z - (m1 / z) ** 2)))
    return tuple(np.array(v) for v in zip(*out))


def print_reweighted(args, pa):
    """--reweight: the curve along the schedule from the last run's histograms, beside the quadrature."""
    taken, _ = pa.histograms()
    grid = np.exp(np.linspace(np.log(taken[0]), np.log(taken[-1]), max(2, args.reweight)))
    if pa.blocks is not None:              # --blocks: every point with its jackknife standard error over the blocks of families
        (log_z, m1, _, c), (log_z_se, m1_se, _, c_se) = pa.reweight(grid, error=True)
    else:
        log_z, m1, _, c = pa.reweight(grid)
    q_log_z, q_m1, q_c = curve_by_quadrature(grid)
    q0 = curve_by_quadrature(taken[:1])[0][0]
    print(f"last run, reweighted over {len(taken)} temperatures, {HIST['n_bins']} bins of [{HIST['lo']:g}, {HIST['hi']:g}): WHAM | quadrature")
    print("     beta       <e>               C                 log(Z / Z(0.5))")
    if pa.blocks is not None:
        for b, e1, s1, e2, c1, s2, c2, z1, s3, z2 in zip(grid, m1, m1_se, q_m1, c, c_se, q_c, log_z, log_z_se, q_log_z - q0):
            print(f"  {b:7.4f}   {e1:7.4f} +- {s1:.4f} | {e2:7.4f}   {c1:7.4f} +- {s2:.4f} | {c2:7.4f}   {z1:8.4f} +- {s3:.4f} | {z2:8.4f}")
        return
    for b, e1, e2, c1, c2, z1, z2 in zip(grid, m1, q_m1, c, q_c, log_z, q_log_z - q0):
        print(f"  {b:7.4f}   {e1:7.4f} | {e2:7.4f}   {c1:7.4f} | {c2:7.4f}   {z1:8.4f} | {z2:8.4f}")


def print_error_bars(pa, exact):
    """--blocks: the last run's log Z with its jackknife standard error over the blocks of families, beside the quadrature."""
    value, se = pa.log_z(error=True)
    done = pa.betas_done()
    print(f"last run, jackknife over {pa.blocks[0]} blocks of families:\n   beta   log Z(beta)/Z(0.5) +- se          quadrature   difference / se")
    for b, v, s, q in zip(done, value, se, exact):
        print(f"{b:7.4f}   {v:12.6f} +- {s:.6f}   {q:12.6f}   {(v - q) / s:+8.2f}")


def one_run(args, path, seed):
    betas = BETA_HOT * (BETA_COLD / BETA_HOT) ** (np.arange(args.stages + 1) / args.stages)
    steps = BURN + args.stages * args.sweeps
    chains = ma.ParticleChains.uniform(args.chains, BETA_HOT, lo=-2.0, hi=2.0, potential="double_well")
    pool = (ma.Move(ma.Displacement(0.0), ma.StandardGaussian(), [SIGMA], 1.0),)
    # BURN sweeps at the hot end, then [anneal; sweeps] per stage: the annealing step is due at BURN, BURN + sweeps, ...
    when = [BURN + i * args.sweeps for i in range(args.stages)]
    schedule = dict(betas=list(betas[1:])) if args.adaptive is None else dict(adaptive=dict(beta_end=BETA_COLD, target=args.adaptive))
    if args.reweight:
        schedule["energy_histogram"] = HIST
    if args.blocks:
        schedule["blocks"] = args.blocks
    algorithm_list = [dict(algorithm=ma.Metropolis, pool=pool, seed=seed),
                      dict(algorithm=ma.PopulationAnnealing, dependencies=(ma.Metropolis,), scheduler=when, families=True, **schedule),
                      dict(algorithm=ma.StoreCallbacks, callbacks=(ma.callback_energy, ma.callback_anneal_beta, ma.callback_anneal_log_z, ma.callback_rho_t),
                           scheduler=when)]
    simulation = ma.Simulation(chains, algorithm_list, steps, path=path)
    ma.run(simulation)
    return simulation, betas


def adaptive_main(args, path):
    """--adaptive: the runs choose their own steps; log(Z(8) / Z(0.5)) of each beside the quadrature, and the last run's steps."""
    ends, pa = [], None
    for r in range(args.runs):
        sim, _ = one_run(args, os.path.join(path, f"run{r}"), args.seed + r)
        pa = sim.algorithms[1]
        if not pa.finished:
            raise SystemExit(f"run {r}: beta = {pa.beta} after {args.stages} steps; raise --stages or lower --adaptive")
        ends.append(pa.log_z()[-1])
    ends = np.array(ends)
    done = pa.betas_done()
    q = log_z_by_quadrature(np.concatenate([[BETA_HOT], done]))
    exact = q[1:] - q[0]
    tol = 8.0 * ends.std(ddof=1) / np.sqrt(args.runs) if args.runs > 1 else float("nan")
    print(f"{args.runs} runs of {args.chains} chains, steps chosen for ESS / M >= {args.adaptive}, {args.sweeps} sweeps behind each")
    print(f"log Z(8) / Z(0.5): mean {ends.mean():.6f}, quadrature {exact[-1]:.6f}, difference {ends.mean() - exact[-1]:+.6f}, tolerance {tol:.6f}")
    print(f"last run, {len(done)} steps:\n   beta   log Z(beta)/Z(0.5)   quadrature   survival   ESS / M kept   search")
    log, lz, survival = pa.search_log(), pa.log_z(), pa.survival()
    for i in range(len(done)):
        kept = float(np.array([log[i, 3]], dtype=np.uint64).view(np.float64)[0])
        print(f"{done[i]:7.4f}   {lz[i]:12.6f}   {exact[i]:12.6f}   {survival[i]:7.4f}   {kept:8.4f}   {ma.ANNEAL_SEARCH_STATUS[int(log[i, 0])]}")
    print(f"last run: rho_t = {pa.rho_t():.2f} of {args.chains} chains")
    if args.blocks:
        print_error_bars(pa, exact)
    if args.reweight:
        print_reweighted(args, pa)
    return ends, exact[-1], tol, done


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--stages", type=int, default=24, help="annealing steps from beta = 0.5 to beta = 8 (geometric)")
    ap.add_argument("--sweeps", type=int, default=10, help="sweeps behind every annealing step")
    ap.add_argument("--runs", type=int, default=8, help="independent runs (seeds); their spread is the tolerance")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--path", default=None)
    ap.add_argument("--adaptive", type=float, default=None, metavar="TARGET",
                    help="choose every step on the device: the largest one that keeps ESS / M >= TARGET (--stages is then the most steps a run may take)")
    ap.add_argument("--reweight", type=int, default=0, metavar="N",
                    help="take the energy histogram at every annealing temperature; print <e>, C and log Z on an N-point grid of beta along "
                         "the schedule by multiple-histogram reweighting, beside the quadrature")
    ap.add_argument("--blocks", type=int, default=0, metavar="B",
                    help="partition the families into B blocks; print the last run's log Z +- its jackknife standard error beside the quadrature")
    args = ap.parse_args(argv)
    path = args.path or f"data/PA/particle_1d/DoubleWell/M{args.chains}/seed{args.seed}"
    if args.adaptive is not None:
        return adaptive_main(args, path)
    log_z, survival, rho, left = [], None, None, None
    for r in range(args.runs):
        sim, betas = one_run(args, os.path.join(path, f"run{r}"), args.seed + r)
        pa = sim.algorithms[1]
        log_z.append(pa.log_z())
        survival, rho = pa.survival(), pa.rho_t()
        left = float((sim.chains.x < 0.0).mean())
    log_z = np.array(log_z)
    mean = log_z.mean(axis=0)
    tol = 8.0 * log_z.std(axis=0, ddof=1) / np.sqrt(args.runs) if args.runs > 1 else np.full_like(mean, np.nan)
    q = log_z_by_quadrature(betas)
    exact = q[1:] - q[0]
    print(f"{args.runs} runs of {args.chains} chains, {args.stages} annealing steps, {args.sweeps} sweeps behind each")
    print("   beta   log Z(beta)/Z(0.5)   quadrature   difference   tolerance   survival (last run)")
    for i in range(args.stages):
        print(f"{betas[i + 1]:7.4f}   {mean[i]:12.6f}   {exact[i]:12.6f}   {mean[i] - exact[i]:+10.6f}   {tol[i]:9.6f}   {survival[i]:7.4f}")
    worst = int(np.argmax(np.abs(mean - exact) / tol)) if args.runs > 1 else args.stages - 1
    print(f"largest deviation in units of its tolerance: {abs(mean[worst] - exact[worst]) / tol[worst]:.3f} at beta = {betas[worst + 1]:.4f}")
    print(f"last run: rho_t = {rho:.2f} of {args.chains} chains, fraction x < 0 at beta = {betas[-1]:.1f}: {left:.4f}")
    if args.blocks:
        print_error_bars(pa, exact)
    if args.reweight:
        print_reweighted(args, pa)
    return mean, exact, tol, survival, rho, left


if __name__ == "__main__":
    main()
