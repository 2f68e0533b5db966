#!/usr/bin/env python3
"""Have the chains at a rung converged?  R-hat per rung of the double-well ladder, measured on the device.

Cold double-well chains started in BOTH wells: at beta = 8 each well equilibrates within a few sweeps while the ensemble as a whole
does not -- the acceptance per rung, the swap acceptance, tau_int from one time origin and the energy moments all look healthy in
that state.  The Gelman-Rubin R-hat of x does not: the chains' time means sit at +-1 while every chain moves by 1 / sqrt(beta V'')
around its own, so R-hat_x is about 10 at the cold rungs.  R-hat of the ENERGY is blind to the wells (the potential is even) and
stays near 1.  The same schedule runs with and without exchange steps: with them the SLOT at a cold rung is visited by replicas from
both wells and its R-hat_x comes down, rung by rung -- the direct complement of the round-trip tracking.

    python examples/rhat_double_well.py [--ladders 16384] [--burn 200] [--every 4] [--samples 64] [--path data/RHAT/...]

``Convergence`` keeps two running sums per chain and half of the window on the device, one memory-bound pass per sample; nothing but
seven sums per rung leaves it.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlo_amd as ma   # noqa: E402

BETAS = (0.5, 1.0, 2.0, 4.0, 8.0)
SIGMA0 = 0.3


def ladder_run(args, path, observable: str, exchange: bool, engine_factory=None):
    R, L = len(BETAS), args.ladders
    sched = [args.burn + args.every * (k + 1) for k in range(args.samples)]
    # ladder l starts in the right well when l is even, in the left one when it is odd: both wells at every rung
    x0 = np.where(np.arange(R * L) // R % 2 == 0, 1.0, -1.0)
    chains = ma.ParticleChains.ladder(L, BETAS, potential="double_well", x=x0)
    pool = (ma.Move(ma.Displacement(0.0), ma.StandardGaussian(), [SIGMA0], 1.0),)
    met = dict(algorithm=ma.Metropolis, pool=pool, seed=args.seed)
    if engine_factory is not None:
        met["engine_factory"] = engine_factory
    # the burn-in always exchanges (both runs start from the same kind of ensemble); afterwards only the run that is asked to
    x_sched = list(range(1, sched[-1] + 1)) if exchange else list(range(1, args.burn + 1))
    al = [met, dict(algorithm=ma.ReplicaExchange, dependencies=(ma.Metropolis,), scheduler=x_sched),
          dict(algorithm=ma.Convergence, dependencies=(ma.Metropolis,), scheduler=sched, observable=observable, n_samples=args.samples)]
    sim = ma.Simulation(chains, al, sched[-1], path=path)
    ma.run(sim)
    return sim.algorithms[2], ma.callback_exchange_acceptance(sim)


def row(label, values, fmt="{:9.3f}"):
    print(f"{label:34s}: " + "  ".join(fmt.format(v) for v in values))


def main(argv=None, engine_factory=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ladders", type=int, default=16384)
    ap.add_argument("--burn", type=int, default=200, help="time steps before the first sample")
    ap.add_argument("--every", type=int, default=4, help="MH steps between two samples")
    ap.add_argument("--samples", type=int, default=64, help="samples of the window (even): half of them per part")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--path", default=None)
    args = ap.parse_args(argv)
    path = args.path or f"data/RHAT/particle_1d/DoubleWell/L{args.ladders}/seed{args.seed}"
    out = {}
    for exchange in (True, False):
        for observable in ("x", "energy"):
            cv, accept = ladder_run(args, os.path.join(path, "exchange" if exchange else "plain", observable), observable, exchange, engine_factory)
            out[exchange, observable] = cv.rhat()
            if exchange:
                out["accept"] = accept
    row("beta", BETAS)
    row("swap acceptance per gap", out["accept"])
    row("R-hat(x), with exchange", out[True, "x"])
    row("R-hat(x), without", out[False, "x"])
    row("R-hat(energy), with exchange", out[True, "energy"])
    row("R-hat(energy), without", out[False, "energy"])
    print("(split R-hat: 2N half-chains per rung; below about 1.01 the rung counts as converged, far above it every other number of "
          "that rung describes one well at a time)")
    return out


if __name__ == "__main__":
    main()
