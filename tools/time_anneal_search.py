#!/usr/bin/env python3
"""Time of one choice of the next beta (amc_anneal_next_beta, rounds = 6) at M = 1e7, harmonic, Float64, next to one population-annealing
step (amc_anneal) and one single-sweep launch of the same handle, in the same run.  tools/time_anneal.py's method: HIP-event timing
(amc_timing_begin / _end) over windows of calls after a ramp, the windows of the figures alternating REPEATS times (median and range
of the windows); prints the markdown table of profiles/population_annealing_adaptive.md.

A search moves nothing, so a window repeats the same search on the same population; it synchronises once per call, so its window is
timed twice: by the events on the stream (which see the idle stream while the host reads the answer and queues the next call) and by
the host's clock.  The annealing step is timed as time_anneal.py times it: steps alternate between beta and beta * (1 + STEP) with
one sweep behind each, and the sweeps' own time is taken off.

    python tools/time_anneal_search.py [--chains 10000000] [--launches 50] [--repeats 7] [--rounds 6] [--target 0.9] [--limit 2.0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlo_amd import _capi   # noqa: E402


def device_us(eng, call, n):
    eng.sync()
    eng.timing_begin()
    for _ in range(n):
        call()
    return eng.timing_end() * 1e3 / n


def host_us(eng, call, n):
    eng.sync()
    t = time.perf_counter()
    for _ in range(n):
        call()
    eng.sync()
    return (time.perf_counter() - t) * 1e6 / n


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--target", type=float, default=0.9)
    ap.add_argument("--limit", type=float, default=2.0)
    ap.add_argument("--step", type=float, default=0.02)
    args = ap.parse_args(argv)
    M, n = args.chains, args.launches
    eng = _capi.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=1, per_chain_counters=False)
    eng.init_uniform(-2.0, 2.0)
    eng.sweep(600)                                       # ramp: clocks up, state equilibrated
    eng.sync()
    flip = [0]

    def anneal_round():
        flip[0] ^= 1
        eng.anneal(1.0 + args.step * flip[0])
        eng.sweep(1)

    def search():
        return eng.anneal_next_beta(args.limit, args.target, args.rounds)

    def search_one_round():
        return eng.anneal_next_beta(args.limit, args.target, 1)

    us = {k: [] for k in ("sweep", "round", "search", "search_host", "search1", "search1_host")}
    for _ in range(args.repeats):
        us["sweep"].append(device_us(eng, lambda: eng.sweep(1), n))
        us["round"].append(device_us(eng, anneal_round, n))
        if flip[0]:
            anneal_round()                               # back at beta = 1 for the searches
        us["search"].append(device_us(eng, search, n))
        us["search_host"].append(host_us(eng, search, n))
        us["search1"].append(device_us(eng, search_one_round, n))
        us["search1_host"].append(host_us(eng, search_one_round, n))
        eng.anneal_records(reset=True)
    med = {k: float(np.median(v)) for k, v in us.items()}
    cell = lambda k, off=0.0: f"{med[k] - off:.1f} ({min(us[k]) - off:.1f} .. {max(us[k]) - off:.1f})"
    s = med["sweep"]
    step = med["round"] - s
    b, diag, trace = search()
    print(f"M = {M}, harmonic, Float64, K = 1, beta = 1, limit {args.limit}, target {args.target}; {args.repeats} alternating windows of {n} calls per "
          f"figure (median, min .. max)\n")
    print("| figure | us | vs one annealing step |")
    print("|---|---|---|")
    print(f"| one single-sweep launch | {cell('sweep')} | {s / step:.2f} |")
    print(f"| one annealing step, a sweep behind each (the sweep's median taken off) | {cell('round', s)} | 1 |")
    print(f"| one amc_anneal_next_beta, rounds = {args.rounds}: stream time (events; one synchronisation per call) | {cell('search')} | {med['search'] / step:.2f} |")
    print(f"| the same, host time | {cell('search_host')} | {med['search_host'] / step:.2f} |")
    print(f"| one amc_anneal_next_beta, rounds = 1: stream time | {cell('search1')} | {med['search1'] / step:.2f} |")
    print(f"| the same, host time | {cell('search1_host')} | {med['search1_host'] / step:.2f} |")
    per_round = (med["search"] - med["search1"]) / max(args.rounds - 1, 1)
    print(f"\none further round (a sums pass over {M} chains and the decision): {per_round:.1f} us, {per_round / M * 1e6:.2f} ps per chain and round, "
          f"{8 * M / per_round / 1e6:.2f} TB/s of energies read, {8 * M / per_round / 1e3:.1f} G exp per second")
    rho = np.array([diag[3], diag[5]], dtype=np.uint64).view(np.float64)
    print(f"the search: status {int(diag[0])}, beta_new = {b!r}, rho at the step {rho[0]:.6f}, rho at the bracket's high end {rho[1]:.6f}, "
          f"S1 / (M 2^30) of the last round's first candidate {int(trace[-1, 0, 0]) / (M * 2.0 ** 30):.4f}")
    eng.close()


if __name__ == "__main__":
    main()
