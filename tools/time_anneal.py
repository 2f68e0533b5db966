#!/usr/bin/env python3
"""Device time of one population-annealing step (amc_anneal) at M = 1e7, harmonic, Float64, next to one single-sweep launch of the same
handle: the step alone, the step with families on, one amc_anneal_family_stats call.  HIP-event timing (amc_timing_begin / _end) over
windows of LAUNCHES steps after a ramp, the windows of the figures alternating REPEATS times (median and range of the windows); prints
the markdown table of profiles/population_annealing.md.

A window's steps alternate between beta and beta * (1 + STEP) with one sweep behind each, as a run does (the sweep keeps the population
from collapsing into copies); the sweeps' own time, measured by windows of the same number of single-sweep launches, is taken off.

    python tools/time_anneal.py [--chains 10000000] [--launches 100] [--repeats 7] [--step 0.02]
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


def make_engine(M, families):
    eng = _capi.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=1, per_chain_counters=False)
    eng.init_uniform(-2.0, 2.0)
    if families:
        eng.set_anneal_families(True)
    eng.sweep(600)                                       # ramp: clocks up, state equilibrated
    eng.sync()
    return eng


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step", type=float, default=0.02)
    args = ap.parse_args(argv)
    M, n = args.chains, args.launches
    plain, fam = make_engine(M, False), make_engine(M, True)
    state = {id(plain): 0, id(fam): 0}

    def round_of(eng):
        def call():
            state[id(eng)] ^= 1
            eng.anneal(1.0 + args.step * state[id(eng)])
            eng.sweep(1)
        return call

    def step_of(eng):
        def call():
            state[id(eng)] ^= 1
            eng.anneal(1.0 + args.step * state[id(eng)])
        return call

    us = {k: [] for k in ("sweep", "round", "round_fam", "alone", "alone_fam", "stats", "stats_host")}
    for _ in range(args.repeats):
        us["sweep"].append(device_us(plain, lambda: plain.sweep(1), n))
        us["round"].append(device_us(plain, round_of(plain), n))
        us["round_fam"].append(device_us(fam, round_of(fam), n))
        us["alone"].append(device_us(plain, step_of(plain), n))
        us["alone_fam"].append(device_us(fam, step_of(fam), n))
        fam.sweep(1)
        us["stats"].append(device_us(fam, fam.anneal_family_stats, 10))
        fam.sync()
        t = time.perf_counter()
        stats = fam.anneal_family_stats()
        us["stats_host"].append((time.perf_counter() - t) * 1e6)
        rec = plain.anneal_records(reset=True)
        fam.anneal_records(reset=True)
    med = {k: float(np.median(v)) for k, v in us.items()}
    cell = lambda k, off=0.0: f"{med[k] - off:.1f} ({min(us[k]) - off:.1f} .. {max(us[k]) - off:.1f})"
    s = med["sweep"]
    print(f"M = {M}, harmonic, Float64, K = 1, beta 1 <-> {1.0 + args.step}; {args.repeats} alternating windows of {n} launches per figure "
          f"(median, min .. max)\n")
    print("| figure | us | vs one single-sweep launch |")
    print("|---|---|---|")
    print(f"| one single-sweep launch | {cell('sweep')} | 1 |")
    print(f"| one annealing step, a sweep behind each (the sweep's median taken off) | {cell('round', s)} | {(med['round'] - s) / s:.2f} |")
    print(f"| the same with families on | {cell('round_fam', s)} | {(med['round_fam'] - s) / s:.2f} |")
    print(f"| one annealing step, back to back (no sweep between) | {cell('alone')} | {med['alone'] / s:.2f} |")
    print(f"| the same with families on | {cell('alone_fam')} | {med['alone_fam'] / s:.2f} |")
    print(f"| one amc_anneal_family_stats call, stream time over 10 back-to-back calls | {cell('stats')} | {med['stats'] / s:.2f} |")
    print(f"| one amc_anneal_family_stats call, host time (synchronises) | {cell('stats_host')} | {med['stats_host'] / s:.2f} |")
    last = rec[-1]
    print(f"\nlast record of the plain handle: status {int(last[0])}, T_w / (M 2^30) = {int(last[4]) / (M * 2.0 ** 30):.4f}, "
          f"n_parents / M = {int(last[6]) / M:.4f}, max_children = {int(last[7])}; families alive / M = {stats[0] / M:.4f}, "
          f"rho_t = {stats[1] / M:.2f}, largest = {stats[2]}")
    plain.close()
    fam.close()


if __name__ == "__main__":
    main()
