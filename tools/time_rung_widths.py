#!/usr/bin/env python3
"""Device time of one single-sweep launch with a table of widths per rung (amc_set_rung_sigma) against the same handle's launch
without, at M = 1e7, R = 8, harmonic, Float64, per-chain counters, K = 1 and K = 2; and one amc_rung_counter_totals call against
amc_counter_totals.  HIP-event timing (amc_timing_begin / _end) over LAUNCHES launches after a ramp; the handle alternates between
the two forms REPEATS times (median and range of the windows).  The table's rows equal the pool's sigma_k, so both forms take the
same steps (the same bits: tests/test_gpu_rung_sigma.py) and the windows differ in the kernel alone.  Prints the markdown tables of
profiles/rung_widths.md.

    python tools/time_rung_widths.py [--chains 10000000] [--rungs 8] [--launches 400] [--repeats 7]
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


def make_engine(M, R, K):
    L = M // R
    betas = 0.5 * 1.3 ** np.arange(R)
    sigma = [0.5 / (1 + k) for k in range(K)]
    eng = _capi.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=sigma, weight=[1.0 / K] * K, seed=1, per_chain_counters=True)
    eng.upload_state(np.zeros(M), np.tile(betas, L))
    eng.init_uniform(-2.0, 2.0)
    eng.set_ladder(R)
    for _ in range(3):                                   # ramp: clocks up, state equilibrated
        eng.sweep_exchange(200, 1)
    eng.sync()
    return eng, np.repeat(np.array(sigma)[:, None], R, axis=1)


def cell(v):
    return f"{np.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--rungs", type=int, default=8)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args(argv)
    R, n = args.rungs, args.launches
    M = (args.chains // R) * R
    print(f"M = {M}, R = {R}, harmonic, Float64, per-chain counters; {args.repeats} alternating windows of {n} launches per figure "
          "(median, min .. max)\n")
    print("| K | plain form us | with a table us | table / plain |")
    print("|---|---|---|---|")
    med = {}
    for K in (1, 2):
        eng, tab = make_engine(M, R, K)
        us = {False: [], True: []}
        for _ in range(args.repeats):
            for on in (False, True):
                eng.set_rung_sigma(tab if on else None)
                eng.sweep(3)                             # (the first launch of a form loads its code object)
                us[on].append(device_us(eng, lambda: eng.sweep(1), n))
        med[K] = {on: float(np.median(v)) for on, v in us.items()}
        print(f"| {K} | {cell(us[False])} | {cell(us[True])} | {med[K][True] / med[K][False]:.3f} |")
        if K == 2:
            host = {"amc_counter_totals": [], "amc_rung_counter_totals": []}
            dev = {"amc_counter_totals": [], "amc_rung_counter_totals": []}
            for _ in range(args.repeats):
                for name, call in (("amc_counter_totals", eng.counter_totals), ("amc_rung_counter_totals", eng.rung_counter_totals)):
                    eng.sweep(1)                         # a log row to fold, as after a sweep
                    eng.sync()
                    t = time.perf_counter()
                    call()
                    host[name].append((time.perf_counter() - t) * 1e6)
                    dev[name].append(device_us(eng, call, 20))
        eng.close()
    print(f"\nthe form with a table at K = 1 against the plain K = 2 form: {med[1][True] / med[2][False]:.3f}\n")
    print("| call (K = 2) | host us, one call after a sweep | stream us per call, 20 back to back |")
    print("|---|---|---|")
    for name in host:
        print(f"| {name} | {cell(host[name])} | {cell(dev[name])} |")


if __name__ == "__main__":
    main()
