#!/usr/bin/env python3
"""Stream time of one tuning of the widths per rung (amc_tune_rung_sigma, local counts) at M = 1e7, R = 8, harmonic, Float64, K = 1
and K = 2, next to one amc_rung_counter_totals (the totals pass the tuning queues, plus its copy and synchronisation; wall clock, the
entry waits for the device) and one single-sweep launch of the same handle.  HIP-event timing (amc_timing_begin / _end) for the
stream-ordered calls.

A tuning ends its window, so the next one would find an empty window (status 1: the rule is not run to its end).  A timed window is
therefore [one sweep; one tuning], which gives every tuning counts to work with, and the same window without the tuning is timed
beside it: the difference is the tuning.  Windows alternate REPEATS times (median, min .. max); tune_status() afterwards must count one
tuning per window.  Prints the markdown table of profiles/rung_sigma_tuning.md.

    python tools/time_tune.py [--chains 10000000] [--rungs 8] [--windows 50] [--repeats 7]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlo_amd import _capi   # noqa: E402
from time_exchange import device_us   # noqa: E402


def make_engine(M, R, K):
    betas = 0.5 * 1.3 ** np.arange(R)
    sigma = [0.5 / (1 + k) for k in range(K)]
    eng = _capi.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=sigma, weight=[1.0 / K] * K, seed=1, per_chain_counters=True)
    eng.upload_state(np.zeros(M), np.tile(betas, M // R))
    eng.init_uniform(-2.0, 2.0)
    eng.set_ladder(R)
    eng.set_rung_sigma(np.array([[s / np.sqrt(b / betas[0]) for b in betas] for s in sigma]))
    for _ in range(3):                                   # ramp: clocks up, state equilibrated
        eng.sweep_exchange(100, 1)
    eng.sync()
    return eng


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--rungs", type=int, default=8)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args(argv)
    R, n = args.rungs, args.windows
    M = (args.chains // R) * R
    print(f"M = {M}, R = {R}, harmonic, Float64; {args.repeats} alternating pairs of windows, {n} x [one sweep (; one tuning)] each "
          f"(median, min .. max)\n")
    print("| K | window without us | window with us | one tuning us | amc_rung_counter_totals us (wall) | one single-sweep launch us | tuning / totals |")
    print("|---|---|---|---|---|---|---|")
    for K in (1, 2):
        eng = make_engine(M, R, K)
        sweep_us = device_us(eng, lambda: eng.sweep(1), 200)
        base, full, totals = [], [], []
        n0 = eng.tune_status()[1]
        for _ in range(args.repeats):
            base.append(device_us(eng, lambda: eng.sweep(1), n))
            full.append(device_us(eng, lambda: (eng.sweep(1), eng.tune_rung_sigma(0.44, 0.5, 1000, 1e-100, 1e100)), n))
            eng.sweep(1)
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(20):
                eng.rung_counter_totals()
            totals.append((time.perf_counter() - t0) * 1e6 / 20)
        st, n1 = eng.tune_status()
        assert np.all(st == 0) and n1 - n0 == args.repeats * n, (st, n1 - n0)
        b, f, t = float(np.median(base)), float(np.median(full)), float(np.median(totals))
        cell = lambda v: f"{np.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"
        print(f"| {K} | {cell(base)} | {cell(full)} | {f - b:.1f} | {cell(totals)} | {sweep_us:.1f} | {(f - b) / t:.2f} |")
        print(f"<!-- table after the windows (K = {K}): " + " ".join(f"{v:.4f}" for v in eng.rung_sigma().reshape(-1)) + " -->")
        eng.close()


if __name__ == "__main__":
    main()
