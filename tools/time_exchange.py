#!/usr/bin/env python3
"""Device time of one exchange step (amc_exchange(1)) at M = 1e7, R = 8, harmonic, Float64, next to one single-sweep launch of the
same handle, and host time per round of amc_sweep_exchange against the separate calls.  HIP-event timing (amc_timing_begin / _end)
over LAUNCHES launches after a ramp; prints the markdown table of profiles/exchange.md.

    python tools/time_exchange.py [--chains 10000000] [--rungs 8] [--launches 400]
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--rungs", type=int, default=8)
    ap.add_argument("--launches", type=int, default=400)
    args = ap.parse_args(argv)
    R = args.rungs
    M = (args.chains // R) * R
    L = M // R
    betas = 0.5 * 1.3 ** np.arange(R)
    eng = _capi.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=1, per_chain_counters=False)
    eng.upload_state(np.zeros(M), np.tile(betas, L))
    eng.init_uniform(-2.0, 2.0)
    eng.set_ladder(R)
    n = args.launches
    for _ in range(3):                                   # ramp: clocks up, state equilibrated
        eng.sweep_exchange(200, 1)
    eng.sync()
    sweep_us = device_us(eng, lambda: eng.sweep(1), n)
    rows = []
    for parity in (0, 1):
        def step():
            eng.exchange_step = parity                   # the same parity every launch
            eng.exchange(1)
        a0, t0 = eng.exchange_counters()
        us = device_us(eng, step, n)
        a1, t1 = eng.exchange_counters()
        partnered = 2 * (t1 - t0).sum() / n
        swaps = (a1 - a0).sum() / n
        nbytes = 16.0 * partnered + 16.0 * swaps
        rows.append((parity, us, partnered, swaps, nbytes, nbytes / (us * 1e-6) / 8e12))
    eng.sync()
    t = time.perf_counter()
    for _ in range(n):
        eng.sweep(1)
        eng.exchange(1)
    host_sep = (time.perf_counter() - t) * 1e6 / n
    eng.sync()
    t = time.perf_counter()
    eng.sweep_exchange(n, 1)
    host_one = (time.perf_counter() - t) * 1e6 / n
    eng.sync()
    print(f"M = {M}, R = {R}, harmonic, Float64, K = 1; {n} launches per figure; one single-sweep launch of the same handle: {sweep_us:.1f} us\n")
    print("| exchange step | us per step | chains with a partner | accepted swaps | algorithmic bytes | fraction of 8 TB/s | vs one sweep launch |")
    print("|---|---|---|---|---|---|---|")
    for parity, us, partnered, swaps, nbytes, frac in rows:
        print(f"| parity {parity} | {us:.1f} | {partnered:.0f} | {swaps:.0f} | {nbytes / 1e6:.1f} MB | {frac:.2f} | {us / sweep_us:.2f} |")
    print(f"\nHost time per round [sweep(1); exchange(1)], queue not drained: separate calls {host_sep:.1f} us, amc_sweep_exchange {host_one:.1f} us")
    eng.close()


if __name__ == "__main__":
    main()
