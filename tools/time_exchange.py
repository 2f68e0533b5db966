#!/usr/bin/env python3
"""Device time of one exchange step (amc_exchange(1)) at M = 1e7, R = 8, harmonic, Float64, next to one single-sweep launch of the
same handle, and host time per round of amc_sweep_exchange against the separate calls.  HIP-event timing (amc_timing_begin / _end)
over LAUNCHES launches after a ramp; prints the markdown table of profiles/exchange.md.

--track: the step of a handle with walker tracking on (exchange_tracked_kernel) against the step of a handle without, the two handles
side by side in this process from the same start, their timed windows alternating REPEATS times (median and range of the windows),
and one amc_flow_rungs call; prints the markdown table of profiles/exchange_tracking.md.

    python tools/time_exchange.py [--chains 10000000] [--rungs 8] [--launches 400] [--track [--repeats 7]]
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


def make_engine(M, R, track):
    L = M // R
    betas = 0.5 * 1.3 ** np.arange(R)
    eng = _capi.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=1, per_chain_counters=False)
    eng.upload_state(np.zeros(M), np.tile(betas, L))
    eng.init_uniform(-2.0, 2.0)
    eng.set_ladder(R)
    if track:
        eng.set_tracking(True)
    for _ in range(3):                                   # ramp: clocks up, state equilibrated, walkers spread over the rungs
        eng.sweep_exchange(200, 1)
    eng.sync()
    return eng


def track_main(args):
    R, n = args.rungs, args.launches
    M = (args.chains // R) * R
    plain, tracked = make_engine(M, R, False), make_engine(M, R, True)
    xp, xt = plain.download_state(want_e=False)[0], tracked.download_state(want_e=False)[0]
    assert np.array_equal(xp.view(np.uint64), xt.view(np.uint64)), "tracking changed the positions"
    print(f"M = {M}, R = {R}, harmonic, Float64, K = 1; {args.repeats} alternating windows of {n} launches per figure (median, min .. max)\n")
    print("| exchange step | untracked us | tracked us | tracked / untracked | accepted swaps per step | bytes tracked / untracked |")
    print("|---|---|---|---|---|---|")
    for parity in (0, 1):
        us = {False: [], True: []}
        swaps = attempts = 0.0
        for _ in range(args.repeats):
            for eng, key in ((plain, False), (tracked, True)):
                def step():
                    eng.exchange_step = parity           # the same parity every launch
                    eng.exchange(1)
                a0, t0 = eng.exchange_counters()
                us[key].append(device_us(eng, step, n))
                a1, t1 = eng.exchange_counters()
                swaps, attempts = (a1 - a0).sum() / n, (t1 - t0).sum() / n
        med = {k: float(np.median(v)) for k, v in us.items()}
        nbytes = {False: 32.0 * attempts + 16.0 * swaps, True: 34.0 * attempts + 18.0 * swaps}
        cell = lambda k: f"{med[k]:.1f} ({min(us[k]):.1f} .. {max(us[k]):.1f})"
        print(f"| parity {parity} | {cell(False)} | {cell(True)} | {med[True] / med[False]:.3f} | {swaps:.0f} of {attempts:.0f} | {nbytes[True] / nbytes[False]:.3f} |")
    host, dev = [], []
    for _ in range(args.repeats):
        tracked.sync()
        t = time.perf_counter()
        flow = tracked.flow_rungs()
        host.append((time.perf_counter() - t) * 1e6)
        dev.append(device_us(tracked, tracked.flow_rungs, 20))
    rt, up = tracked.tracking_counters()
    with np.errstate(invalid="ignore"):
        f = flow[:, 1] / (flow[:, 1] + flow[:, 2])
    print(f"\none amc_flow_rungs call (memset, rung_flow_kernel, copy of {3 * R} counts, synchronise): host {np.median(host):.1f} us "
          f"({min(host):.1f} .. {max(host):.1f}); stream time per call over 20 back-to-back calls {np.median(dev):.1f} us ({min(dev):.1f} .. {max(dev):.1f})")
    print(f"round trips {rt}, up trips {up} over {M // R} ladders; f(r) = " + " ".join(f"{v:.3f}" for v in f))
    plain.close()
    tracked.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--rungs", type=int, default=8)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--track", action="store_true", help="tracked against untracked steps, and one amc_flow_rungs")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args(argv)
    if args.track:
        return track_main(args)
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
