#!/usr/bin/env python3
"""Device time of one energy-histogram snapshot (amc_energy_histogram_accumulate) at M = 1e7 chains, R = 8, 200 bins, double well,
Float64, next to what reads the same bytes on the same handle: amc_histogram_rungs at the same bins, a bridge snapshot of E alone, one
single-sweep launch -- and the shapes around it: G = 1, Float32 state, one global-path shape (R x (bins + 3) above the static LDS cell
count), and a ladder whose cold rung sits in two or three bins (the same-address LDS atomics at their worst).  HIP-event timing
(amc_timing_begin / _end) over windows of LAUNCHES queued calls after a ramp, the windows of the figures alternating REPEATS times
(median and range of the windows); prints the markdown table of profiles/energy_histogram.md.

amc_histogram_rungs copies its counts to the host and synchronises in every call, so its figure includes that round trip; the
accumulating entries queue and return.

    python tools/time_energy_histogram.py [--chains 10000000] [--launches 100] [--repeats 7]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlo_amd import _capi   # noqa: E402

R = 8
BINS = (0.0, 16.0, 200)


def device_us(eng, call, n):
    eng.sync()
    eng.timing_begin()
    for _ in range(n):
        call()
    return eng.timing_end() * 1e3 / n


def make_engine(M, rungs, dtype="f64", betas=None):
    eng = _capi.HipEngine(n_chains=M, potential="double_well", beta=1.0, sigma=[0.5], weight=[1.0], seed=1, dtype=dtype)
    eng.init_uniform(-1.5, 1.5)
    if rungs:
        b = np.asarray(betas if betas is not None else 0.5 * 1.5 ** np.arange(rungs), dtype=np.float64)
        x = eng.download_state(want_e=False)[0]
        eng.upload_state(x, np.tile(b, M // rungs))
        eng.set_ladder(rungs)
    eng.sweep(300)                                       # ramp: clocks up, every rung near its own distribution
    eng.sync()
    return eng


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args(argv)
    M, n = args.chains - args.chains % (2 * R), args.launches
    ladder = make_engine(M, R)
    cold = make_engine(M, R, betas=[0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 64.0, 4000.0])      # the cold rung: e of order 1 / 4000, bin width 0.08
    flat = make_engine(M, 0)
    f32 = make_engine(M, R, dtype="f32")
    wide = make_engine(M, R)                             # 8 x (2000 + 3) cells: the global path
    acc = lambda eng, bins=BINS: (lambda: eng.energy_histogram_accumulate(*bins))
    figures = [("sweep", "one single-sweep launch", ladder, lambda: ladder.sweep_launches(1)),
               ("ehist", "one energy-histogram snapshot, R = 8, 200 bins", ladder, acc(ladder)),
               ("rungs", "amc_histogram_rungs at the same bins (x; copies to the host and synchronises)", ladder, lambda: ladder.histogram_rungs(*BINS)),
               ("bridge", "one bridge snapshot of E alone", ladder, lambda: ladder.bridge_accumulate(_capi.AMC_BRIDGE_E)),
               ("flat", "one energy-histogram snapshot, no ladder (G = 1)", flat, acc(flat)),
               ("f32", "the same as the second row with Float32 state", f32, acc(f32)),
               ("wide", "R = 8, 2000 bins: 16 024 cells, one global atomic per chain", wide, acc(wide, (0.0, 16.0, 2000))),
               ("cold", "R = 8, 200 bins, the cold rung in two or three bins (beta = 4000)", cold, acc(cold))]
    us = {k: [] for k, _, _, _ in figures}
    for _ in range(args.repeats):
        for key, _, eng, call in figures:
            us[key].append(device_us(eng, call, n if key != "rungs" else max(n // 10, 1)))
    med = {k: float(np.median(v)) for k, v in us.items()}
    print(f"M = {M}, double well, K = 1; {args.repeats} alternating windows of {n} queued calls per figure (median, min .. max)\n")
    print("| figure | us | vs one energy-histogram snapshot |")
    print("|---|---|---|")
    for key, text, _, _ in figures:
        print(f"| {text} | {med[key]:.1f} ({min(us[key]):.1f} .. {max(us[key]):.1f}) | {med[key] / med['ehist']:.2f} |")
    counts, n_snap, _ = cold.energy_histogram_fetch()
    row = counts[R - 1, :BINS[2]]
    print(f"\ncold rung: {int((row > 0).sum())} non-empty bins, the fullest holds {row.max() / max(row.sum(), 1):.3f} of its chains; "
          f"{n_snap} snapshots in the accumulator; rows sum to {counts.sum(axis=1)[0]} = snapshots x ladders: {counts.sum(axis=1)[0] == n_snap * (M // R)}")
    for eng in (ladder, cold, flat, f32, wide):
        eng.close()


if __name__ == "__main__":
    main()
