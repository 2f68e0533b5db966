#!/usr/bin/env python3
"""Device time of one energy-histogram snapshot kept per jackknife block (amc_energy_histogram_accumulate_blocks) at M = 1e7 chains,
R = 8, 200 bins, double well, Float64, beside the plain snapshot (amc_energy_histogram_accumulate) on a handle of the same shape in
the same run: B = 32 with the default chunk (32 ladders), B = 2 and B = 64, a chunk of ONE ladder (the traversal at its worst: a HIP
block reads one ladder of 8 chains per chunk), and the global path (2000 bins).  HIP-event timing (amc_timing_begin / _end) over
windows of LAUNCHES queued calls after a ramp, the figures' windows alternating REPEATS times (median and range); prints the markdown
table of profiles/energy_histogram_blocks.md.

    python tools/time_energy_histogram_blocks.py [--chains 10000000] [--launches 100] [--repeats 7]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlo_amd import _capi   # noqa: E402
from tools.time_energy_histogram import BINS, R, device_us, make_engine   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args(argv)
    M, n = args.chains - args.chains % (2 * R), args.launches
    wide_bins = (0.0, 16.0, 2000)
    shapes = [("plain", "plain snapshot, no partition (the baseline)", None, BINS),
              ("b32", "per block, B = 32, default chunk (32 ladders)", (32, 0), BINS),
              ("b2", "per block, B = 2, default chunk", (2, 0), BINS),
              ("b64", "per block, B = 64, default chunk", (64, 0), BINS),
              ("c1", "per block, B = 32, chunk of ONE ladder", (32, 1), BINS),
              ("wide_plain", "plain snapshot, 2000 bins: one global atomic per chain", None, wide_bins),
              ("wide_b32", "per block, B = 32, 2000 bins: one global atomic per chain", (32, 0), wide_bins)]
    figures = []
    for key, text, part, bins in shapes:
        eng = make_engine(M, R)
        if part:
            eng.set_blocks(*part)
            call = (lambda e=eng, b=bins: e.energy_histogram_accumulate_blocks(*b))
        else:
            call = (lambda e=eng, b=bins: e.energy_histogram_accumulate(*b))
        call()                                           # the first call allocates (and, per block, waits for the stream)
        figures.append((key, text, eng, call))
    us = {k: [] for k, _, _, _ in figures}
    for _ in range(args.repeats):
        for key, _, eng, call in figures:
            us[key].append(device_us(eng, call, n))
    med = {k: float(np.median(v)) for k, v in us.items()}
    print(f"M = {M}, R = {R}, double well, K = 1; {args.repeats} alternating windows of {n} queued calls per figure (median, min .. max)\n")
    print("| figure | us | vs the plain snapshot |")
    print("|---|---|---|")
    for key, text, _, _ in figures:
        base = med["wide_plain"] if key.startswith("wide") else med["plain"]
        print(f"| {text} | {med[key]:.1f} ({min(us[key]):.1f} .. {max(us[key]):.1f}) | {med[key] / base:.2f} |")
    for key, _, eng, _ in figures:                       # the counts are what they must be: every row sums to snapshots x ladders
        counts, n_snap, _ = eng.energy_histogram_fetch()
        assert n_snap == 1 + args.repeats * n and np.all(counts.sum(axis=1) == n_snap * (M // R)), key
        eng.close()
    print(f"\nevery accumulator: {1 + args.repeats * n} snapshots, every row sums to snapshots x ladders")


if __name__ == "__main__":
    main()
