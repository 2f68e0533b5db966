#!/usr/bin/env python3
"""Stream time of one ladder respacing (amc_respace_ladder, local counts) at M = 1e7, R = 8, harmonic, Float64, with tracking on and
off, next to one exchange step and one single-sweep launch of the same handle.  HIP-event timing (amc_timing_begin / _end).

A respacing that is taken zeroes the counts it reads, so the next one would be refused (status 2) and its retile pass would return at
once.  A timed window is therefore [2R exchange steps; one respacing], which gives every respacing counts to work with, and the same
window without the respacing is timed beside it: the difference is the respacing.  Windows alternate REPEATS times (median, min .. max);
respace_status() afterwards must count one status-0 respacing per window.  Prints the markdown table of profiles/ladder_respacing.md.

    python tools/time_respace.py [--chains 10000000] [--rungs 8] [--windows 50] [--repeats 7]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlo_amd import _capi   # noqa: E402
from time_exchange import device_us, make_engine   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--rungs", type=int, default=8)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args(argv)
    R, n = args.rungs, args.windows
    M = (args.chains // R) * R
    print(f"M = {M}, R = {R}, harmonic, Float64, K = 1; {args.repeats} alternating pairs of windows, {n} x [{2 * R} exchange steps (; respacing)] each "
          f"(median, min .. max)\n")
    print("| tracking | rule | window without us | window with us | one respacing us | one exchange step us | one single-sweep launch us | respacing / exchange step |")
    print("|---|---|---|---|---|---|---|---|")
    for track in (False, True):
        eng = make_engine(M, R, track)
        sweep_us = device_us(eng, lambda: eng.sweep(1), 200)
        for rule in (("acceptance", "flow") if track else ("acceptance",)):
            base, full = [], []
            n0 = eng.respace_status()[1]
            for _ in range(args.repeats):
                base.append(device_us(eng, lambda: eng.exchange(2 * R), n))
                full.append(device_us(eng, lambda: (eng.exchange(2 * R), eng.respace_ladder(rule, 0.5, 0.01)), n))
            status, n1 = eng.respace_status()
            assert status == 0 and n1 - n0 == args.repeats * n, (status, n1 - n0)
            b, f = float(np.median(base)), float(np.median(full))
            step = b / (2 * R)
            cell = lambda v: f"{np.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"
            print(f"| {'on' if track else 'off'} | {rule} | {cell(base)} | {cell(full)} | {f - b:.1f} | {step:.1f} | {sweep_us:.1f} | {(f - b) / step:.2f} |")
        print(f"<!-- ladder after the windows (tracking {'on' if track else 'off'}): " + " ".join(f"{v:.4f}" for v in eng.ladder()) + " -->")
        eng.close()


if __name__ == "__main__":
    main()
