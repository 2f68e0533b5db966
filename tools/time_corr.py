#!/usr/bin/env python3
"""Device time of one mark (amc_corr_mark) and one sample (amc_corr_sample) of the time correlation at M = 1e7, harmonic, Float64,
for R = 1 (no ladder: one group) and R = 8, next to the two passes they most resemble on the same handle in the same process: one
amc_reduce_rungs_exact(E) call and one bridge snapshot with the columns E | EE (R = 8 only: both need a ladder).  tools/time_bridge.py's
method: HIP-event timing (amc_timing_begin / _end) over LAUNCHES calls per window after a ramp, the figures' windows alternating
REPEATS times (median and range of the windows); prints the markdown table of profiles/time_correlation.md.  A window of samples
re-marks every 255 calls (a mark has 256 slots); the mark's share of such a window is below half a percent.

--blocks B [--chunk C]: the same figures with a jackknife partition set (amc_set_blocks; C = 0: the default chunk), the rows of
profiles/jackknife_blocks.md.  Every window begins with five untimed calls, and with a partition one untimed mark with all its 255
samples comes first: the blocked accumulator grows with the slots in use, and an allocation waits for the stream.

    python tools/time_corr.py [--chains 10000000] [--launches 300] [--repeats 7] [--observable energy] [--potential harmonic] [--blocks 0] [--chunk 0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlo_amd import _capi   # noqa: E402


def device_us(eng, call, n):
    for _ in range(5):
        call()
    eng.sync()
    eng.timing_begin()
    for _ in range(n):
        call()
    return eng.timing_end() * 1e3 / n


def make_engine(M, R, potential="harmonic", blocks=0, chunk=0):
    eng = _capi.HipEngine(n_chains=M, potential=potential, beta=1.0, sigma=[0.5], weight=[1.0], seed=1, per_chain_counters=False)
    if R > 1:
        eng.upload_state(np.zeros(M), np.tile(0.5 * 1.3 ** np.arange(R), M // R))
    eng.init_uniform(-2.0, 2.0)
    if R > 1:
        eng.set_ladder(R)
    if blocks:
        eng.set_blocks(blocks, chunk)
    for _ in range(3):                                   # ramp: clocks up, state equilibrated
        eng.sweep(200)
    eng.sync()
    return eng


def cell(v):
    return f"{np.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--observable", default="energy", choices=("energy", "x"))
    ap.add_argument("--potential", default="harmonic", choices=("harmonic", "double_well"))
    ap.add_argument("--blocks", type=int, default=0, help="jackknife blocks B (0: no partition)")
    ap.add_argument("--chunk", type=int, default=0, help="ladders (chains without a ladder) per chunk C (0: the default chunk)")
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8], help="R of the handles timed (1: no ladder)")
    args = ap.parse_args(argv)
    n = args.launches
    for R in args.groups:
        M = (args.chains // R) * R
        eng = make_engine(M, R, args.potential, args.blocks, args.chunk)
        state = {"left": 0}

        def sample():
            if state["left"] == 0:
                eng.corr_mark(args.observable)
                state["left"] = 255
            eng.corr_sample()
            state["left"] -= 1

        if args.blocks:
            for _ in range(255):
                sample()
        us = {"mark": [], "sample": [], "reduce_rungs(E)": [], "bridge(E | EE)": [], "sweep": []}
        for _ in range(args.repeats):
            us["mark"].append(device_us(eng, lambda: eng.corr_mark(args.observable), n))
            state["left"] = 0
            us["sample"].append(device_us(eng, sample, n))
            if R > 1:
                us["reduce_rungs(E)"].append(device_us(eng, lambda: eng.reduce_rungs(1), n))
                eng.bridge_fetch(reset=True)
                us["bridge(E | EE)"].append(device_us(eng, lambda: eng.bridge_accumulate(3), n))
            us["sweep"].append(device_us(eng, lambda: eng.sweep(1), n))
        part = f", B = {args.blocks}, C = {args.chunk or 'default'}" if args.blocks else ""
        print(f"\nM = {M}, R = {R}, {args.potential}, Float64, K = 1{part}, observable {args.observable}; {args.repeats} alternating windows of {n} calls "
              "per figure (median, min .. max)\n")
        print("| call | us per call | bytes per chain | fraction of 8 TB/s | vs bridge(E | EE) | vs one sweep launch |")
        print("|---|---|---|---|---|---|")
        sweep = float(np.median(us["sweep"]))
        bridge = float(np.median(us["bridge(E | EE)"])) if R > 1 else float("nan")
        for name, nbytes in (("mark", 16), ("sample", 16), ("reduce_rungs(E)", 8), ("bridge(E | EE)", 16), ("sweep", 16)):
            if not us[name]:
                continue
            med = float(np.median(us[name]))
            note = {"mark": "corr_mark (reads x, writes a)", "sample": "corr_sample (reads x and a)", "reduce_rungs(E)": "reduce_rungs(E) (synchronises per call)",
                    "bridge(E | EE)": "bridge_accumulate(E | EE) (reads x and beta)", "sweep": "one single-sweep launch"}[name]
            print(f"| {note} | {cell(us[name])} | {nbytes} | {nbytes * M / (med * 1e-6) / 8e12:.2f} | {med / bridge:.2f} | {med / sweep:.2f} |")
        eng.close()


if __name__ == "__main__":
    main()
