#!/usr/bin/env python3
"""Device time of one bridge snapshot (amc_bridge_accumulate) at M = 1e7, R = 8, harmonic, Float64, for three masks -- E alone, the
acceptance set E | EE | MF | MB, all six columns -- next to two yardsticks of the same handle in the same process: one
amc_reduce_rungs_exact(E) call and one single-sweep launch (boxes differ by a fixed cost per launch, so ratios to these travel where
microseconds do not).  HIP-event timing (amc_timing_begin / _end) over LAUNCHES calls per window after a ramp, the figures' windows
alternating REPEATS times (median and range of the windows); prints the markdown table of profiles/bridge_sums.md.

--rounds: device time per round of amc_sweep_exchange(n, 1) on a handle that never accumulates -- entries that exist unchanged before
the bridge sums did, so the same command on an older checkout gives the figure to compare with (the bridge-off path launches nothing
new) -- and, beside it, per round with a snapshot behind every round.

--blocks B [--chunk C]: the same figures with a jackknife partition set (amc_set_blocks; C = 0: the default chunk), the rows of
profiles/jackknife_blocks.md; amc_reduce_rungs_exact stays unpartitioned under a partition, so its row is the same yardstick.  Every
window begins with five untimed calls: the first snapshot allocates its accumulator, and an allocation waits for the stream.

    python tools/time_bridge.py [--chains 10000000] [--rungs 8] [--launches 300] [--repeats 7] [--potential harmonic] [--blocks 0] [--chunk 0] [--rounds]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlo_amd import _capi   # noqa: E402

MASKS = (("E", 1), ("E | EE | MF | MB", 1 | 2 | 16 | 32), ("all six", 63))


def device_us(eng, call, n):
    for _ in range(5):
        call()
    eng.sync()
    eng.timing_begin()
    for _ in range(n):
        call()
    return eng.timing_end() * 1e3 / n


def make_engine(M, R, potential="harmonic", blocks=0, chunk=0):
    betas = 0.5 * 1.3 ** np.arange(R)
    eng = _capi.HipEngine(n_chains=M, potential=potential, beta=1.0, sigma=[0.5], weight=[1.0], seed=1, per_chain_counters=False)
    eng.upload_state(np.zeros(M), np.tile(betas, M // R))
    eng.init_uniform(-2.0, 2.0)
    eng.set_ladder(R)
    if blocks:
        eng.set_blocks(blocks, chunk)
    for _ in range(3):                                   # ramp: clocks up, state equilibrated
        eng.sweep_exchange(200, 1)
    eng.sync()
    return eng


def cell(v):
    return f"{np.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--rungs", type=int, default=8)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--potential", default="harmonic", choices=("harmonic", "double_well"))
    ap.add_argument("--blocks", type=int, default=0, help="jackknife blocks B (0: no partition)")
    ap.add_argument("--chunk", type=int, default=0, help="ladders per chunk C (0: the default chunk)")
    ap.add_argument("--rounds", action="store_true", help="[sweep; exchange] rounds with the bridge off (and on)")
    args = ap.parse_args(argv)
    R, n = args.rungs, args.launches
    M = (args.chains // R) * R
    eng = make_engine(M, R, args.potential, args.blocks, args.chunk)
    part = f", B = {args.blocks}, C = {args.chunk or 'default'}" if args.blocks else ""
    print(f"M = {M}, R = {R}, {args.potential}, Float64, K = 1{part}; {args.repeats} alternating windows of {n} calls per figure (median, min .. max)\n")
    if args.rounds:
        off, on = [], []
        has_bridge = hasattr(eng, "bridge_accumulate")
        def rounds_with_snapshots():
            for _ in range(n):
                eng.sweep_exchange(1, 1)
                eng.bridge_accumulate(MASKS[1][1])
        for _ in range(args.repeats):
            off.append(device_us(eng, lambda: eng.sweep_exchange(n, 1), 1) / n)
            if has_bridge:
                on.append(device_us(eng, rounds_with_snapshots, 1) / n)
        print("| per round of [sweep; exchange] | us |")
        print("|---|---|")
        print(f"| bridge off (amc_sweep_exchange alone) | {cell(off)} |")
        if has_bridge:
            print(f"| a snapshot of E, EE, MF, MB behind every round | {cell(on)} |")
        eng.close()
        return
    us = {name: [] for name, _ in MASKS}
    us["reduce_rungs(E)"], us["sweep"] = [], []
    for _ in range(args.repeats):
        for name, mask in MASKS:
            eng.bridge_fetch(reset=True)                 # the mask is free again
            us[name].append(device_us(eng, lambda: eng.bridge_accumulate(mask), n))
        us["reduce_rungs(E)"].append(device_us(eng, lambda: eng.reduce_rungs(1), n))
        us["sweep"].append(device_us(eng, lambda: eng.sweep(1), n))
    rung, sweep = float(np.median(us["reduce_rungs(E)"])), float(np.median(us["sweep"]))
    nbytes = 8.0 * M + 8.0 * M                           # x and beta of every chain; the neighbours' beta are the same lines
    print("| call | us per call | vs reduce_rungs(E) | vs one sweep launch | fraction of 8 TB/s (x and beta once) |")
    print("|---|---|---|---|---|")
    for name, _ in MASKS:
        med = float(np.median(us[name]))
        print(f"| bridge_accumulate({name}) | {cell(us[name])} | {med / rung:.2f} | {med / sweep:.2f} | {nbytes / (med * 1e-6) / 8e12:.2f} |")
    print(f"| reduce_rungs(E) (synchronises per call) | {cell(us['reduce_rungs(E)'])} | 1.00 | {rung / sweep:.2f} | |")
    print(f"| one single-sweep launch | {cell(us['sweep'])} | {sweep / rung:.2f} | 1.00 | |")
    eng.close()


if __name__ == "__main__":
    main()
