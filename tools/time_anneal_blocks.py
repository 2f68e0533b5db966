#!/usr/bin/env python3
"""Device time of one population-annealing step (amc_anneal) at M = 1e7, harmonic, Float64, with families on -- the step as it was --
against the same step under a partition into blocks of families (amc_set_anneal_blocks): B = 32 with the default chunk (a block is a
contiguous range of ancestors: the wave-uniform path) and B = 64 with chunk 1 (neighbouring families in different blocks: lanes deposit
one by one wherever a wave holds more than one family).  HIP-event timing (amc_timing_begin / _end) over windows of LAUNCHES steps with
one sweep behind each, as a run does; the windows of the figures alternate REPEATS times on the same box in the same run (median and
range of the windows), and the sweeps' own time, measured the same way, is taken off.  In the same run: one energy-histogram pass of
the population, plain (amc_energy_histogram_accumulate) against per block of families (amc_energy_histogram_accumulate_blocks under
the partition), at 188 bins (B = 64: the rows fit the LDS cells) and at 190 bins (B = 64: one global atomic per chain).  The families start afresh in front of every
window, so that every window sees the same mix of families per wave.  Prints the markdown table of
profiles/population_annealing_blocks.md.

    python tools/time_anneal_blocks.py [--chains 10000000] [--launches 50] [--repeats 7] [--step 0.02]
"""
import argparse
import os
import sys

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
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step", type=float, default=0.02)
    args = ap.parse_args(argv)
    M, n = args.chains, args.launches
    eng = _capi.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=1, per_chain_counters=False)
    eng.init_uniform(-2.0, 2.0)
    eng.sweep(600)                                       # ramp: clocks up, state equilibrated
    eng.sync()
    flip = [0]

    def round_():
        flip[0] ^= 1
        eng.anneal(1.0 + args.step * flip[0])
        eng.sweep(1)

    forms = {"families": None, "blocks32": (32, 0), "blocks64c1": (64, 1)}
    us = {k: [] for k in ("sweep", *forms)}
    last = {}
    for _ in range(args.repeats):
        us["sweep"].append(device_us(eng, lambda: eng.sweep(1), n))
        for name, part in forms.items():
            eng.set_anneal_families(True)                # afresh: fam[c] = c, the partition off
            if part:
                eng.set_anneal_blocks(*part)
            us[name].append(device_us(eng, round_, n))
            rec = eng.anneal_records(reset=True)
            if part:
                blk = eng.anneal_block_records(reset=True)
                assert np.array_equal(blk[:, 1].sum(axis=1), rec[:, 4]) and np.all(blk[:, 0].sum(axis=1) == M)
                last[name] = blk[-1]
    # one histogram pass: plain, then per block of families (the population as the rounds above left it)
    hist = {(n, B): [] for n in (188, 190) for B in (0, 32, 64)}
    for _ in range(args.repeats):
        for (nb, B), out in hist.items():
            eng.set_anneal_blocks(B)
            if B:
                out.append(device_us(eng, lambda: eng.energy_histogram_accumulate_blocks(0.0, 4.0, nb), n))
                eng.energy_histogram_fetch_blocks(reset=True)
            else:
                out.append(device_us(eng, lambda: eng.energy_histogram_accumulate(0.0, 4.0, nb), n))
                eng.energy_histogram_fetch(reset=True)
    med = {k: float(np.median(v)) for k, v in us.items()}
    s, base = med["sweep"], med["families"] - med["sweep"]
    cell = lambda k, off=0.0: f"{med[k] - off:.1f} ({min(us[k]) - off:.1f} .. {max(us[k]) - off:.1f})"
    print(f"M = {M}, harmonic, Float64, K = 1, beta 1 <-> {1.0 + args.step}; {args.repeats} alternating windows of {n} [anneal; sweep] rounds per "
          f"figure, the sweep's median taken off (median, min .. max)\n")
    print("| figure | us | vs the step with families on |")
    print("|---|---|---|")
    print(f"| one single-sweep launch | {cell('sweep')} | |")
    print(f"| one annealing step, families on, no partition | {cell('families', s)} | 1 |")
    print(f"| the same under B = 32, default chunk | {cell('blocks32', s)} | {(med['blocks32'] - s) / base:.3f} |")
    print(f"| the same under B = 64, chunk 1 | {cell('blocks64c1', s)} | {(med['blocks64c1'] - s) / base:.3f} |")
    print(f"\nlast block record under B = 32: blocks alive {int((last['blocks32'][0] > 0).sum())}, largest n_b / M = {int(last['blocks32'][0].max()) / M:.4f}")
    print("\n| one energy-histogram pass | us | vs the plain pass |")
    print("|---|---|---|")
    for (nb, B), v in hist.items():
        m, base_h = float(np.median(v)), float(np.median(hist[(nb, 0)]))
        what = "plain" if not B else f"per block of families, B = {B} ({B * (nb + 3)} cells: {'LDS' if B * (nb + 3) <= 12288 else 'global atomics'})"
        print(f"| {nb} bins, {what} | {m:.1f} ({min(v):.1f} .. {max(v):.1f}) | {m / base_h:.3f} |")
    eng.close()


if __name__ == "__main__":
    main()
