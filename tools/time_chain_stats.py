#!/usr/bin/env python3
"""Device time of one sample of the convergence sums (amc_chain_stats_accumulate) and of one fetch (amc_chain_stats_fetch) at M = 1e7
chains, R = 8, double well, both observables and both state types, next to what runs on the same handle in the same run: a mark and a
sample of the time correlation, a bridge snapshot of E alone, one single-sweep launch.  HIP-event timing (amc_timing_begin / _end) over
windows of LAUNCHES queued calls after a ramp and one untimed call of every figure (run-time builds happen there), the windows of the
figures alternating REPEATS times (median and range of the windows); prints the markdown tables of profiles/chain_stats.md.

WHERE THE BYTES COME FROM.  A window of identical passes at 1e7 chains works on x and ONE part's S and Q, 240 MB at Float64 state:
that fits the 256 MiB of the Infinity Cache, as the 80 MB of a single-sweep launch do, so those figures are cache-resident ones.  Two
further figures take the cache out: "alternating parts" queues the passes into part 0 and part 1 in turn at 1e7 chains -- x and both
parts, 400 MB, more than the cache holds, every pass finds its S and Q evicted by the one before --, and a second table repeats the
accumulate pass, the corr mark and the sweep at --hbm-chains (4e7: 960 MB per accumulate pass, 320 MB per sweep).

A fetch copies its 56 records to the host and synchronises in every call, so its figure includes that round trip; the other entries
queue and return.  The bytes of a figure are what its kernels read and write per chain (state, accumulators, origin values); the
bandwidth column divides them by the time.  A corr sample is timed as [mark; sample] pairs (a mark holds 256 slots, a window of
samples alone would overrun them) less the median of a mark.

    python tools/time_chain_stats.py [--chains 10000000] [--hbm-chains 40000000] [--launches 100] [--repeats 7]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlo_amd import _capi   # noqa: E402

R = 8
XB = {"f64": 8, "f32": 4}


def device_us(eng, call, n):
    eng.sync()
    eng.timing_begin()
    for _ in range(n):
        call()
    return eng.timing_end() * 1e3 / n


def make_engine(M, dtype):
    eng = _capi.HipEngine(n_chains=M, potential="double_well", beta=1.0, sigma=[0.5], weight=[1.0], seed=1, dtype=dtype)
    eng.init_uniform(-1.5, 1.5)
    x = eng.download_state(want_e=False)[0]
    eng.upload_state(x, np.tile(0.5 * 1.5 ** np.arange(R), M // R))
    eng.set_ladder(R)
    eng.sweep(300)                                       # ramp: clocks up, every rung near its own distribution
    eng.sync()
    return eng


def figures_of(eng, dtype, kinds, n, full):
    """(key, text, call, bytes per chain, calls per window, what puts the handle into the figure's state)."""
    xb, out = XB[dtype], []
    for kind in kinds:
        def begin(eng=eng, kind=kind):                   # the sums of this observable stand (both parts), the mark of the same one too
            eng.chain_stats_clear()
            eng.chain_stats_accumulate(kind, 0)
            eng.chain_stats_accumulate(kind, 1)
            eng.corr_mark(kind)

        def alternate(eng=eng, kind=kind, turn=[0]):
            turn[0] ^= 1
            eng.chain_stats_accumulate(kind, turn[0])
        tag = f"{dtype} {kind}"
        out += [(f"acc {tag}", f"one accumulate pass, {tag}", lambda eng=eng, kind=kind: eng.chain_stats_accumulate(kind, 1), xb + 32, n, begin),
                (f"alt {tag}", f"one accumulate pass, alternating parts, {tag}", alternate, xb + 32, n, begin)]
        if full:
            out += [(f"fetch {tag}", f"one fetch (sums by group, finish, copy, wait), {tag}", lambda eng=eng: eng.chain_stats_fetch(), 32, max(n // 10, 1), begin)]
        out += [(f"mark {tag}", f"a corr mark, {tag}", lambda eng=eng, kind=kind: eng.corr_mark(kind), xb + 8, n, begin)]
        if full:
            out += [(f"sample {tag}", f"a corr sample, {tag}", lambda eng=eng, kind=kind: (eng.corr_mark(kind), eng.corr_sample())[0], xb + 8, n, begin)]
    if full:
        out += [(f"bridge {dtype}", f"a bridge snapshot of E alone, {dtype}", lambda eng=eng: eng.bridge_accumulate(_capi.AMC_BRIDGE_E), 2 * xb, n, None)]
    out += [(f"sweep {dtype}", f"one single-sweep launch, {dtype}", lambda eng=eng: eng.sweep_launches(1), 2 * xb, n, None)]
    return [(eng,) + f for f in out]


def table(M, figures, repeats, n):
    for eng, _, _, call, _, _, begin in figures:         # one untimed call of every figure: what is built at run time is built here
        if begin:
            begin()
        call()
        eng.sync()
    us = {f[1]: [] for f in figures}
    for _ in range(repeats):
        for eng, key, _, call, _, calls, begin in figures:
            if begin:
                begin()
            us[key].append(device_us(eng, call, calls))
    med = {k: float(np.median(v)) for k, v in us.items()}
    lo, hi = {k: min(v) for k, v in us.items()}, {k: max(v) for k, v in us.items()}
    for key in [k for k in med if k.startswith("sample")]:      # the pair less the mark
        mark = med["mark" + key[len("sample"):]]
        med[key], lo[key], hi[key] = med[key] - mark, lo[key] - mark, hi[key] - mark
    print(f"M = {M}, R = {R}, double well, K = 1; {repeats} alternating windows of {n} queued calls per figure (a fetch: {max(n // 10, 1)}); median "
          "(min .. max) of the windows\n")
    print("| figure | us | bytes per chain | GB/s | vs the accumulate pass of its state type and observable |")
    print("|---|---|---|---|---|")
    for _, key, text, _, nbytes, _, _ in figures:
        words = key.split()
        base = med[f"acc {words[1]} {words[2] if len(words) > 2 else 'energy'}"]
        print(f"| {text} | {med[key]:.1f} ({lo[key]:.1f} .. {hi[key]:.1f}) | {nbytes} | {nbytes * M / med[key] / 1e3:.0f} | {med[key] / base:.2f} |")
    print("\n| accumulate pass | us | its bytes at the corr mark's bandwidth, us | ratio | vs a single-sweep launch |")
    print("|---|---|---|---|---|")
    for _, key, text, _, nbytes, _, _ in figures:
        if key.startswith(("acc", "alt")):
            _, dtype, kind = key.split()
            want = nbytes * med[f"mark {dtype} {kind}"] / (XB[dtype] + 8)
            print(f"| {text[len('one accumulate pass, '):]} | {med[key]:.1f} | {want:.1f} | {med[key] / want:.2f} | {med[key] / med[f'sweep {dtype}']:.2f} |")
    print()
    return med


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--hbm-chains", type=int, default=40_000_000, help="chains of the second table, beyond the Infinity Cache (0: none)")
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args(argv)
    M, n = args.chains - args.chains % (2 * R), args.launches
    engines = {dtype: make_engine(M, dtype) for dtype in XB}
    table(M, [f for dtype, eng in engines.items() for f in figures_of(eng, dtype, ("energy", "x"), n, True)], args.repeats, n)
    for eng in engines.values():
        eng.close()
    if args.hbm_chains:
        Mh = args.hbm_chains - args.hbm_chains % (2 * R)
        eng = make_engine(Mh, "f64")
        table(Mh, figures_of(eng, "f64", ("energy", "x"), max(n // 4, 1), False), args.repeats, max(n // 4, 1))
        eng.close()


if __name__ == "__main__":
    main()
