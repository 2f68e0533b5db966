#!/usr/bin/env python3
"""Time of the per-rung reproducible sums (amc_reduce_rungs_exact) at M = 1e7, harmonic, Float64, next to (a) amc_reduce, the
whole-ensemble pass over the same bytes, and (c) the host pass rung_energy makes (R strided downloads, potential and np.sum on the
host).  Every figure is a whole CALL -- launches, the copy of the records and the host's wait --: wall clock around calls that start from
an idle stream, REPEATS of them after a warm-up; median and the spread (min .. max).  Prints the markdown table of
profiles/rung_sums.md.  On a library without the entry (the parent commit) rows (b) are left out.

    python tools/time_rung_sums.py [--chains 10000000] [--repeats 50]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlo_amd import _capi   # noqa: E402


def timed(eng, call, repeats, warmup=5):
    for _ in range(warmup):
        call()
    out = []
    for _ in range(repeats):
        eng.sync()
        t = time.perf_counter()
        call()
        out.append((time.perf_counter() - t) * 1e6)
    out = np.array(out)
    return float(np.median(out)), float(out.min()), float(out.max())


def engine(M, R):
    eng = _capi.HipEngine(n_chains=M, potential="harmonic", beta=1.0, sigma=[0.5], weight=[1.0], seed=1, per_chain_counters=False)
    eng.upload_state(np.zeros(M), np.tile(0.5 * 1.3 ** np.arange(R), M // R))
    eng.init_uniform(-2.0, 2.0)
    eng.set_ladder(R)
    eng.sweep_exchange(50, 1)                            # clocks up, state equilibrated
    eng.sync()
    return eng


def host_rung_energy(eng, R, count):
    """The pass of montecarlo_amd.exchange.rung_energy on one shard: one strided download per rung, x * x and a plain sum."""
    return np.array([float(np.sum(np.square(eng.download_strided(r, R, count)))) for r in range(R)]) / count


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=50)
    args = ap.parse_args(argv)
    rows = []
    base = None
    for R, cols_list in [(8, [7, 1]), (64, [7]), (7, [7])]:
        M = (args.chains // R) * R
        eng = engine(M, R)
        if base is None:
            base = timed(eng, eng.reduce, args.repeats)
            rows.append(("(a) `amc_reduce`, whole ensemble", M, base))
            host = timed(eng, lambda: host_rung_energy(eng, R, M // R), max(3, args.repeats // 10), warmup=1)
            rows.append((f"(c) host pass of `rung_energy`, R = {R}", M, host))
        if hasattr(eng, "reduce_rungs"):
            for cols in cols_list:
                what = "all columns" if cols == 7 else "sum e only"
                rows.append((f"(b) `amc_reduce_rungs_exact`, R = {R}, {what}", M, timed(eng, lambda: eng.reduce_rungs(cols), args.repeats)))
        eng.close()
    print(f"harmonic, Float64, K = 1; wall clock per call from an idle stream, {args.repeats} repeats after 5 warm-up calls\n")
    print("| call | chains | median us | min .. max us | ratio to (a) |")
    print("|---|---|---|---|---|")
    for name, M, (med, lo, hi) in rows:
        print(f"| {name} | {M} | {med:.1f} | {lo:.1f} .. {hi:.1f} | {med / base[0]:.2f} |")


if __name__ == "__main__":
    main()
