#!/usr/bin/env python3
"""Developer tool: the ladder behind the defaults of AMC_SWEEP_SLICES / AMC_SWEEP_SLICE_BLOCKS_PER_CU / AMC_SWEEP_SLICE_MIN_CHAINS.
The headline workload (K = 1 harmonic, pool-wide counter) as calls of N single-sweep launches, for every ensemble size and every
(slices, blocks per CU per slice); S = 1 is the whole launch in its own default grid.  HIP events around each call, us per STEP.
Every figure comes from a process of its own with ONE engine in it, as bench.py has it: which hardware queues a handle's streams land
on depends on the streams the process made before, and several engines in one process measure that instead.  The configurations of
one size are interleaved ROUNDS times; the table shows each configuration's rounds side by side.
usage (GPU box): python3 tools/time_sliced_launches.py [--sizes 1000000,2500000,10000000,40000000] [--launches 2000] [--rounds 2]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("AMC_PKG_ROOT", ROOT))



def engine(m, slices, bpc):
    os.environ["AMC_SWEEP_SLICES"] = str(slices)
    os.environ["AMC_SWEEP_SLICE_MIN_CHAINS"] = "0"
    if bpc:
        os.environ["AMC_SWEEP_SLICE_BLOCKS_PER_CU"] = str(bpc)
    else:
        os.environ.pop("AMC_SWEEP_SLICE_BLOCKS_PER_CU", None)
    from montecarlo_amd import _capi as A
    e = A.HipEngine(n_chains=m, potential="harmonic", beta=2.0, sigma=[0.5], weight=[1.0], seed=1, sweepstep=1, per_chain_counters=False)
    e.init_uniform(-2.0, 2.0)
    return e


def one(m, slices, bpc, n):
    """the child: one engine, a ramp, two timed calls; prints the faster, us per step"""
    e = engine(m, slices, bpc)
    for _ in range(3):
        e.sweep_launches(n)
    e.sync()
    us = []
    for _ in range(2):
        e.sweep_launches(200)
        e.sync()
        e.timing_begin()
        e.sweep_launches(n)
        us.append(e.timing_end() * 1e3 / n)
    e.close()
    print("%.3f" % min(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,2500000,10000000,40000000")
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--slices", default="2,3")
    ap.add_argument("--blocks", default="2,3,4,6")
    ap.add_argument("--one", nargs=4, type=int, metavar=("M", "S", "B", "N"), help="(the child's arguments)")
    args = ap.parse_args()
    if args.one:
        return one(*args.one)
    configs = [(1, 0)] + [(s, b) for s in map(int, args.slices.split(",")) for b in map(int, args.blocks.split(","))]
    for m in map(int, args.sizes.split(",")):
        n = max(200, min(args.launches, int(args.launches * 1e7 / m)))
        us = [[] for _ in configs]
        for _ in range(args.rounds):
            for i, (s, b) in enumerate(configs):      # one GPU process at a time; a child that fails ends the ladder
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(m), str(s), str(b), str(n)],
                                   capture_output=True, text=True, timeout=120)
                if r.returncode != 0:
                    raise SystemExit(f"child {m} S={s} b={b} failed with {r.returncode}:\n{r.stderr[-2000:]}")
                us[i].append(float(r.stdout.split()[-1]))
        base = min(us[0])
        print(f"{m} chains, calls of {n} launches, us per step by round (S = 1: {' '.join('%.2f' % v for v in us[0])})", flush=True)
        for (s, b), v in list(zip(configs, us))[1:]:
            print(f"  S={s} blocks/CU/slice={b}: {' '.join('%.2f' % x for x in v)}   best vs S=1 best: {100 * (min(v) / base - 1):+.1f} %", flush=True)


if __name__ == "__main__":
    main()
