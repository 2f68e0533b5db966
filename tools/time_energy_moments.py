#!/usr/bin/env python3
"""Device time of one snapshot of the moments per energy bin (amc_energy_moments_accumulate) at M = 1e7 chains, R = 8, 200 bins,
double well, Float64, beside the plain energy-histogram snapshot (amc_energy_histogram_accumulate) of the same handle measured in the
same run: the mask X, X | XX and all three columns; the same three on a ladder whose cold rung sits in one or two bins (its chains'
LDS atomics on the same few addresses, the 64-bit sum cells included); amc_reduce_rungs_exact for scale.  HIP-event timing
(amc_timing_begin / _end) over windows of LAUNCHES queued calls after a ramp, the windows of the figures alternating REPEATS times
(median and range of the windows); prints the markdown table of profiles/energy_moments.md.

A moments accumulator holds fewer than 2^31 / (M / R) snapshots (1717 at 1e7 chains, R = 8) and has one form while it stands, so every
window begins with a fetch with reset and one call that allocates the new accumulator, both outside the timed region.
amc_reduce_rungs_exact copies its records to the host and synchronises in every call, so its figure includes that round trip.

With --blocks B the tool times the pass per jackknife block instead (amc_energy_moments_accumulate_blocks; DESIGN.md section 3.17
"Moments per block") beside the plain moments pass of the same handle in the same run: one, two and three columns under the
partition (B, default chunk), and all three columns under chunks of ONE ladder, the bad case (every chunk is a trip of its own for
G lanes of a HIP block).  It prints the markdown table of profiles/energy_moments_blocks.md.

    python tools/time_energy_moments.py [--chains 10000000] [--launches 50] [--repeats 5] [--blocks 32]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlo_amd import _capi   # noqa: E402

R = 8
BINS = (0.0, 16.0, 200)
X_BOUND = 4.0
X, XX, POS = _capi.AMC_EMOM_X, _capi.AMC_EMOM_XX, _capi.AMC_EMOM_POS


def device_us(eng, call, n):
    eng.sync()
    eng.timing_begin()
    for _ in range(n):
        call()
    return eng.timing_end() * 1e3 / n


def make_engine(M, betas):
    eng = _capi.HipEngine(n_chains=M, potential="double_well", beta=1.0, sigma=[0.5], weight=[1.0], seed=1)
    eng.init_uniform(-1.5, 1.5)
    x = eng.download_state(want_e=False)[0]
    eng.upload_state(x, np.tile(np.asarray(betas, dtype=np.float64), M // R))
    eng.set_ladder(R)
    eng.sweep(300)                                       # ramp: clocks up, every rung near its own distribution
    eng.sync()
    return eng


def blocked_table(args, M, n):
    """The pass per jackknife block beside the plain moments pass, windows alternating."""
    B = args.blocks
    eng = make_engine(M, 0.5 * 1.5 ** np.arange(R))
    plain = lambda mask: (lambda: eng.energy_moments_accumulate(*BINS, mask, X_BOUND))
    blocked = lambda mask: (lambda: eng.energy_moments_accumulate_blocks(*BINS, mask, X_BOUND))
    default = max(1, 256 // R)
    figures = [("ehist", "the plain energy-histogram snapshot", None, lambda: eng.energy_histogram_accumulate(*BINS), None)]
    for key, text, mask in (("x", "mask X", X), ("x_xx", "mask X + XX", X | XX), ("all", "mask X + XX + POS", X | XX | POS)):
        figures.append((key, f"moments, {text}", (0, 0), plain(mask), None))
        figures.append((f"blk_{key}", f"moments per block, {text}, B = {B}, chunk {default}", (B, 0), blocked(mask), key))
    figures.append(("blk_all_1", f"moments per block, mask X + XX + POS, B = {B}, chunk 1", (B, 1), blocked(X | XX | POS), "all"))
    us = {f[0]: [] for f in figures}
    for _ in range(args.repeats):
        for key, _, part, call, _ in figures:
            eng.energy_moments_fetch(reset=True)         # (another mask or form is another accumulator; outside the timed region ...
            if part is not None:
                eng.set_blocks(*part)
            call()                                       #  ... as is the call that allocates and zeroes the new accumulator)
            us[key].append(device_us(eng, call, n))
    med = {k: float(np.median(v)) for k, v in us.items()}
    print(f"M = {M}, R = {R}, double well, K = 1, {BINS[2]} bins of [{BINS[0]:g}, {BINS[1]:g}), x_bound = {X_BOUND:g}; {args.repeats} alternating "
          f"windows of {n} queued calls per figure (median, min .. max)\n")
    print("| figure | us | vs the plain moments pass of the same mask |")
    print("|---|---|---|")
    for key, text, _, _, base in figures:
        ratio = f"{med[key] / med[base]:.2f}" if base else ""
        print(f"| {text} | {med[key]:.1f} ({min(us[key]):.1f} .. {max(us[key]):.1f}) | {ratio} |")
    # what the last window left: the identities of the contract
    counts, sums, n_snap, _ = eng.energy_moments_fetch_blocks()
    per_block = counts.sum(axis=2)[:, 0]
    merged = eng.energy_moments_fetch()
    print(f"\n{n_snap} snapshots in the accumulator; ladders per block {int(per_block.min()) // max(n_snap, 1)} .. {int(per_block.max()) // max(n_snap, 1)}; "
          f"the merged fetch is the sum over the blocks: {bool(np.array_equal(merged[0], counts.sum(axis=0, dtype=np.uint64)) and np.array_equal(merged[1], sums.sum(axis=0)))}; "
          f"beyond x_bound: {int(counts[:, :, -1].sum())}")
    eng.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=0, metavar="B", help="time the pass per jackknife block beside the plain moments pass")
    args = ap.parse_args(argv)
    M, n = args.chains - args.chains % (2 * R), args.launches
    if n + 1 >= 2 ** 31 // (M // R):
        ap.error(f"--launches {n}: a moments accumulator of {M // R} chains per rung holds fewer than {2 ** 31 // (M // R)} snapshots")
    if args.blocks:
        return blocked_table(args, M, n)
    ladder = make_engine(M, 0.5 * 1.5 ** np.arange(R))
    cold = make_engine(M, [0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 64.0, 4000.0])      # the cold rung: e of order 1 / 4000, bin width 0.08
    mom = lambda eng, mask: (lambda: eng.energy_moments_accumulate(*BINS, mask, X_BOUND))
    figures = [("ehist", "the plain energy-histogram snapshot", ladder, lambda: ladder.energy_histogram_accumulate(*BINS)),
               ("x", "moments, mask X", ladder, mom(ladder, X)),
               ("x_xx", "moments, mask X + XX", ladder, mom(ladder, X | XX)),
               ("all", "moments, mask X + XX + POS", ladder, mom(ladder, X | XX | POS)),
               ("cold_ehist", "cold ladder (beta = 4000 at the last rung): the plain snapshot", cold, lambda: cold.energy_histogram_accumulate(*BINS)),
               ("cold_x", "cold ladder: moments, mask X", cold, mom(cold, X)),
               ("cold_x_xx", "cold ladder: moments, mask X + XX", cold, mom(cold, X | XX)),
               ("cold_all", "cold ladder: moments, mask X + XX + POS", cold, mom(cold, X | XX | POS)),
               ("rungs", "amc_reduce_rungs_exact (e, x, x^2 per rung; copies to the host and synchronises)", ladder, lambda: ladder.reduce_rungs())]
    us = {k: [] for k, _, _, _ in figures}
    for _ in range(args.repeats):
        for key, _, eng, call in figures:
            eng.energy_moments_fetch(reset=True)         # (another mask is another form; outside the timed region ...
            call()                                       #  ... as is the call that allocates and zeroes the new accumulator)
            us[key].append(device_us(eng, call, n if key != "rungs" else max(n // 10, 1)))
    med = {k: float(np.median(v)) for k, v in us.items()}
    print(f"M = {M}, R = {R}, double well, K = 1, {BINS[2]} bins of [{BINS[0]:g}, {BINS[1]:g}), x_bound = {X_BOUND:g}; {args.repeats} alternating "
          f"windows of {n} queued calls per figure (median, min .. max)\n")
    print("| figure | us | vs the plain snapshot of the same run |")
    print("|---|---|---|")
    for key, text, _, _ in figures:
        print(f"| {text} | {med[key]:.1f} ({min(us[key]):.1f} .. {max(us[key]):.1f}) | {med[key] / med['ehist']:.2f} |")
    # what the last window of the cold ladder left: the crowding of its coldest row, and the identities of the contract
    counts, sums, n_snap, _ = cold.energy_moments_fetch()
    row = counts[R - 1, :BINS[2]]
    print(f"\ncold rung: {int((row > 0).sum())} non-empty bins, the fullest holds {row.max() / max(row.sum(), 1):.3f} of its chains; {n_snap} snapshots in "
          f"the accumulator; rows sum to snapshots x ladders: {bool(np.all(counts.sum(axis=1) == n_snap * (M // R)))}; beyond x_bound: {int(counts[:, -1].sum())}")
    print(f"cold over spread, all three columns: {med['cold_all'] / med['all']:.2f}")
    for eng in (ladder, cold):
        eng.close()


if __name__ == "__main__":
    main()
