"""The slice plan of the single-sweep launches (montecarlo_amd/csrc/amc_slices.h): pure host arithmetic, checked in a small C++
program of its own built with AddressSanitizer and UBSan.  No GPU.

For every pair count, slice count and grid shape: the slices tile the range exactly, boundaries are multiples of 256 pairs, only the
last slice is ragged (or ends in a lone chain), no slice is empty, full_rounds * grid * 256 + tail_pairs is the slice's pair count,
and every grid fits the shared counter slots."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "amc_slices.h"
#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            std::printf("FAILED %s: chains=%lld S=%d cu=%d bpc=%d slots=%d slice=%d\n", #cond, (long long)n_chains, S, cu, bpc, slots, i); \
            return 1;                                                                                                        \
        }                                                                                                                    \
    } while (0)

int main()
{
    const int B = 256;
    const long long pair_counts[] = {0, 1, 255, 256, 257, 3 * 256, 3 * 256 + 1, 5000000, (1ll << 31) + 17};
    const int grids[][3] = {{256, 2, 2560}, {256, 3, 2560}, {256, 4, 2560}, {256, 6, 2560}, {256, 64, 2560}, {1, 1, 10}, {304, 6, 3040}, {7, 3, 5}};
    long cases = 0;
    for (long long pairs : pair_counts)
        for (int odd = 0; odd < 2; ++odd) {
            const long long n_chains = 2 * pairs - odd;      // the last pair whole, or a lone chain
            if (n_chains < 0) continue;
            for (int S = 1; S <= 3; ++S)
                for (const auto& g : grids) {
                    const int cu = g[0], bpc = g[1], slots = g[2];
                    int i = -1;
                    const amc::SlicePlan p = amc::plan_slices(n_chains, B, S, cu, bpc, slots);
                    const long long n_pairs = (n_chains + 1) / 2, n_blocks = (n_pairs + B - 1) / B;
                    CHECK(p.count == (n_blocks < S ? n_blocks : S));
                    long long next_pair = 0, chains = 0;
                    for (i = 0; i < p.count; ++i) {
                        const amc::Slice& s = p.s[i];
                        const long long sp = (s.n_chains + 1) / 2;
                        CHECK(s.first_pair == next_pair);                         // tiles the range, in order
                        CHECK(s.first_pair % B == 0);                             // boundaries on whole blocks
                        CHECK(s.n_chains > 0);                                    // no empty slice
                        if (i + 1 < p.count) CHECK(sp % B == 0 && s.n_chains == 2 * sp);      // only the last is ragged or odd
                        CHECK(s.grid >= 1 && s.grid <= slots);
                        CHECK((long long)s.grid <= (long long)cu * bpc);
                        CHECK((long long)s.grid <= (sp + B - 1) / B);             // no block without a trip of its own
                        CHECK(s.full_rounds >= 0 && s.tail_pairs >= 0 && s.tail_pairs < (long long)s.grid * B);
                        CHECK((long long)s.full_rounds * s.grid * B + s.tail_pairs == sp);
                        next_pair += sp;
                        chains += s.n_chains;
                    }
                    i = -1;
                    CHECK(next_pair == n_pairs && chains == n_chains);
                    if (p.count > 1) {                                            // whole blocks dealt out evenly
                        const long long b0 = (p.s[0].n_chains / 2 + B - 1) / B, bl = ((p.s[p.count - 1].n_chains + 1) / 2 + B - 1) / B;
                        CHECK(b0 - bl >= 0 && b0 - bl <= 1);
                    }
                    ++cases;
                }
        }
    std::printf("ok %ld\n", cases);
    return 0;
}
"""


def test_slice_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "slice_plan_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "slice_plan_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "montecarlo_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) == 9 * 2 * 3 * 8 - 3 * 8      # every case ran (0 pairs has no odd form)
