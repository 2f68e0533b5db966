// xsum_lanes_host.cpp -- the kind-R lane arithmetic of the kernels (montecarlo_amd/csrc/amc_xsum.h, "kind R in a lane") run on the host.
//
//   xsum_lanes_host <file of raw Float64s> <L> [<blocks>]
// The values are cut into <blocks> contiguous pieces (default 1); a piece is one "block" of L lanes.  Summand i of a block goes to
// lane i mod L, which runs the per-lane sequence of rl_deposit (amc_wave_sums.h): the special-flag check, xs_r_rebase when its top
// cannot take the value, xs_r_split, ++n.  Then the block end of the sums by group (group_rows_end, amc_exchange.h): the maximum of the
// lanes' tops and the OR of their flags, every lane's xs_r_multiples brought to that top by xs_r_settle, integer addition,
// rec_from_r.  Prints the XS_WORDS words of each block's record on one line.
// Build: c++ -O2 -std=c++17 -ffp-contract=off (tests/test_xsum.py); the header is plain host C++ once the two qualifiers are empty.
#define __host__
#define __device__
#include "amc_xsum.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace amc::xs;

struct Lane {
    uint64_t a1 = 0, a2 = 0;
    int top = XS_LMIN;
    uint32_t flags = 0;
    int n = 0;
};

static void lane_deposit(Lane& L, double v)
{
    if (!(std::fabs(v) < xs_level_cap(L.top))) {
        const int need = xs_level_of(v);                   // > LMAX: no level takes it, a flag carries it
        if (need > XS_LMAX) {
            L.flags |= xs_r_flag_beyond(xs_double_bits(v));
            v = 0.0;
        } else {
            xs_r_rebase(L.a1, L.a2, (uint64_t)L.n, L.top, need);
        }
    }
    uint64_t t, t2;
    xs_r_split(v, xs_bits_double(xs_level_c_bits(L.top)), xs_bits_double(xs_level_c_bits(L.top - 1)), t, t2);
    L.a1 += t;
    L.a2 += t2;
    L.n += 1;
}

static void block_record(const double* v, size_t count, int n_lanes, double* rec)
{
    std::vector<Lane> lanes((size_t)n_lanes);
    for (size_t i = 0; i < count; ++i) lane_deposit(lanes[i % (size_t)n_lanes], v[i]);
    PartR p = part_r_empty();
    for (const Lane& L : lanes) {
        if (L.n == 0) continue;                            // (the kernel's `mine`)
        p.top = L.top > p.top ? L.top : p.top;
        p.flags |= L.flags;
    }
    for (const Lane& L : lanes) {
        if (L.n == 0) continue;
        RPair k = xs_r_multiples(L.a1, L.a2, (uint64_t)L.n, L.top);
        xs_r_settle(p.top - L.top, k.k1, k.k2);
        p.k1 = i128_add(p.k1, i128_of(k.k1));
        p.k2 = i128_add(p.k2, i128_of(k.k2));
    }
    rec_from_r(rec, p);
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const int n_lanes = std::atoi(argv[2]), n_blocks = argc > 3 ? std::atoi(argv[3]) : 1;
    if (n_lanes < 1 || n_blocks < 1) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> v;
    double buf[256];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) v.insert(v.end(), buf, buf + got);
    std::fclose(f);
    for (int b = 0; b < n_blocks; ++b) {
        const size_t lo = v.size() * (size_t)b / (size_t)n_blocks, hi = v.size() * (size_t)(b + 1) / (size_t)n_blocks;
        double rec[XS_WORDS];
        block_record(v.data() + lo, hi - lo, n_lanes, rec);
        for (int i = 0; i < XS_WORDS; ++i) std::printf("%.17g%c", rec[i], i + 1 < XS_WORDS ? ' ' : '\n');
    }
    return 0;
}
