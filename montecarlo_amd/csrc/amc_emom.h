// amc_emom.h -- moments per energy bin (DESIGN.md section 3.17 "Moments per bin"): energy_moments_kernel<POT>, the pass of
// energy_histogram_kernel that, beside the count of every cell, adds x, x^2 and [x > 0] of the chains of a bin into integer sums per
// (group, column, bin) -- the microcanonical means that multiple-histogram reweighting needs for <x>, <x^2> and the occupancy of a well
// at any beta.  Every summand is an integer multiple of a quantum fixed by x_bound (kind Q of section 3.8), added as a signed 64-bit
// integer: the same on any grid, in any order, on any split.  energy_moments_blocks_kernel<POT> is the same pass with a set of cells
// per jackknife block ("Moments per block").  The cells, the traversals and the plain kernels are amc_ehist.h's.
// Part of the kernel sources of the many-chain Metropolis engine (gfx950 / CDNA4); amc_kernels.h includes all of them, in order.
#pragma once

#include "amc_xsum.h"

namespace amc {

// The columns, in mask-bit order (AMC_EMOM_X, AMC_EMOM_XX, AMC_EMOM_POS of include/amc.h).
enum { EMOM_X = 1, EMOM_XX = 2, EMOM_POS = 4, EMOM_ALL = 7 };

// The quanta of the columns X and XX from the bound: eb = ilogb(x_bound) + 1, so |x| <= x_bound < 2^eb and x^2 < 2^(2 eb);
// E_X = eb - 32, E_XX = 2 eb - 32: a summand is at most 2^32 quanta.  (x_bound normal: the biased exponent field is its ilogb.)
AMC_XS_HD int emom_eb(double x_bound) { return (int)((xs::xs_double_bits(x_bound) >> 52) & 0x7FFu) - 1023 + 1; }
AMC_XS_HD int emom_e_x(double x_bound) { return emom_eb(x_bound) - 32; }
AMC_XS_HD int emom_e_xx(double x_bound) { return 2 * emom_eb(x_bound) - 32; }

// One summand in quanta: k = RN(lsb1(v) 2^-e) for |v| <= 2^(e + 32), by the accumulator add of amc_xsum.h -- t = 1.5 2^(e + 52) + lsb1(v)
// has the ulp 2^e, so the one rounding of that addition is the rounding to the quantum, and the bit patterns of t and of the constant
// differ by k.  lsb1 sets the last bit of v: a value with an odd 53-bit significand and an exponent of at most e + 32 never lies half
// way between two multiples of 2^e, so no tie exists and the rounding mode's tie rule never decides.  The host compiles this too
// (tests/aux/emom_deposit_host.cpp).
AMC_XS_HD int64_t emom_quanta(double v, int e)
{
    const double t = xs::xs_c(e) + xs::xs_lsb1(v);
    return (int64_t)(xs::xs_double_bits(t) - xs::xs_c_bits(e));
}
// The summand of column X for xd = (double)x, and of column XX: v = xd * xd is rounded to Float64 once (exact for Float32 state); the
// bit operation of lsb1 stands between the product and the addition, so nothing can be contracted.
AMC_XS_HD int64_t emom_deposit_x(double xd, int e_x) { return emom_quanta(xd, e_x); }
AMC_XS_HD int64_t emom_deposit_xx(double xd, int e_xx)
{
    const double v = xd * xd;
    return emom_quanta(v, e_xx);
}
// A chain of a bin whose position lies beyond the bound (NaN included) goes into the fourth tail cell and into no sum.
AMC_XS_HD bool emom_x_inside(double xd, double x_bound) { return __builtin_fabs(xd) <= x_bound; }

}  // namespace amc

// (what stands above is plain host + device arithmetic over amc_xsum.h: a host compiler stops here)
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#include "amc_ehist.h"

namespace amc {

struct EmomArgs {
    const real_t* x;              // [n_chains] positions of the local shard
    unsigned long long* counts;   // [n_groups][n_bins + 4] the count cells
    unsigned long long* sums;     // [n_groups][n_cols][n_bins] the sum cells: signed 64-bit integers, added modulo 2^64
    int64_t n_chains;
    double lo, hi, inv_w;         // inv_w = (double)n_bins / (hi - lo), formed by the host
    double x_bound;
    int32_t n_groups, n_bins;
    int32_t mask, n_cols;         // the columns kept; C = popcount(mask)
    int32_t e_x, e_xx;            // the quanta's exponents, formed by the host (emom_e_x, emom_e_xx)
};

// One chain into row r: its cell by ehist_count's rule, the fourth tail cell for a position beyond the bound, and the selected columns
// of its row -- count cells r (n_bins + 4) + cell, sum cells (r C + column) n_bins + cell.
template <int POT>
__device__ __forceinline__ void emom_count(const EmomArgs& a, const BinCells& c, real_t x, const double* s_math, int r)
{
    int cell = hist_bin((double)potential<POT>(x, s_math), a.lo, a.hi, a.inv_w, a.n_bins);
    const double xd = (double)x;
    const bool binned = cell < a.n_bins;
    const bool inside = emom_x_inside(xd, a.x_bound);
    if (binned && !inside) cell = a.n_bins + 3;
    const int count_at = r * (a.n_bins + 4) + cell;
    if (c.lds) atomicAdd(&c.s_counts[count_at], 1u);
    else atomicAdd(&c.counts[count_at], 1ull);
    if (!(binned && inside)) return;
    int at = r * a.n_cols * a.n_bins + cell;
    auto add = [&](unsigned long long k) {
        if (c.lds) atomicAdd(&c.s_sums[at], k);
        else atomicAdd(&c.sums[at], k);
        at += a.n_bins;
    };
    if (a.mask & EMOM_X) add((unsigned long long)emom_deposit_x(xd, a.e_x));
    if (a.mask & EMOM_XX) add((unsigned long long)emom_deposit_xx(xd, a.e_xx));
    if ((a.mask & EMOM_POS) && xd > 0.0) add(1ull);
}

// Per group (amc_energy_moments_accumulate): energy_histogram_kernel's traversal and cells (amc_ehist.h), G C n_bins sum cells in front of
// the G (n_bins + 4) count cells in the same 48 KiB, so the LDS path's threshold is G (n_bins + 4) + 2 C G n_bins words.  A u32 count
// cell holds a block's share of ONE pass, far below 2^31 chains (the host's capacity check).
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void energy_moments_kernel(const EmomArgs a)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_words[EHIST_LDS_CELLS / 2];
    const BinCells c = bin_cells_begin(s_words, s_math, a.counts, a.sums, a.n_groups * (a.n_bins + 4), a.n_groups * a.n_cols * a.n_bins);
    chains_by_group(a.x, a.n_chains, a.n_groups, [&](real_t x, int g) { emom_count<POT>(a, c, x, s_math, g); });
    bin_cells_flush(c);
}

// Per jackknife block (amc_energy_moments_accumulate_blocks): energy_histogram_blocks_kernel's traversal, the cells of ONE jackknife
// block.  The accumulator is B sets of the plain layout, a.counts = set 0: set b begins b (count_cells + sum_cells) words behind it, its
// sums count_cells words further.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void energy_moments_blocks_kernel(const EmomArgs a, const blk::Part part)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_words[EHIST_LDS_CELLS / 2];
    const int count_cells = a.n_groups * (a.n_bins + 4), sum_cells = a.n_groups * a.n_cols * a.n_bins;
    unsigned long long* set = a.counts + (int64_t)((int)blockIdx.x % part.n_blocks) * ((int64_t)count_cells + sum_cells);
    const BinCells c = bin_cells_begin(s_words, s_math, set, set + count_cells, count_cells, sum_cells);
    chains_by_block(a.x, a.n_chains, a.n_groups, part, [&](real_t x, int g) { emom_count<POT>(a, c, x, s_math, g); });
    bin_cells_flush(c);
}

}  // namespace amc
#endif
