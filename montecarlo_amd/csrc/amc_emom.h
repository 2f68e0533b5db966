// amc_emom.h -- moments per energy bin (DESIGN.md section 3.17 "Moments per bin"): energy_moments_kernel<POT>, the pass of
// energy_histogram_kernel that, beside the count of every cell, adds x, x^2 and [x > 0] of the chains of a bin into integer sums per
// (group, column, bin) -- the microcanonical means that multiple-histogram reweighting needs for <x>, <x^2> and the occupancy of a well
// at any beta.  Every summand is an integer multiple of a quantum fixed by x_bound (kind Q of section 3.8), added as a signed 64-bit
// integer: the same on any grid, in any order, on any split.  energy_moments_blocks_kernel<POT> is the same pass with a set of cells
// per jackknife block ("Moments per block").  The plain kernel zeroes the cells behind a respacing that was taken.
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

// One chain: its cell by ehist_count's rule, the fourth tail cell for a position beyond the bound, and the selected columns of its
// row.  count_base = g (n_bins + 4), sum_base = g C n_bins.  lds: u32 count cells and 64-bit sum cells of the block; otherwise every
// deposit is a 64-bit global atomic.
template <int POT>
__device__ __forceinline__ void emom_count(const EmomArgs& a, real_t x, const double* s_math, bool lds, unsigned int* s_counts,
                                           unsigned long long* s_sums, int count_base, int sum_base)
{
    int cell = hist_bin((double)potential<POT>(x, s_math), a.lo, a.hi, a.inv_w, a.n_bins);
    const double xd = (double)x;
    const bool binned = cell < a.n_bins;
    const bool inside = emom_x_inside(xd, a.x_bound);
    if (binned && !inside) cell = a.n_bins + 3;
    if (lds) atomicAdd(&s_counts[count_base + cell], 1u);
    else atomicAdd(&a.counts[count_base + cell], 1ull);
    if (!(binned && inside)) return;
    int at = sum_base + cell;
    auto add = [&](unsigned long long k) {
        if (lds) atomicAdd(&s_sums[at], k);
        else atomicAdd(&a.sums[at], k);
        at += a.n_bins;
    };
    if (a.mask & EMOM_X) add((unsigned long long)emom_deposit_x(xd, a.e_x));
    if (a.mask & EMOM_XX) add((unsigned long long)emom_deposit_xx(xd, a.e_xx));
    if ((a.mask & EMOM_POS) && xd > 0.0) add(1ull);
}

// energy_histogram_kernel's traversal: thread id = l0 G + r, a thread keeps its group, four loads in flight per lane, hist_grid's
// grid.  The block's cells live in the SAME 48 KiB of static LDS as the plain pass's (EHIST_LDS_CELLS u32 words, declared as 64-bit
// words so that the sum cells are 8-byte aligned): first the 64-bit sum cells, G C n_bins of them, then the u32 count cells,
// G (n_bins + 4) -- together G (n_bins + 4) + 2 C G n_bins words, the LDS path's threshold; beyond it every deposit is a 64-bit global
// atomic.  At the end of the block every non-zero cell goes to the global accumulator with one 64-bit atomic.  A u32 count cell holds a
// block's share of ONE pass, far below 2^31 chains (the host's capacity check); a 64-bit sum cell at most as many summands of at
// most 2^32 quanta each.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void energy_moments_kernel(const EmomArgs a)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_words[EHIST_LDS_CELLS / 2];
    const int row = a.n_bins + 4, count_cells = a.n_groups * row, sum_cells = a.n_groups * a.n_cols * a.n_bins;
    const bool lds = (int64_t)count_cells + 2 * (int64_t)sum_cells <= EHIST_LDS_CELLS;
    unsigned long long* s_sums = s_words;
    unsigned int* s_counts = reinterpret_cast<unsigned int*>(s_words + (lds ? sum_cells : 0));
    if (lds) {
        for (int i = threadIdx.x; i < sum_cells; i += AMC_BLOCK) s_sums[i] = 0ull;
        for (int i = threadIdx.x; i < count_cells; i += AMC_BLOCK) s_counts[i] = 0u;
    }
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier: the cells are cleared too)

    const uint32_t tid = blockIdx.x * AMC_BLOCK + threadIdx.x;      // (a grid of hist_grid: far below 2^32 threads)
    const uint32_t ladders_per_trip = (gridDim.x * AMC_BLOCK) / (uint32_t)a.n_groups;
    const uint32_t l0 = tid / (uint32_t)a.n_groups;
    if (l0 < ladders_per_trip) {
        const int g = (int)(tid - l0 * (uint32_t)a.n_groups);
        const int count_base = g * row, sum_base = g * a.n_cols * a.n_bins;
        const int64_t step = (int64_t)ladders_per_trip * a.n_groups;      // chains per trip
        int64_t i = tid;                                                  // chain l0 G + r
        for (; i + 3 * step < a.n_chains; i += 4 * step) {
            const real_t x0 = a.x[i], x1 = a.x[i + step], x2 = a.x[i + 2 * step], x3 = a.x[i + 3 * step];
            emom_count<POT>(a, x0, s_math, lds, s_counts, s_sums, count_base, sum_base);
            emom_count<POT>(a, x1, s_math, lds, s_counts, s_sums, count_base, sum_base);
            emom_count<POT>(a, x2, s_math, lds, s_counts, s_sums, count_base, sum_base);
            emom_count<POT>(a, x3, s_math, lds, s_counts, s_sums, count_base, sum_base);
        }
        for (; i < a.n_chains; i += step) emom_count<POT>(a, a.x[i], s_math, lds, s_counts, s_sums, count_base, sum_base);
    }
    if (lds) {
        __syncthreads();
        flush_cells(s_counts, a.counts, count_cells);
        for (int i = threadIdx.x; i < sum_cells; i += AMC_BLOCK)
            if (s_sums[i]) atomicAdd(&a.sums[i], s_sums[i]);
    }
}

// Per jackknife block (amc_energy_moments_accumulate_blocks): energy_moments_kernel's body on the traversal of
// energy_histogram_blocks_kernel.  The grid is a multiple of B and HIP block k serves jackknife block b = k mod B alone, over ALL local
// ladders in one launch, so the LDS array stays the cells of ONE jackknife block -- the same words, the same threshold, the same
// occupancy -- and is flushed into that block's set; beyond the threshold every deposit is a 64-bit global atomic into the block's
// set.  The accumulator is B sets of the plain layout, a.counts = set 0: set b begins b (count_cells + sum_cells) words behind it, its
// sums count_cells words further.  A thread keeps its group (blk::walk_begin), so both bases are formed once; four loads in flight per
// lane over the flattened (chunk, trip) sequence.  A u32 count cell holds at most blk::lane_bound x AMC_BLOCK chains of one pass: the
// host refuses a launch that could reach 2^32.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void energy_moments_blocks_kernel(const EmomArgs a, const blk::Part part)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_words[EHIST_LDS_CELLS / 2];
    const int row = a.n_bins + 4, count_cells = a.n_groups * row, sum_cells = a.n_groups * a.n_cols * a.n_bins;
    const bool lds = (int64_t)count_cells + 2 * (int64_t)sum_cells <= EHIST_LDS_CELLS;
    unsigned long long* s_sums = s_words;
    unsigned int* s_counts = reinterpret_cast<unsigned int*>(s_words + (lds ? sum_cells : 0));
    if (lds) {
        for (int i = threadIdx.x; i < sum_cells; i += AMC_BLOCK) s_sums[i] = 0ull;
        for (int i = threadIdx.x; i < count_cells; i += AMC_BLOCK) s_counts[i] = 0u;
    }
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier: the cells are cleared too)

    EmomArgs mine = a;                                         // ... with the set of this HIP block's jackknife block
    mine.counts = a.counts + (int64_t)((int)blockIdx.x % part.n_blocks) * ((int64_t)count_cells + sum_cells);
    mine.sums = mine.counts + count_cells;
    blk::Walk w;
    const int g = blk::walk_begin(w, part, a.n_groups, (int)gridDim.x, AMC_BLOCK, (int)blockIdx.x, (int)threadIdx.x, 0, a.n_chains / a.n_groups);
    const int count_base = g * row, sum_base = g * a.n_cols * a.n_bins;
    for (;;) {
        const int64_t l0 = blk::walk_next(w), l1 = blk::walk_next(w), l2 = blk::walk_next(w), l3 = blk::walk_next(w);
        if (l3 < 0) {                                             // fewer than four are left: one by one
            const int64_t rest[3] = {l0, l1, l2};
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (rest[j] >= 0) emom_count<POT>(mine, a.x[rest[j] * a.n_groups + g], s_math, lds, s_counts, s_sums, count_base, sum_base);
            break;
        }
        const real_t x0 = a.x[l0 * a.n_groups + g], x1 = a.x[l1 * a.n_groups + g], x2 = a.x[l2 * a.n_groups + g], x3 = a.x[l3 * a.n_groups + g];
        emom_count<POT>(mine, x0, s_math, lds, s_counts, s_sums, count_base, sum_base);
        emom_count<POT>(mine, x1, s_math, lds, s_counts, s_sums, count_base, sum_base);
        emom_count<POT>(mine, x2, s_math, lds, s_counts, s_sums, count_base, sum_base);
        emom_count<POT>(mine, x3, s_math, lds, s_counts, s_sums, count_base, sum_base);
    }
    if (lds) {
        __syncthreads();
        flush_cells(s_counts, mine.counts, count_cells);
        for (int i = threadIdx.x; i < sum_cells; i += AMC_BLOCK)
            if (s_sums[i]) atomicAdd(&mine.sums[i], s_sums[i]);
    }
}

#if AMC_PLAIN_KERNELS
// Behind ladder_respace_kernel on the stream, beside ehist_respaced_kernel: a respacing that was taken zeroes the count cells and the sum
// cells (one allocation, `words` 64-bit words; every block's set, of a blocked accumulator) -- sums taken at other beta belong to another
// ladder.  Any other status leaves them.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void emom_respaced_kernel(unsigned long long* words_ptr, int words, const unsigned long long* rec)
{
    if (rec[RESPACE_STATUS] != 0ull) return;
    for (int i = blockIdx.x * AMC_BLOCK + threadIdx.x; i < words; i += gridDim.x * AMC_BLOCK) words_ptr[i] = 0ull;
}
#endif

}  // namespace amc
#endif
