// amc_ehist.h -- energy histograms per group.  What every pass over the energy bins is made of -- the block's cells
// in LDS (BinCells: set up, flushed), the three traversals of the chains (by group, by jackknife block, by family) over a callable, the
// deposit rule of the counts (ehist_count) -- and the three passes themselves: energy_histogram_kernel<POT> bins e = potential_T(x) of
// every local chain into the row of its group (its rung; ONE group without a ladder), energy_histogram_blocks_kernel<POT> keeps a set
// of rows per jackknife block, energy_histogram_families_kernel<POT> a row per block of an annealed population's families.  The moments
// per bin (amc_emom.h) are the same cells and traversals under another deposit rule.  Then the plain kernels that zero an
// accumulator's words behind a respacing that was taken and fold the blocks' sets into one, for both accumulators.  Counts are
// integers: the same on any grid, in any order, on any split.
// Part of the kernel sources of the many-chain Metropolis engine (gfx950 / CDNA4); amc_kernels.h includes all of them, in order.
#pragma once

#include "amc_blocks.h"

namespace amc {

// The per-block cells are a STATIC LDS array (launch_by_potential and rtc_launch pass no dynamic LDS): 12288 u32 words = 48 KiB,
// beside the 4.4 KiB of math tables 52.4 KiB per block.  That stays below the 64 KiB a workgroup's static LDS may take without special
// options, and three such blocks fit the 160 KiB of a CU -- the pass runs two per CU (hist_grid: the flush, not the occupancy, sets
// its grid), so LDS never lowers what is resident.  It is amc_histogram_rungs' threshold too: R = 64 rungs of 189 bins fit.  Beyond
// it every deposit is one 64-bit global atomic, as in rung_histogram_kernel.  A u32 cell holds a block's share of ONE pass, at most
// ceil(M / gridDim.x) chains: the host refuses a launch whose grid would let that reach 2^32 (amc_energy_histogram_accumulate).
enum { EHIST_LDS_CELLS = 12288 };

// The cells one HIP block deposits into.  In LDS (declared as 64-bit words, so that the sum cells are 8-byte aligned): first the 64-bit
// sum cells, n_sums of them (none for the histograms), then the u32 count cells, n_counts -- together n_counts + 2 n_sums u32 words,
// the LDS path's threshold; beyond it (lds == false) every deposit is a 64-bit global atomic.  counts / sums: the global cells the block
// serves, the set of its jackknife block in a blocked pass.
struct BinCells {
    unsigned long long* counts;
    unsigned long long* sums;
    unsigned int* s_counts;
    unsigned long long* s_sums;
    int n_counts, n_sums;
    bool lds;
};

// The start of every pass: the threshold decided, the block's cells cleared, the math tables staged behind them.
__device__ __forceinline__ BinCells bin_cells_begin(unsigned long long* s_words, double* s_math, unsigned long long* counts, unsigned long long* sums,
                                                    int n_counts, int n_sums)
{
    BinCells c;
    c.counts = counts;
    c.sums = sums;
    c.n_counts = n_counts;
    c.n_sums = n_sums;
    c.lds = (int64_t)n_counts + 2 * (int64_t)n_sums <= EHIST_LDS_CELLS;
    c.s_sums = s_words;
    c.s_counts = reinterpret_cast<unsigned int*>(s_words + (c.lds ? n_sums : 0));
    if (c.lds) {
        for (int i = threadIdx.x; i < n_sums; i += AMC_BLOCK) c.s_sums[i] = 0ull;
        for (int i = threadIdx.x; i < n_counts; i += AMC_BLOCK) c.s_counts[i] = 0u;
    }
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier: the cells are cleared too)
    return c;
}

// The end of every pass: every non-zero cell of the block goes to the global accumulator with one 64-bit atomic.  A u32 count cell
// holds a block's share of ONE pass (the host's checks); a 64-bit sum cell at most as many summands of at most 2^32 quanta each.
__device__ __forceinline__ void bin_cells_flush(const BinCells& c)
{
    if (!c.lds) return;
    __syncthreads();
    flush_cells(c.s_counts, c.counts, c.n_counts);
    for (int i = threadIdx.x; i < c.n_sums; i += AMC_BLOCK)
        if (c.s_sums[i]) atomicAdd(&c.sums[i], c.s_sums[i]);
}

// The three traversals.  Each hands deposit(x, r) the position of a chain and the row it goes into: its group, or the block of its
// family.  Memory-bound, one read of x; four loads in flight per lane, all issued before the first deposit (one load per trip leaves
// the pass waiting for latency: histogram_kernel), the tail one chain at a time.  Float32 state halves the bytes.
//
// By group: work items as in the sums by group, thread id = l0 G + r.  A thread keeps its group -- whatever the deposit forms from r
// is formed once, no modulo per chain -- and advances by (threads / G) ladders per trip, so neighbouring lanes read neighbouring
// chains.  The grid is hist_grid's: the flush ends every block with atomics on the same few addresses.
template <class Deposit>
__device__ __forceinline__ void chains_by_group(const real_t* x, int64_t n_chains, int n_groups, Deposit&& deposit)
{
    const uint32_t tid = blockIdx.x * AMC_BLOCK + threadIdx.x;      // (a grid of hist_grid: far below 2^32 threads)
    const uint32_t ladders_per_trip = (gridDim.x * AMC_BLOCK) / (uint32_t)n_groups;
    const uint32_t l0 = tid / (uint32_t)n_groups;
    if (l0 >= ladders_per_trip) return;
    const int g = (int)(tid - l0 * (uint32_t)n_groups);
    const int64_t step = (int64_t)ladders_per_trip * n_groups;        // chains per trip
    int64_t i = tid;                                                  // chain l0 G + r
    for (; i + 3 * step < n_chains; i += 4 * step) {
        const real_t x0 = x[i], x1 = x[i + step], x2 = x[i + 2 * step], x3 = x[i + 3 * step];
        deposit(x0, g);
        deposit(x1, g);
        deposit(x2, g);
        deposit(x3, g);
    }
    for (; i < n_chains; i += step) deposit(x[i], g);
}

// By jackknife block: the traversal of bridge_sums_blocks_kernel.  The grid is a multiple of B and HIP block k serves jackknife block
// b = k mod B alone, over ALL local ladders in one launch (a count has no lane cap), so the block's cells stay those of ONE jackknife
// block -- the same cells, the same threshold, the same occupancy.  A thread keeps its group (blk::walk_begin); four loads in flight per
// lane over the flattened (chunk, trip) sequence.  A u32 cell holds at most blk::lane_bound x AMC_BLOCK chains of one pass: the host
// refuses a launch that could reach 2^32.
template <class Deposit>
__device__ __forceinline__ void chains_by_block(const real_t* x, int64_t n_chains, int n_groups, const blk::Part& part, Deposit&& deposit)
{
    blk::Walk w;
    const int g = blk::walk_begin(w, part, n_groups, (int)gridDim.x, AMC_BLOCK, (int)blockIdx.x, (int)threadIdx.x, 0, n_chains / n_groups);
    for (;;) {
        const int64_t l0 = blk::walk_next(w), l1 = blk::walk_next(w), l2 = blk::walk_next(w), l3 = blk::walk_next(w);
        if (l3 < 0) {                                             // fewer than four are left: one by one
            const int64_t rest[3] = {l0, l1, l2};
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (rest[j] >= 0) deposit(x[rest[j] * n_groups + g], g);
            break;
        }
        const real_t x0 = x[l0 * n_groups + g], x1 = x[l1 * n_groups + g], x2 = x[l2 * n_groups + g], x3 = x[l3 * n_groups + g];
        deposit(x0, g);
        deposit(x1, g);
        deposit(x2, g);
        deposit(x3, g);
    }
}

// By family, for the ONE group of an annealed population: flat over the chains, chain i into the row of the block of its ancestor,
// b = (fam[i] div chunk) mod B.  The block is a property of the chain, not of the HIP block.  chunk is capped at 2^32 - 1 by the host
// (anneal_block_sums_kernel).
template <class Deposit>
__device__ __forceinline__ void chains_by_family(const real_t* x, const uint32_t* fam, int64_t n_chains, uint32_t chunk, int n_blocks, Deposit&& deposit)
{
    auto row = [&](uint32_t f) { return (int)((f / chunk) % (uint32_t)n_blocks); };
    const int64_t step = (int64_t)gridDim.x * AMC_BLOCK;
    int64_t i = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    for (; i + 3 * step < n_chains; i += 4 * step) {          // four loads of x and of fam in flight per lane
        const real_t x0 = x[i], x1 = x[i + step], x2 = x[i + 2 * step], x3 = x[i + 3 * step];
        const uint32_t f0 = fam[i], f1 = fam[i + step], f2 = fam[i + 2 * step], f3 = fam[i + 3 * step];
        deposit(x0, row(f0));
        deposit(x1, row(f1));
        deposit(x2, row(f2));
        deposit(x3, row(f3));
    }
    for (; i < n_chains; i += step) deposit(x[i], row(fam[i]));
}

struct EhistArgs {
    const real_t* x;              // [n_chains] positions of the local shard
    unsigned long long* counts;   // [n_groups][n_bins + 3] the accumulator
    int64_t n_chains;
    double lo, hi, inv_w;         // inv_w = (double)n_bins / (hi - lo), formed by the host
    int32_t n_groups, n_bins;     // G (the shard starts at a multiple of it); bins
};

// One chain into its cell of row r: e in T as the bridge sums form it, widened exactly, binned by hist_bin.
template <int POT>
__device__ __forceinline__ void ehist_count(const EhistArgs& a, const BinCells& c, real_t x, const double* s_math, int r)
{
    const int cell = r * (a.n_bins + 3) + hist_bin((double)potential<POT>(x, s_math), a.lo, a.hi, a.inv_w, a.n_bins);
    if (c.lds) atomicAdd(&c.s_counts[cell], 1u);
    else atomicAdd(&c.counts[cell], 1ull);
}

// Per group (amc_energy_histogram_accumulate): counts[G][n_bins + 3].
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void energy_histogram_kernel(const EhistArgs a)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_words[EHIST_LDS_CELLS / 2];
    const BinCells c = bin_cells_begin(s_words, s_math, a.counts, nullptr, a.n_groups * (a.n_bins + 3), 0);
    chains_by_group(a.x, a.n_chains, a.n_groups, [&](real_t x, int g) { ehist_count<POT>(a, c, x, s_math, g); });
    bin_cells_flush(c);
}

// Per jackknife block (amc_energy_histogram_accumulate_blocks): the G rows of this HIP block's jackknife block b, counts + b G (n_bins + 3).
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void energy_histogram_blocks_kernel(const EhistArgs a, const blk::Part part)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_words[EHIST_LDS_CELLS / 2];
    const int cells = a.n_groups * (a.n_bins + 3);
    const BinCells c = bin_cells_begin(s_words, s_math, a.counts + (int64_t)((int)blockIdx.x % part.n_blocks) * cells, nullptr, cells, 0);
    chains_by_block(a.x, a.n_chains, a.n_groups, part, [&](real_t x, int g) { ehist_count<POT>(a, c, x, s_math, g); });
    bin_cells_flush(c);
}

// Per block of FAMILIES (amc_energy_histogram_accumulate_blocks under amc_set_anneal_blocks; DESIGN.md section 3.14 "Error bars"):
// counts[B][n_bins + 3], so the block's cells hold all B rows.  Integer counts: the sum over the blocks is the plain histogram cell for
// cell.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void energy_histogram_families_kernel(const EhistArgs a, const uint32_t* fam, uint32_t chunk, int n_blocks)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_words[EHIST_LDS_CELLS / 2];
    const BinCells c = bin_cells_begin(s_words, s_math, a.counts, nullptr, n_blocks * (a.n_bins + 3), 0);
    chains_by_family(a.x, fam, a.n_chains, chunk, n_blocks, [&](real_t x, int b) { ehist_count<POT>(a, c, x, s_math, b); });
    bin_cells_flush(c);
}

#if AMC_PLAIN_KERNELS
// amc_set_blocks on a blocked accumulator of either kind: the B blocks' sets added into the first, in place (thread i reads word i of
// every set and writes word i of set 0 alone) -- what a plain accumulator would hold, integer for integer (signed sums as unsigned words
// modulo 2^64: exact).
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void ehist_fold_kernel(unsigned long long* counts, int cells, int n_blocks)
{
    for (int i = blockIdx.x * AMC_BLOCK + threadIdx.x; i < cells; i += gridDim.x * AMC_BLOCK) {
        unsigned long long s = counts[i];
        for (int b = 1; b < n_blocks; ++b) s += counts[(int64_t)b * cells + i];
        counts[i] = s;
    }
}

// Behind ladder_respace_kernel on the stream: a respacing that was taken zeroes the words of an accumulator of either kind (every
// block's set, of a blocked one), as it zeroes the bridge records -- counts and sums taken at other beta belong to another ladder.  Any
// other status leaves them.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void ehist_respaced_kernel(unsigned long long* words, int n, const unsigned long long* rec)
{
    if (rec[RESPACE_STATUS] != 0ull) return;
    for (int i = blockIdx.x * AMC_BLOCK + threadIdx.x; i < n; i += gridDim.x * AMC_BLOCK) words[i] = 0ull;
}
#endif

}  // namespace amc
