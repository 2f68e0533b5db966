// amc_ehist.h -- energy histograms per group: energy_histogram_kernel<POT>, one pass that bins
// e = potential_T(x) of every local chain into the row of its group (its rung; ONE group without a ladder),
// energy_histogram_blocks_kernel<POT>, the same pass with a set of rows per jackknife block, energy_histogram_families_kernel<POT>, the
// pass with a row per block of an annealed population's families, and the plain kernels that zero the cells
// behind a respacing that was taken and fold the blocks' rows into one set.  Counts are integers: the same on any grid, in any order, on any split.
// Part of the kernel sources of the many-chain Metropolis engine (gfx950 / CDNA4); amc_kernels.h includes all of them, in order.
#pragma once

#include "amc_blocks.h"

namespace amc {

// The per-block histogram is a STATIC LDS array (launch_by_potential and rtc_launch pass no dynamic LDS): 12288 u32 cells = 48 KiB,
// beside the 4.4 KiB of math tables 52.4 KiB per block.  That stays below the 64 KiB a workgroup's static LDS may take without special
// options, and three such blocks fit the 160 KiB of a CU -- the pass runs two per CU (hist_grid: the flush, not the occupancy, sets
// its grid), so LDS never lowers what is resident.  It is amc_histogram_rungs' threshold too: R = 64 rungs of 189 bins fit.  Beyond
// it every chain is one 64-bit global atomic, as in rung_histogram_kernel.  A u32 cell holds a block's share of ONE pass, at most
// ceil(M / gridDim.x) chains: the host refuses a launch whose grid would let that reach 2^32 (amc_energy_histogram_accumulate).
enum { EHIST_LDS_CELLS = 12288 };

struct EhistArgs {
    const real_t* x;              // [n_chains] positions of the local shard
    unsigned long long* counts;   // [n_groups][n_bins + 3] the accumulator
    int64_t n_chains;
    double lo, hi, inv_w;         // inv_w = (double)n_bins / (hi - lo), formed by the host
    int32_t n_groups, n_bins;     // G (the shard starts at a multiple of it); bins
};

// One chain into its cell: e in T as the bridge sums form it, widened exactly, binned by hist_bin.
template <int POT>
__device__ __forceinline__ void ehist_count(const EhistArgs& a, real_t x, const double* s_math, bool lds, unsigned int* s_cells, int base)
{
    const int cell = base + hist_bin((double)potential<POT>(x, s_math), a.lo, a.hi, a.inv_w, a.n_bins);
    if (lds) atomicAdd(&s_cells[cell], 1u);
    else atomicAdd(&a.counts[cell], 1ull);
}

// Memory-bound, one read of x.  Work items as in the sums by group: thread id = l0 G + r, a thread keeps its group -- the base of its
// row is formed once, no modulo per chain -- and advances by (threads / G) ladders per trip, so neighbouring lanes read neighbouring
// chains; four loads in flight per lane (one load per trip leaves the pass waiting for latency: histogram_kernel).  Float32 state
// halves the bytes.  The grid is hist_grid's: the flush ends every block with atomics on the same few addresses.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void energy_histogram_kernel(const EhistArgs a)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned int s_cells[EHIST_LDS_CELLS];
    const int row = a.n_bins + 3, cells = a.n_groups * row;
    const bool lds = cells <= EHIST_LDS_CELLS;
    if (lds)
        for (int i = threadIdx.x; i < cells; i += AMC_BLOCK) s_cells[i] = 0u;
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier: the cells are cleared too)

    const uint32_t tid = blockIdx.x * AMC_BLOCK + threadIdx.x;      // (a grid of hist_grid: far below 2^32 threads)
    const uint32_t ladders_per_trip = (gridDim.x * AMC_BLOCK) / (uint32_t)a.n_groups;
    const uint32_t l0 = tid / (uint32_t)a.n_groups;
    if (l0 < ladders_per_trip) {
        const int base = (int)(tid - l0 * (uint32_t)a.n_groups) * row;
        const int64_t step = (int64_t)ladders_per_trip * a.n_groups;      // chains per trip
        int64_t i = tid;                                                  // chain l0 G + r
        for (; i + 3 * step < a.n_chains; i += 4 * step) {
            const real_t x0 = a.x[i], x1 = a.x[i + step], x2 = a.x[i + 2 * step], x3 = a.x[i + 3 * step];
            ehist_count<POT>(a, x0, s_math, lds, s_cells, base);
            ehist_count<POT>(a, x1, s_math, lds, s_cells, base);
            ehist_count<POT>(a, x2, s_math, lds, s_cells, base);
            ehist_count<POT>(a, x3, s_math, lds, s_cells, base);
        }
        for (; i < a.n_chains; i += step) ehist_count<POT>(a, a.x[i], s_math, lds, s_cells, base);
    }
    if (lds) {
        __syncthreads();
        flush_cells(s_cells, a.counts, cells);
    }
}

// Per jackknife block (amc_energy_histogram_accumulate_blocks): energy_histogram_kernel's body on the traversal of
// bridge_sums_blocks_kernel.  The grid is a multiple of B and HIP block k serves jackknife block b = k mod B alone, over ALL local
// ladders in one launch (a count has no lane cap), so the LDS array stays G rows for ONE jackknife block -- the same cells, the same
// threshold, the same occupancy -- and is flushed into that block's rows, counts + b G (n_bins + 3); beyond the threshold every chain
// is one 64-bit global atomic into its block's row.  A thread keeps its group (blk::walk_begin), so the row base is formed once; four
// loads in flight per lane over the flattened (chunk, trip) sequence.  A u32 cell holds at most blk::lane_bound x AMC_BLOCK chains of
// one pass: the host refuses a launch that could reach 2^32.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void energy_histogram_blocks_kernel(const EhistArgs a, const blk::Part part)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned int s_cells[EHIST_LDS_CELLS];
    const int row = a.n_bins + 3, cells = a.n_groups * row;
    const bool lds = cells <= EHIST_LDS_CELLS;
    if (lds)
        for (int i = threadIdx.x; i < cells; i += AMC_BLOCK) s_cells[i] = 0u;
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier: the cells are cleared too)

    EhistArgs mine = a;                                        // ... with the rows of this HIP block's jackknife block
    mine.counts = a.counts + (int64_t)((int)blockIdx.x % part.n_blocks) * cells;
    blk::Walk w;
    const int g = blk::walk_begin(w, part, a.n_groups, (int)gridDim.x, AMC_BLOCK, (int)blockIdx.x, (int)threadIdx.x, 0, a.n_chains / a.n_groups);
    const int base = g * row;
    for (;;) {
        const int64_t l0 = blk::walk_next(w), l1 = blk::walk_next(w), l2 = blk::walk_next(w), l3 = blk::walk_next(w);
        if (l3 < 0) {                                             // fewer than four are left: one by one
            const int64_t rest[3] = {l0, l1, l2};
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (rest[j] >= 0) ehist_count<POT>(mine, a.x[rest[j] * a.n_groups + g], s_math, lds, s_cells, base);
            break;
        }
        const real_t x0 = a.x[l0 * a.n_groups + g], x1 = a.x[l1 * a.n_groups + g], x2 = a.x[l2 * a.n_groups + g], x3 = a.x[l3 * a.n_groups + g];
        ehist_count<POT>(mine, x0, s_math, lds, s_cells, base);
        ehist_count<POT>(mine, x1, s_math, lds, s_cells, base);
        ehist_count<POT>(mine, x2, s_math, lds, s_cells, base);
        ehist_count<POT>(mine, x3, s_math, lds, s_cells, base);
    }
    if (lds) {
        __syncthreads();
        flush_cells(s_cells, mine.counts, cells);
    }
}

// Per block of FAMILIES (amc_energy_histogram_accumulate_blocks under amc_set_anneal_blocks; DESIGN.md section 3.14 "Error bars"):
// energy_histogram_kernel's pass for the ONE group of an annealed population, chain i counted into the row of the block of its
// ancestor, b = (fam[i] div chunk) mod B -- counts[b][n_bins + 3].  The block is a property of the chain, not of the HIP block, so
// the LDS array holds all B rows: u32 cells flushed as energy_histogram_kernel flushes them while B (n_bins + 3) <= EHIST_LDS_CELLS,
// one 64-bit global atomic per chain beyond.  A u32 cell holds at most a HIP block's share of one pass (the host's check, as for the
// plain pass).  chunk is capped at 2^32 - 1 by the host (anneal_block_sums_kernel).  Integer counts: the sum over the blocks is the
// plain histogram cell for cell.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void energy_histogram_families_kernel(const EhistArgs a, const uint32_t* fam, uint32_t chunk, int n_blocks)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned int s_cells[EHIST_LDS_CELLS];
    const int row = a.n_bins + 3, cells = n_blocks * row;
    const bool lds = cells <= EHIST_LDS_CELLS;
    if (lds)
        for (int i = threadIdx.x; i < cells; i += AMC_BLOCK) s_cells[i] = 0u;
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier: the cells are cleared too)

    const int64_t step = (int64_t)gridDim.x * AMC_BLOCK;
    int64_t i = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    for (; i + 3 * step < a.n_chains; i += 4 * step) {        // four loads of x and of fam in flight per lane
        const real_t x0 = a.x[i], x1 = a.x[i + step], x2 = a.x[i + 2 * step], x3 = a.x[i + 3 * step];
        const uint32_t f0 = fam[i], f1 = fam[i + step], f2 = fam[i + 2 * step], f3 = fam[i + 3 * step];
        ehist_count<POT>(a, x0, s_math, lds, s_cells, (int)((f0 / chunk) % (uint32_t)n_blocks) * row);
        ehist_count<POT>(a, x1, s_math, lds, s_cells, (int)((f1 / chunk) % (uint32_t)n_blocks) * row);
        ehist_count<POT>(a, x2, s_math, lds, s_cells, (int)((f2 / chunk) % (uint32_t)n_blocks) * row);
        ehist_count<POT>(a, x3, s_math, lds, s_cells, (int)((f3 / chunk) % (uint32_t)n_blocks) * row);
    }
    for (; i < a.n_chains; i += step) ehist_count<POT>(a, a.x[i], s_math, lds, s_cells, (int)((fam[i] / chunk) % (uint32_t)n_blocks) * row);
    if (lds) {
        __syncthreads();
        flush_cells(s_cells, a.counts, cells);
    }
}

#if AMC_PLAIN_KERNELS
// amc_set_blocks on a blocked accumulator: the B blocks' rows added into the first, in place (thread i reads cell i of every block and
// writes cell i of block 0 alone) -- what a plain accumulator would hold, integer for integer.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void ehist_fold_kernel(unsigned long long* counts, int cells, int n_blocks)
{
    for (int i = blockIdx.x * AMC_BLOCK + threadIdx.x; i < cells; i += gridDim.x * AMC_BLOCK) {
        unsigned long long s = counts[i];
        for (int b = 1; b < n_blocks; ++b) s += counts[(int64_t)b * cells + i];
        counts[i] = s;
    }
}

// Behind ladder_respace_kernel on the stream: a respacing that was taken zeroes the cells (every block's, of a blocked accumulator), as
// it zeroes the bridge records -- counts taken at other beta belong to another ladder.  Any other status leaves them.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void ehist_respaced_kernel(unsigned long long* counts, int cells, const unsigned long long* rec)
{
    if (rec[RESPACE_STATUS] != 0ull) return;
    for (int i = blockIdx.x * AMC_BLOCK + threadIdx.x; i < cells; i += gridDim.x * AMC_BLOCK) counts[i] = 0ull;
}
#endif

}  // namespace amc
