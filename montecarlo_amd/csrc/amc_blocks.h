// amc_blocks.h -- the bridge sums and the time correlation kept per jackknife block of ladders (amc_set_blocks):
// the partition's index arithmetic -- which launch, HIP block, thread and trip visits which local ladder -- as host-and-device inline
// functions, then bridge_sums_blocks_kernel / corr_sums_blocks_kernel, in which every HIP block serves ONE jackknife block.  Prologue
// and block end are the frame's (amc_exchange.h "the frame of the sums by group"); bridge_finish_kernel and corr_finish_kernel merge the
// rows of the HIP blocks of each jackknife block.
// Part of the kernel sources of the many-chain Metropolis engine (gfx950 / CDNA4); amc_kernels.h includes all of them, in order.
// With AMC_BLOCKS_INDEX_ONLY defined the file is its index arithmetic alone, plain host C++ once __host__ and __device__ are empty: the
// same text then runs on the CPU under the sanitizers (tests/aux/blocks_plan_host.cpp).
#pragma once

#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#define AMC_BLK_HD __host__ __device__ inline

namespace amc {
namespace blk {

enum { BLK_MAX_BLOCKS = 64 };

// The partition (B, C) and where the shard lies in it.  The block of a ladder is b(l) = (l_global div C) mod B with
// l_global = l_first + l_local: a function of the global ladder index and of nothing else.
struct Part {
    int64_t l_first;              // l_global of local ladder 0: chain_offset / G
    int64_t chunk;                // C >= 1: consecutive ladders that share a block
    int32_t n_blocks;             // 2 <= B <= BLK_MAX_BLOCKS
    int32_t pad_;
};

AMC_BLK_HD int block_of(const Part& p, int64_t l_local) { return (int)(((p.l_first + l_local) / p.chunk) % p.n_blocks); }

// Local ladders [0, n_ladders) that lie in block b, in closed form: whole periods of B C ladders hold C each, the two cut periods at the
// ends what below() counts.
AMC_BLK_HD int64_t ladders_below(const Part& p, int b, int64_t g)      // global ladders of block b in [0, g)
{
    const int64_t period = p.chunk * p.n_blocks, whole = g / period, rest = g - whole * period, from = (int64_t)b * p.chunk;
    const int64_t cut = rest <= from ? 0 : (rest - from < p.chunk ? rest - from : p.chunk);
    return whole * p.chunk + cut;
}
AMC_BLK_HD int64_t ladders_in_block(const Part& p, int b, int64_t n_ladders)
{
    return ladders_below(p, b, p.l_first + n_ladders) - ladders_below(p, b, p.l_first);
}

// A launch covers the local ladders [l_begin, l_end) with a grid that is a multiple of B: HIP block k serves b = k mod B with rank
// k div B among the grid / B HIP blocks of that b, and walks the global chunks q = b (mod B) that meet the launch's range, every
// (grid / B)-th of them.  Inside a chunk the threads t < (threads div G) G take group g = t mod G and ladder-in-chunk t div G and
// advance by threads div G ladders per trip: a thread keeps its group, neighbouring lanes read neighbouring chains.  A chunk the
// shard or the launch cuts is walked from its first ladder inside the range.
struct Walk {
    int64_t q, q_stop, q_step;    // the global chunk at hand; one past the last chunk of the launch; (grid / B) B
    int64_t l, hi;                // the next local ladder of this lane in the chunk; one past the chunk's last local ladder
    int64_t g_begin, g_end;       // the launch's range as global ladders
    int64_t l_first, chunk;
    int32_t per_trip, li;         // threads div G; this lane's ladder-in-chunk
};

AMC_BLK_HD void walk_enter(Walk& w)
{
    if (w.q >= w.q_stop) { w.l = w.hi = 0; return; }
    const int64_t a = w.q * w.chunk, z = a + w.chunk;
    const int64_t lo = a > w.g_begin ? a : w.g_begin, up = z < w.g_end ? z : w.g_end;
    w.l = lo - w.l_first + w.li;
    w.hi = up - w.l_first;
}

// Thread t of HIP block k begins its walk; returns its group g.  A thread beyond (threads div G) G has nothing to walk.
AMC_BLK_HD int walk_begin(Walk& w, const Part& p, int n_groups, int grid, int threads, int k, int t, int64_t l_begin, int64_t l_end)
{
    const int B = p.n_blocks, b = k % B, rank = k / B, per_b = grid / B;
    w.per_trip = threads / n_groups;
    w.li = t / n_groups;
    w.chunk = p.chunk;
    w.l_first = p.l_first;
    w.g_begin = p.l_first + l_begin;
    w.g_end = p.l_first + l_end;
    const int64_t q_lo = w.g_begin / p.chunk;
    w.q_stop = l_end > l_begin ? (w.g_end - 1) / p.chunk + 1 : q_lo;
    w.q = q_lo + (b - (int)(q_lo % B) + B) % B + (int64_t)rank * B;      // the first chunk of b at or behind q_lo, then rank more
    w.q_step = (int64_t)per_b * B;
    if (w.li >= w.per_trip) w.q = w.q_stop;
    walk_enter(w);
    return t - w.li * n_groups;
}

// The lane's next local ladder over the flattened (chunk, trip) sequence; -1 when the walk is over, and at every call after that.
AMC_BLK_HD int64_t walk_next(Walk& w)
{
    while (w.q < w.q_stop) {
        if (w.l < w.hi) {
            const int64_t l = w.l;
            w.l += w.per_trip;
            return l;
        }
        w.q += w.q_step;
        walk_enter(w);
    }
    return -1;
}

// The most summands one lane can take in a launch over `len` consecutive ladders, wherever the range begins: the range meets at most
// (len + C - 2) div C + 1 chunks, every B-th of them belongs to one b, every (grid / B)-th of those to one HIP block, and a chunk
// takes ceil(min(C, len) / per_trip) trips.  Never below the truth, 1 for len = 1, and it does not fall as len grows.
AMC_BLK_HD int64_t lane_bound(int64_t len, int n_blocks, int64_t chunk, int n_groups, int grid, int threads)
{
    const int64_t per_trip = threads / n_groups, per_b = grid / n_blocks;
    const int64_t met = (len + chunk - 2) / chunk + 1;
    const int64_t of_b = (met + n_blocks - 1) / n_blocks;
    const int64_t of_rank = (of_b + per_b - 1) / per_b;
    const int64_t widest = len < chunk ? len : chunk;
    return of_rank * ((widest + per_trip - 1) / per_trip);
}

// Ladders per launch: the longest range whose lane_bound stays within `cap` (the host splits the pass into launches of that many
// ladders, as rung_pass_plan does).  cap >= 1; n_ladders >= 1.
AMC_BLK_HD int64_t ladders_per_launch(int64_t n_ladders, int n_blocks, int64_t chunk, int n_groups, int grid, int threads, int64_t cap)
{
    int64_t lo = 1, hi = n_ladders;              // lane_bound(lo) <= cap holds throughout
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (lane_bound(mid, n_blocks, chunk, n_groups, grid, threads) <= cap) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The grid of a blocked pass: `grid` rounded up to a multiple of B.
AMC_BLK_HD int grid_round(int grid, int n_blocks) { return (grid + n_blocks - 1) / n_blocks * n_blocks; }

}  // namespace blk
}  // namespace amc

#ifndef AMC_BLOCKS_INDEX_ONLY

#include "amc_corr.h"

namespace amc {

// bridge_sums_kernel with the traversal of blk::Walk: HIP block k sums the ladders of jackknife block k mod B alone, so its rows are
// rows of that block; the summands (bridge_add), the lane arithmetic and the end of the block are the unpartitioned pass's own.  Four
// ladders' loads in flight per lane across the flattened (chunk, trip) sequence.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void bridge_sums_blocks_kernel(const BridgeArgs a, const blk::Part part)
{
    constexpr int MAX_SLOTS = AMC_MAX_RUNGS * BR_COLS;
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];                               // exp for every potential
    __shared__ int s_top[MAX_SLOTS];
    __shared__ unsigned int s_flags[MAX_SLOTS];
    __shared__ unsigned long long s_k[MAX_SLOTS][4];
    const int n_slots = a.n_rungs * BR_COLS;
    group_slots_clear(n_slots, s_top, s_flags, s_k);
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);                  // (ends in a barrier: the slots are cleared too)

    blk::Walk w;
    const int r = blk::walk_begin(w, part, a.n_rungs, (int)gridDim.x, AMC_BLOCK, (int)blockIdx.x, (int)threadIdx.x, a.l_begin, a.l_end);
    int mine = bridge_cols_at(a.cols, r, a.n_rungs);
    const bool fwd = (mine & (BR_WF | BR_MF)) != 0, bwd = (mine & (BR_WB | BR_MB)) != 0;
    RLaneCols<BR_COLS> L;
    rl_init(L);
    real_t x0, x1, x2, x3, b0, b1, b2, b3, n0, n1, n2, n3, p0, p1, p2, p3;
    for (;;) {
        const int64_t l0 = blk::walk_next(w), l1 = blk::walk_next(w), l2 = blk::walk_next(w), l3 = blk::walk_next(w);
        if (l3 < 0) {                                             // fewer than four are left: one by one
            const int64_t rest[3] = {l0, l1, l2};
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (rest[j] >= 0) {
                    bridge_load<POT>(a, rest[j] * a.n_rungs + r, fwd, bwd, x0, b0, n0, p0);
                    bridge_add<POT>(L, x0, b0, n0, p0, s_math, mine);
                }
            break;
        }
        bridge_load<POT>(a, l0 * a.n_rungs + r, fwd, bwd, x0, b0, n0, p0);
        bridge_load<POT>(a, l1 * a.n_rungs + r, fwd, bwd, x1, b1, n1, p1);
        bridge_load<POT>(a, l2 * a.n_rungs + r, fwd, bwd, x2, b2, n2, p2);
        bridge_load<POT>(a, l3 * a.n_rungs + r, fwd, bwd, x3, b3, n3, p3);
        bridge_add<POT>(L, x0, b0, n0, p0, s_math, mine);
        bridge_add<POT>(L, x1, b1, n1, p1, s_math, mine);
        bridge_add<POT>(L, x2, b2, n2, p2, s_math, mine);
        bridge_add<POT>(L, x3, b3, n3, p3, s_math, mine);
    }
    if (L.n == 0) mine = 0;
    group_rows_end<BR_COLS>(L, r, mine, n_slots, s_top, s_flags, s_k, a.rows + (int64_t)blockIdx.x * n_slots * XS_ROW_R);
}

// corr_sums_kernel with the same traversal (a mark stores the origin values of the ladders it visits: every local ladder, once).
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void corr_sums_blocks_kernel(const CorrArgs a, const blk::Part part)
{
    constexpr int MAX_SLOTS = AMC_MAX_RUNGS * CORR_COLS;
    __shared__ AMC_MATH_LDS_ALIGN double s_math[POT == POT_CUSTOM ? TAB_DOUBLES : 1];      // a custom potential may call amc_exp
    __shared__ int s_top[MAX_SLOTS];
    __shared__ unsigned int s_flags[MAX_SLOTS];
    __shared__ unsigned long long s_k[MAX_SLOTS][4];
    const int n_slots = a.n_rungs * CORR_COLS;
    group_slots_clear(n_slots, s_top, s_flags, s_k);
    if (POT == POT_CUSTOM) stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier)

    blk::Walk w;
    const int r = blk::walk_begin(w, part, a.n_rungs, (int)gridDim.x, AMC_BLOCK, (int)blockIdx.x, (int)threadIdx.x, a.l_begin, a.l_end);
    RLaneCols<CORR_COLS> L;
    rl_init(L);
    for (;;) {
        const int64_t l0 = blk::walk_next(w), l1 = blk::walk_next(w), l2 = blk::walk_next(w), l3 = blk::walk_next(w);
        if (l3 < 0) {
            const int64_t rest[3] = {l0, l1, l2};
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (rest[j] >= 0) {
                    const int64_t i = rest[j] * a.n_rungs + r;
                    corr_add<POT>(L, a.x[i], a.mark ? 0.0 : a.origin[i], a, i, s_math);
                }
            break;
        }
        const int64_t i0 = l0 * a.n_rungs + r, i1 = l1 * a.n_rungs + r, i2 = l2 * a.n_rungs + r, i3 = l3 * a.n_rungs + r;
        const real_t x0 = a.x[i0], x1 = a.x[i1], x2 = a.x[i2], x3 = a.x[i3];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (!a.mark) {
            a0 = a.origin[i0];
            a1 = a.origin[i1];
            a2 = a.origin[i2];
            a3 = a.origin[i3];
        }
        corr_add<POT>(L, x0, a0, a, i0, s_math);
        corr_add<POT>(L, x1, a1, a, i1, s_math);
        corr_add<POT>(L, x2, a2, a, i2, s_math);
        corr_add<POT>(L, x3, a3, a, i3, s_math);
    }
    __syncthreads();                                              // the slots are cleared
    group_rows_end<CORR_COLS>(L, r, L.n > 0 ? (1 << CORR_COLS) - 1 : 0, n_slots, s_top, s_flags, s_k,
                               a.rows + (int64_t)blockIdx.x * n_slots * XS_ROW_R);
}

}  // namespace amc

#endif  // AMC_BLOCKS_INDEX_ONLY
