// amc_chainstats.h -- convergence per group from running sums PER CHAIN (amc_chain_stats_accumulate .. amc_chain_stats_fetch; DESIGN.md
// section 3.18): chain_stats_add_kernel<POT>, the pass that adds one sample of the observable to every chain's own S and Q,
// chain_stats_sums_kernel, the reproducible sums over the chains of a group of what the chains hold, and chain_stats_finish_kernel,
// which leaves them as [G][7] rows.
// Part of the kernel sources of the many-chain Metropolis engine (gfx950 / CDNA4); amc_kernels.h includes all of them, in order.
#pragma once

#include "amc_ehist.h"

namespace amc {

// Per local chain i and part p (the two halves of the window): S[p][i] = the running sum of o_i, Q[p][i] = of fl(o_i o_i), o_i the
// observable of the time correlation (amc_corr.h: CORR_E, CORR_X).  One sample does S <- S + o, Q <- Q + fl(o o): the product and
// each addition round once, nothing is contracted -- sequential in time per chain, so no function of the grid.
// The fetch sums over the chains i = l G + g of group g, kind R (amc_xsum.h), column by column:
//   S0  S[0][i]   S0S0  fl(S[0][i] S[0][i])   Q0  Q[0][i]     S1, S1S1, Q1 likewise of part 1     S0S1  fl(S[0][i] S[1][i])
// A NaN or an infinity flags the sums it is a summand of, as in the time correlation.
enum { CS_PARTS = 2, CS_COLS = 7 };
// The buffer d_sums: [CS_PARTS][S, Q][n_chains] doubles -- the layout amc_chain_stats_download returns.

struct ChainStatsArgs {
    const real_t* x;              // [n_chains] positions of the local shard
    double* s;                    // [n_chains] S of the part this sample goes to
    double* q;                    // [n_chains] Q of the same part
    int64_t n_chains;
    int32_t observable;           // CORR_E or CORR_X
};

template <int POT, bool OBS_X>
__device__ __forceinline__ void chain_stats_add(const ChainStatsArgs& a, int64_t i, real_t x, double s, double q, const double* s_math)
{
    const double o = OBS_X ? (double)x : (double)potential<POT>(x, s_math);
    a.s[i] = s + o;
    a.q[i] = q + o * o;
}

// The loop of one observable: chain i = thread id, then a grid of chains further per trip, so neighbouring lanes read and write
// neighbouring chains; four chains in flight per lane, their x and their accumulators loaded before any arithmetic (one load per trip
// leaves such a pass waiting for latency: histogram_kernel).  Every chain is read and written by exactly one lane: plain vector loads
// and stores, no atomic, no LDS, no barrier.
template <int POT, bool OBS_X>
__device__ __forceinline__ void chain_stats_walk(const ChainStatsArgs& a, const double* s_math)
{
    const int64_t step = (int64_t)gridDim.x * AMC_BLOCK;
    int64_t i = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    for (; i + 3 * step < a.n_chains; i += 4 * step) {
        const real_t x0 = a.x[i], x1 = a.x[i + step], x2 = a.x[i + 2 * step], x3 = a.x[i + 3 * step];
        const double s0 = a.s[i], s1 = a.s[i + step], s2 = a.s[i + 2 * step], s3 = a.s[i + 3 * step];
        const double q0 = a.q[i], q1 = a.q[i + step], q2 = a.q[i + 2 * step], q3 = a.q[i + 3 * step];
        chain_stats_add<POT, OBS_X>(a, i, x0, s0, q0, s_math);
        chain_stats_add<POT, OBS_X>(a, i + step, x1, s1, q1, s_math);
        chain_stats_add<POT, OBS_X>(a, i + 2 * step, x2, s2, q2, s_math);
        chain_stats_add<POT, OBS_X>(a, i + 3 * step, x3, s3, q3, s_math);
    }
    for (; i < a.n_chains; i += step) chain_stats_add<POT, OBS_X>(a, i, a.x[i], a.s[i], a.q[i], s_math);
}

// The hot pass: 8 B (4 B: Float32 state) of x read, 16 B of S and Q read and written per chain.  The observable is the same for the
// whole launch: the branch is wave-uniform, and the X side never evaluates the potential.  The math tables are staged where
// corr_sums_kernel stages them: for a custom potential, which may call amc_exp.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void chain_stats_add_kernel(const ChainStatsArgs a)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[POT == POT_CUSTOM ? TAB_DOUBLES : 1];
    if (a.observable == CORR_X) {
        chain_stats_walk<POT, true>(a, s_math);
        return;
    }
    if (POT == POT_CUSTOM) stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier)
    chain_stats_walk<POT, false>(a, s_math);
}

#if AMC_PLAIN_KERNELS
struct ChainStatsSumsArgs {
    const double* sums;           // [CS_PARTS][S, Q][n_chains] the accumulators of the local shard
    int64_t n_chains;
    xs_word* rows;                // [gridDim.x][n_rungs][CS_COLS][XS_ROW_R]: this launch's block rows
    int64_t l_begin, l_end;       // the ladders of this launch: at most XS_LANE_CAP - 2 trips per lane (the host splits beyond)
    int32_t n_rungs;              // G: the groups (R of the ladder; 1 without one: a "ladder" is then one chain)
    int32_t cols;                 // (the frame's field; every column is formed)
};

__device__ __forceinline__ void chain_stats_deposit(RLaneCols<CS_COLS>& L, double s0, double q0, double s1, double q1)
{
    rl_deposit(L, 0, s0);
    rl_deposit(L, 1, s0 * s0);
    rl_deposit(L, 2, q0);
    rl_deposit(L, 3, s1);
    rl_deposit(L, 4, s1 * s1);
    rl_deposit(L, 5, q1);
    rl_deposit(L, 6, s0 * s1);
    L.n += 1;
}

// corr_sums_kernel's frame over the four arrays instead of x: thread id = l0 G + g, a thread keeps its group and advances by
// (threads / G) ladders per trip, four chains -- sixteen loads -- in flight per lane; 32 B read per chain, no potential, so one kernel
// for every model and state type.  Prologue and block end are the frame's (amc_exchange.h "the frame of the sums by group").
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void chain_stats_sums_kernel(const ChainStatsSumsArgs a)
{
    constexpr int MAX_SLOTS = AMC_MAX_RUNGS * CS_COLS;
    __shared__ int s_top[MAX_SLOTS];
    __shared__ unsigned int s_flags[MAX_SLOTS];
    __shared__ unsigned long long s_k[MAX_SLOTS][4];
    const int n_slots = a.n_rungs * CS_COLS;
    group_slots_clear(n_slots, s_top, s_flags, s_k);

    const double *S0 = a.sums, *Q0 = a.sums + a.n_chains, *S1 = a.sums + 2 * a.n_chains, *Q1 = a.sums + 3 * a.n_chains;
    const int64_t tid = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    const int64_t ladders_per_trip = ((int64_t)gridDim.x * AMC_BLOCK) / a.n_rungs;
    const int64_t l0 = tid / a.n_rungs;
    const int r = (int)(tid - l0 * a.n_rungs);
    RLaneCols<CS_COLS> L;
    rl_init(L);
    if (l0 < ladders_per_trip) {
        const int64_t step = ladders_per_trip * a.n_rungs;        // chains per trip
        const int64_t end = a.l_end * a.n_rungs;                  // chain l G + g lies below it exactly when l < l_end
        int64_t i = (a.l_begin + l0) * a.n_rungs + r;
        for (; i + 3 * step < end; i += 4 * step) {
            const int64_t i1 = i + step, i2 = i + 2 * step, i3 = i + 3 * step;
            const double a0 = S0[i], a1 = S0[i1], a2 = S0[i2], a3 = S0[i3];
            const double b0 = Q0[i], b1 = Q0[i1], b2 = Q0[i2], b3 = Q0[i3];
            const double c0 = S1[i], c1 = S1[i1], c2 = S1[i2], c3 = S1[i3];
            const double d0 = Q1[i], d1 = Q1[i1], d2 = Q1[i2], d3 = Q1[i3];
            chain_stats_deposit(L, a0, b0, c0, d0);
            chain_stats_deposit(L, a1, b1, c1, d1);
            chain_stats_deposit(L, a2, b2, c2, d2);
            chain_stats_deposit(L, a3, b3, c3, d3);
        }
        for (; i < end; i += step) chain_stats_deposit(L, S0[i], Q0[i], S1[i], Q1[i]);
    }
    __syncthreads();                                              // the slots are cleared
    group_rows_end<CS_COLS>(L, r, L.n > 0 ? (1 << CS_COLS) - 1 : 0, n_slots, s_top, s_flags, s_k, a.rows + (int64_t)blockIdx.x * n_slots * XS_ROW_R);
}

// The launches' block rows merged into the rows [g][c] at `acc`, in corr_finish_kernel's form without a partition: written once per
// fetch, whatever an earlier fetch left there is replaced.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(64) void chain_stats_finish_kernel(const xs_word* rows, int n_rows, int n_groups, xs_word* acc)
{
    const int n_slots = n_groups * CS_COLS, s = blockIdx.x;
    const xs::PartR p = group_rows_merge(rows, n_rows, n_slots, s, 0, 1);
    if (threadIdx.x == 0) xs_store_r_row(acc + (int64_t)s * XS_ROW_R, p);
}
#endif

}  // namespace amc
