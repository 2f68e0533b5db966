// amc_corr.h -- time correlation from one time origin (amc_corr_mark .. amc_corr_fetch): corr_sums_kernel, the
// reproducible sums of O, O^2 and a O by group, a = the observable at the mark, and corr_finish_kernel, which leaves them in the
// slot of their lag -- with a partition (amc_blocks.h) per jackknife block.
// Part of the kernel sources of the many-chain Metropolis engine (gfx950 / CDNA4); amc_kernels.h includes all of them, in order.
#pragma once

#include "amc_anneal_search.h"

namespace amc {

// S[s][g][c], c = O, OO, AO: the kind-R sum (amc_xsum.h) over the chains i = l G + g of one chain's summand at sample s --
//   O  o_i = double(potential_T(x_i)) (CORR_E) or double(x_i) (CORR_X)     OO  fl(o_i o_i)     AO  fl(a_i o_i)
// a_i = o_i as it was at the mark; the products are Float64, one multiplication each, never contracted.  The level of a sum is fixed
// by the largest summand of its own group, column and sample; a NaN or an infinity flags the sums it is a summand of: a NaN o_i all
// three, a NaN a_i with a finite o_i the AO sum alone.
enum { CORR_E = 1, CORR_X = 2, CORR_COLS = 3, CORR_MAX_LAGS = 256 };
// The accumulator d_corr: one row of XS_ROW_R words per (sample, group, column), rows of a sample together -- the layout of the
// records amc_corr_fetch returns, G as the handle has it while the mark stands.  Room for the most there can be.
enum { CORR_ACC_WORDS = CORR_MAX_LAGS * AMC_MAX_RUNGS * CORR_COLS * XS_ROW_R };

struct CorrArgs {
    const real_t* x;              // [n_ladders * n_rungs] positions of the local shard
    xs_word* rows;                // [gridDim.x][n_rungs][CORR_COLS][XS_ROW_R]: this launch's block rows
    int64_t l_begin, l_end;       // the ladders of this launch: at most XS_LANE_CAP - 2 trips per lane (the host splits beyond)
    int32_t n_rungs;              // G: the groups (R of the ladder; 1 without one: a "ladder" is then one chain)
    int32_t cols;                 // the observable, CORR_E or CORR_X
    double* origin;               // [n_ladders * n_rungs] a_i: read by a sample, WRITTEN by a mark
    int32_t mark;                 // != 0: the launch is a mark -- a_i = o_i is stored, and the sums are those of sample 0
};

template <int POT>
__device__ __forceinline__ void corr_add(RLaneCols<CORR_COLS>& L, real_t x, double a, const CorrArgs& args, int64_t i, const double* s_math)
{
    const double o = args.cols == CORR_X ? (double)x : (double)potential<POT>(x, s_math);
    if (args.mark) {
        args.origin[i] = o;
        a = o;
    }
    rl_deposit(L, 0, o);
    rl_deposit(L, 1, o * o);
    rl_deposit(L, 2, a * o);
    L.n += 1;
}

// One memory-bound pass in the form of rung_sums_kernel / bridge_sums_kernel (amc_exchange.h): thread id = l0 G + g, a thread keeps
// its group for the whole launch and advances by (threads / G) ladders per trip, four loads of x -- and, in a sample, of a -- in
// flight per lane; a mark reads 8 B and writes 8 B per chain, a sample reads 16 B (Float64 state).  Prologue and block end are the
// frame's (amc_exchange.h "the frame of the sums by group"): no floating-point atomic, no block waits on another, plain vector stores
// only.  A block without a chain of a group leaves that group's rows empty.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void corr_sums_kernel(const CorrArgs a)
{
    constexpr int MAX_SLOTS = AMC_MAX_RUNGS * CORR_COLS;
    __shared__ AMC_MATH_LDS_ALIGN double s_math[POT == POT_CUSTOM ? TAB_DOUBLES : 1];      // a custom potential may call amc_exp
    __shared__ int s_top[MAX_SLOTS];
    __shared__ unsigned int s_flags[MAX_SLOTS];
    __shared__ unsigned long long s_k[MAX_SLOTS][4];
    const int n_slots = a.n_rungs * CORR_COLS;
    group_slots_clear(n_slots, s_top, s_flags, s_k);
    if (POT == POT_CUSTOM) stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier)

    const int64_t tid = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    const int64_t ladders_per_trip = ((int64_t)gridDim.x * AMC_BLOCK) / a.n_rungs;
    const int64_t l0 = tid / a.n_rungs;
    const int r = (int)(tid - l0 * a.n_rungs);
    RLaneCols<CORR_COLS> L;
    rl_init(L);
    if (l0 < ladders_per_trip) {
        const int64_t step = ladders_per_trip * a.n_rungs;        // chains per trip
        const int64_t end = a.l_end * a.n_rungs;                  // chain l G + g lies below it exactly when l < l_end
        int64_t i = (a.l_begin + l0) * a.n_rungs + r;
        for (; i + 3 * step < end; i += 4 * step) {
            const real_t x0 = a.x[i], x1 = a.x[i + step], x2 = a.x[i + 2 * step], x3 = a.x[i + 3 * step];
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            if (!a.mark) {
                a0 = a.origin[i];
                a1 = a.origin[i + step];
                a2 = a.origin[i + 2 * step];
                a3 = a.origin[i + 3 * step];
            }
            corr_add<POT>(L, x0, a0, a, i, s_math);
            corr_add<POT>(L, x1, a1, a, i + step, s_math);
            corr_add<POT>(L, x2, a2, a, i + 2 * step, s_math);
            corr_add<POT>(L, x3, a3, a, i + 3 * step, s_math);
        }
        for (; i < end; i += step) corr_add<POT>(L, a.x[i], a.mark ? 0.0 : a.origin[i], a, i, s_math);
    }
    __syncthreads();                                              // the slots are cleared
    group_rows_end<CORR_COLS>(L, r, L.n > 0 ? (1 << CORR_COLS) - 1 : 0, n_slots, s_top, s_flags, s_k, a.rows + (int64_t)blockIdx.x * n_slots * XS_ROW_R);
}

// The launches' block rows merged into the rows [b][g][c] of ONE sample, at which `acc` points: bridge_finish_kernel's blocks and
// strides (n_blocks = 1 without a partition) without an accumulator to add to -- a sample's rows are written once, whatever an
// earlier mark left there is replaced.
#if AMC_PLAIN_KERNELS
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(64) void corr_finish_kernel(const xs_word* rows, int n_rows, int n_groups, int n_blocks, xs_word* acc)
{
    const int n_slots = n_groups * CORR_COLS, b = blockIdx.x / n_slots, s = blockIdx.x - b * n_slots;
    const xs::PartR p = group_rows_merge(rows, n_rows, n_slots, s, b, n_blocks);
    if (threadIdx.x == 0) xs_store_r_row(acc + ((int64_t)b * n_slots + s) * XS_ROW_R, p);
}
#endif

}  // namespace amc
