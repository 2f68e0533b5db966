// amc_exchange.h -- replica exchange along a temperature ladder: exchange_kernel, one step of neighbour
// swaps inside every ladder of R consecutive chains, and rung_histogram_kernel, amc_histogram's binning resolved by rung.
// The reference has no such algorithm of its own: a user writes it as an AriannaAlgorithm whose make_step! walks simulation.chains
// (the plugin protocol, src/algorithms.jl:6-37); with the chains in HBM the engine provides the cross-chain move.
// Part of the kernel sources of the many-chain Metropolis engine (gfx950 / CDNA4); amc_kernels.h includes all of them, in order.
#pragma once

#include "amc_aux_kernels.h"

#define AMC_MAX_RUNGS 64

namespace amc {

enum : uint32_t { STREAM_EXCHANGE = 3 };

struct ExchangeArgs {
    real_t* x;                    // [n_ladders * n_rungs] positions of the local shard
    const real_t* beta;           // the per-chain beta array (a ladder needs one)
    unsigned long long* counts;   // [2][AMC_MAX_RUNGS]: attempted, accepted per gap
    int64_t n_ladders;            // local ladders: n_chains / n_rungs
    uint64_t chain0;              // global id of local chain 0 (a multiple of n_rungs)
    uint64_t t_x;                 // index of this exchange step
    int32_t n_rungs;              // R
    int32_t n_gaps;               // gaps attempted per ladder at this step's parity: (R - parity) / 2, >= 1
    uint32_t key0, key1;
};

// One exchange step.  Gap r of ladder l pairs the chains a = l R + r and b = a + 1; the step attempts the gaps with r mod 2 == t_x mod 2.
//   e = potential(x)      (Particle.e is potential(x) by construction, particle_1d.jl:13-15,33)
//   delta = (((-e_b) beta_a) + ((-e_a) beta_b)) - (((-e_a) beta_a) + ((-e_b) beta_b))       in T, the log target of particle_1d.jl:20-22
//   alpha = min(1, exp(delta)), Julia's min (a NaN stays a NaN); accept iff alpha > u (strict), u = rand(Float64) of the gap's own draw
//   accept: x_a <-> x_b, bit patterns unchanged; beta stays with the rung
// Work items: a thread keeps ONE gap index j (r = parity + 2 j) for the whole launch and walks ladders -- thread id = l0 * n_gaps + j,
// l advancing by (threads / n_gaps) per trip -- so neighbouring lanes read neighbouring chains, the loop divides nothing, and the
// per-gap counts live in two registers until the block's end: one LDS add per lane, then one 64-bit atomic per block and touched
// gap (same-address atomics serialise, ~13 ns each: amc_state.hip hist_grid).  The gaps of one parity share no chain: no two items
// touch the same position.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void exchange_kernel(const ExchangeArgs a)
{
    __shared__ double s_math[TAB_DOUBLES];
    __shared__ unsigned int s_cnt[2 * AMC_MAX_RUNGS];
    if (threadIdx.x < 2 * AMC_MAX_RUNGS) s_cnt[threadIdx.x] = 0u;
    stage_math_tables(s_math, threadIdx.x, AMC_BLOCK);        // (ends in a barrier)

    const int64_t tid = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    const int64_t ladders_per_trip = ((int64_t)gridDim.x * AMC_BLOCK) / a.n_gaps;
    const int64_t l0 = tid / a.n_gaps;
    const int r = (int)(a.t_x & 1u) + 2 * (int)(tid - l0 * a.n_gaps);
    unsigned int attempted = 0u, accepted = 0u;
    if (l0 < ladders_per_trip) {
        for (int64_t l = l0; l < a.n_ladders; l += ladders_per_trip) {
            const int64_t ia = l * a.n_rungs + r;                 // r + 1 < n_rungs: ia + 1 is a chain of the same ladder
            const real_t xa = a.x[ia], xb = a.x[ia + 1];
            const real_t ba = a.beta[ia], bb = a.beta[ia + 1];
            const u32x4 w = philox4x32_10(draw_counter(a.chain0 + (uint64_t)ia, a.t_x, 0u, STREAM_EXCHANGE), a.key0, a.key1);
            const double u = uniform_co(w.x, w.y);
            const real_t nea = -potential<POT>(xa, s_math), neb = -potential<POT>(xb, s_math);
            const real_t delta = ((neb * ba) + (nea * bb)) - ((nea * ba) + (neb * bb));
            const double ex = exp_f64((double)delta, s_math);
            const double alpha = (ex != ex) ? ex : (ex < 1.0 ? ex : 1.0);     // min(1, ex) that keeps a NaN
            ++attempted;
            if (alpha > u) {
                a.x[ia] = xb;
                a.x[ia + 1] = xa;
                ++accepted;
            }
        }
    }
    if (attempted) atomicAdd(&s_cnt[r], attempted);
    if (accepted) atomicAdd(&s_cnt[AMC_MAX_RUNGS + r], accepted);
    __syncthreads();
    if (threadIdx.x < 2 * AMC_MAX_RUNGS && s_cnt[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// amc_histogram's binning (histogram_kernel) with a row per rung: counts[n_rungs][n_bins + 3], the rung of local chain c being
// c mod n_rungs (the shard starts at a multiple of n_rungs).  Rows live in LDS while (n_bins + 3) n_rungs counters fit
// (lds_rows != 0: the dynamic LDS holds them); otherwise every position is one global atomic.
#if AMC_PLAIN_KERNELS
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void rung_histogram_kernel(const double* x, int64_t n_chains, int n_rungs, double lo, double hi,
                                                                                       double inv_w, int n_bins, int lds_rows, unsigned long long* counts)
{
    extern __shared__ unsigned int s_rows[];
    const int cells = (n_bins + 3) * n_rungs;
    if (lds_rows) {
        for (int i = threadIdx.x; i < cells; i += AMC_BLOCK) s_rows[i] = 0u;
        __syncthreads();
    }
    const int64_t stride = (int64_t)gridDim.x * AMC_BLOCK;
    for (int64_t c = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x; c < n_chains; c += stride) {
        const double v = x[c];
        int b;
        if (v != v) b = n_bins + 2;
        else if (v < lo) b = n_bins;
        else if (v >= hi) b = n_bins + 1;
        else {
            b = (int)((v - lo) * inv_w);
            b = b < n_bins ? b : n_bins - 1;       // (hi - ulp - lo) * inv_w can round up to n_bins
        }
        const int cell = (int)(c % n_rungs) * (n_bins + 3) + b;
        if (lds_rows) atomicAdd(&s_rows[cell], 1u);
        else atomicAdd(&counts[cell], 1ull);
    }
    if (lds_rows) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += AMC_BLOCK)
            if (s_rows[i]) atomicAdd(&counts[i], (unsigned long long)s_rows[i]);
    }
}
#endif

}  // namespace amc
