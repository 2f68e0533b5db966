// amc_anneal_search.h -- population annealing, choosing the next beta (DESIGN.md section 3.14 "Choosing the next beta"): the largest step
// from the shared beta towards a limit whose reweighting keeps the effective-sample fraction ESS / M at or above a target, found by R
// rounds of SEARCH_K candidates each over a bracket [lo, hi] of steps that lives in device memory.  2 R + 1 launches behind one memset,
// none of which waits on another block or on the host:
//   anneal_energy_kernel<POT>     ne_i = -potential(x_i) per chain (exact in Float64), the largest and the smallest of the non-NaN ones
//                                 as ordered keys (LDS atomics, then one 64-bit atomic each per block), the bracket's start
//   anneal_search_sums_kernel     per candidate k: W_i = floor(2^30 exp(a_i - a_max,k)), S1 = sum W, S2h = sum (W^2 >> 30),
//                                 S2l = sum (W^2 & (2^30 - 1)): 24 integer sums per round, the same on any grid
//   anneal_search_decide_kernel   one thread: rho_k from the sums, the first candidate that fails, the new bracket; after the last
//                                 round the step, beta_new and the status
// Part of the kernel sources of the many-chain Metropolis engine (gfx950 / CDNA4); amc_kernels.h includes all of them, in order.
#pragma once

#include "amc_anneal.h"

#define AMC_ANNEAL_SEARCH_CANDIDATES 8

namespace amc {

enum { SEARCH_K = AMC_ANNEAL_SEARCH_CANDIDATES, SEARCH_SUMS = 3 * SEARCH_K, SEARCH_MAX_ROUNDS = 16 };

// The search's words in device memory (all zeroed on the stream in front of the energy pass).  KEY_HI: the ordered key of ne_hi (0: no
// chain had a non-NaN energy); KEY_LO: the COMPLEMENT of the key of ne_lo, so that a maximum finds the minimum and 0 still says "none";
// LO, HI, RHO_LO, RHO_HI: the bracket and the rho of its ends, bits of doubles; DONE: the search has its answer, later passes return at
// once; the sums of round r are the SEARCH_SUMS words from SEARCH_S_HEAD + r * SEARCH_SUMS, candidate k's S1, S2h, S2l at 3 k.
enum { SEARCH_S_KEY_HI = 0, SEARCH_S_KEY_LO = 1, SEARCH_S_LO = 2, SEARCH_S_HI = 3, SEARCH_S_RHO_LO = 4, SEARCH_S_RHO_HI = 5, SEARCH_S_STATUS = 6,
       SEARCH_S_ROUNDS = 7, SEARCH_S_STEP = 8, SEARCH_S_BETA = 9, SEARCH_S_DONE = 10, SEARCH_S_NE_HI = 11, SEARCH_S_NE_LO = 12, SEARCH_S_HEAD = 16,
       SEARCH_S_WORDS = SEARCH_S_HEAD + SEARCH_MAX_ROUNDS * SEARCH_SUMS };
// Status of a search (include/amc.h AMC_ANNEAL_SEARCH_*).
enum { SEARCH_OK = 0, SEARCH_LIMIT = 1, SEARCH_BELOW_RESOLUTION = 2, SEARCH_STALLED = 3, SEARCH_ALL_NAN = 4, SEARCH_INF = 5, SEARCH_NO_WEIGHT = 6 };

__device__ __forceinline__ double search_f64(unsigned long long bits) { return __longlong_as_double((long long)bits); }
__device__ __forceinline__ unsigned long long search_bits(double v) { return (unsigned long long)__double_as_longlong(v); }

// Float64(T(ne) * T(d)): the product in the state's type, as step 1 of amc_anneal forms it.  ne and d are exact in T already.
__device__ __forceinline__ double search_product(double ne, double d, int f32)
{
    return f32 ? (double)((float)ne * (float)d) : ne * d;
}

// The candidates of a round and the largest log-weight of each: delta_k = Float64(T(lo + w c_k)), c_k = (k + 1) / 8, for k < 7 and hi
// itself for k = 7; a_max,k = the product of delta_k with ne_hi (delta_k > 0) or ne_lo.  Every thread of the sums pass and the one
// thread of the decide pass form the same sixteen numbers from the same four words.
__device__ __forceinline__ void search_candidates(double lo, double hi, double ne_hi, double ne_lo, int f32, double (&delta)[SEARCH_K], double (&a_max)[SEARCH_K])
{
    const double w = hi - lo;
#pragma unroll
    for (int k = 0; k < SEARCH_K - 1; ++k) {
        const double d = lo + w * ((double)(k + 1) * 0.125);
        delta[k] = f32 ? (double)(float)d : d;
    }
    delta[SEARCH_K - 1] = hi;
#pragma unroll
    for (int k = 0; k < SEARCH_K; ++k) a_max[k] = search_product(delta[k] > 0.0 ? ne_hi : ne_lo, delta[k], f32);
}

struct AnnealEnergyArgs {
    const real_t* x;              // [n_chains] positions
    unsigned long long* ne;       // [n_chains] out: the bits of Float64(-potential(x_i))
    unsigned long long* scratch;  // [SEARCH_S_WORDS], zeroed on the stream in front of this launch
    int64_t n_chains;
    double span;                  // D = Float64(T(beta_limit) - T(beta)), formed by the host
};

// ne_i and both extremes.  A maximum is the same in any order; the minimum is the maximum of the complemented keys.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void anneal_energy_kernel(const AnnealEnergyArgs a)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_hi, s_lo;
    if (threadIdx.x == 0) s_hi = s_lo = 0ull;
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier)
    if (blockIdx.x == 0 && threadIdx.x == 0) {                // the bracket starts at [0, D] with rho(0) = 1
        a.scratch[SEARCH_S_HI] = search_bits(a.span);
        a.scratch[SEARCH_S_RHO_LO] = search_bits(1.0);
    }
    const int64_t stride = (int64_t)gridDim.x * AMC_BLOCK;
    unsigned long long hi = 0ull, lo = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x; i < a.n_chains; i += stride) {
        const double ne = (double)(-potential<POT>(a.x[i], s_math));
        a.ne[i] = search_bits(ne);
        if (ne == ne) {
            const unsigned long long k = anneal_key(ne);
            hi = k > hi ? k : hi;
            lo = ~k > lo ? ~k : lo;
        }
    }
    if (hi) {
        atomicMax(&s_hi, hi);
        atomicMax(&s_lo, lo);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_hi) {
        atomicMax(&a.scratch[SEARCH_S_KEY_HI], s_hi);
        atomicMax(&a.scratch[SEARCH_S_KEY_LO], s_lo);
    }
}

#if AMC_PLAIN_KERNELS
// The 24 sums of one round.  The stored ne is exact in Float64 whatever the state type, so T is a flag.  A lane keeps the 24 sums of
// its chains in registers (every loop below is unrolled: no array is indexed at run time), the wave totals go through wave_total_i64,
// the four waves meet in LDS, and the block adds with at most 24 atomics.  a <= a_max,k by the monotonicity of rounding, so W <= 2^30
// and W^2 <= 2^60; a difference that is a NaN or -Inf (a NaN or -Inf a; any a where a_max,k is not finite) gives W = 0.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void anneal_search_sums_kernel(const unsigned long long* ne, int64_t n_chains, int f32, int round,
                                                                                           unsigned long long* scratch)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_part[AMC_BLOCK / 64][SEARCH_SUMS];
    const unsigned long long key_hi = scratch[SEARCH_S_KEY_HI];
    if (key_hi == 0ull || scratch[SEARCH_S_DONE]) return;      // (the same in every thread of every block)
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier)
    double delta[SEARCH_K], a_max[SEARCH_K];
    search_candidates(search_f64(scratch[SEARCH_S_LO]), search_f64(scratch[SEARCH_S_HI]), anneal_unkey(key_hi), anneal_unkey(~scratch[SEARCH_S_KEY_LO]), f32,
                      delta, a_max);
    long long acc[SEARCH_SUMS];
#pragma unroll
    for (int c = 0; c < SEARCH_SUMS; ++c) acc[c] = 0ll;
    const int64_t stride = (int64_t)gridDim.x * AMC_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x; i < n_chains; i += stride) {
        const double nei = search_f64(ne[i]);
#pragma unroll
        for (int k = 0; k < SEARCH_K; ++k) {
            const double t = search_product(nei, delta[k], f32) - a_max[k];
            unsigned long long w = 0ull;
            if (t == t && t != -__builtin_huge_val()) w = (unsigned long long)__builtin_floor(0x1.0p30 * exp_f64(t, s_math));
            const unsigned long long sq = w * w;
            acc[3 * k] += (long long)w;
            acc[3 * k + 1] += (long long)(sq >> AMC_ANNEAL_WEIGHT_BITS);
            acc[3 * k + 2] += (long long)(sq & ((1ull << AMC_ANNEAL_WEIGHT_BITS) - 1ull));
        }
    }
    wave_total_i64<SEARCH_SUMS>(acc);                          // (every lane of every wave arrives here)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < SEARCH_SUMS; ++c) s_part[threadIdx.x >> 6][c] = (unsigned long long)acc[c];
    }
    __syncthreads();
    if (threadIdx.x < SEARCH_SUMS) {
        unsigned long long sum = 0ull;
#pragma unroll
        for (int w = 0; w < AMC_BLOCK / 64; ++w) sum += s_part[w][threadIdx.x];
        if (sum) atomicAdd(&scratch[SEARCH_S_HEAD + round * SEARCH_SUMS + threadIdx.x], sum);
    }
}

struct AnnealDecideArgs {
    unsigned long long* scratch;  // [SEARCH_S_WORDS]
    int64_t n_chains;
    int round, rounds, f32;
    double span, beta, beta_limit, target;
};

// The answer of a search that ends without a step of its own (every candidate passed; no usable weights): the limit itself.
__device__ __forceinline__ void search_finish_at_limit(const AnnealDecideArgs& a, int status, int rounds_done)
{
    a.scratch[SEARCH_S_STATUS] = (unsigned long long)status;
    a.scratch[SEARCH_S_ROUNDS] = (unsigned long long)rounds_done;
    a.scratch[SEARCH_S_STEP] = search_bits(a.span);
    a.scratch[SEARCH_S_BETA] = search_bits(a.beta_limit);
    a.scratch[SEARCH_S_DONE] = 1ull;
}

// One thread: the decision of round a.round, and behind the last round the answer.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(64) void anneal_search_decide_kernel(const AnnealDecideArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long* s = a.scratch;
    if (s[SEARCH_S_DONE]) return;
    const unsigned long long key_hi = s[SEARCH_S_KEY_HI];
    if (key_hi == 0ull) {                                      // (round 0: nothing has been written since the memset)
        s[SEARCH_S_NE_HI] = s[SEARCH_S_NE_LO] = 0x7FF8000000000000ull;
        search_finish_at_limit(a, SEARCH_ALL_NAN, 0);
        return;
    }
    const double ne_hi = anneal_unkey(key_hi), ne_lo = anneal_unkey(~s[SEARCH_S_KEY_LO]);
    const double lo = search_f64(s[SEARCH_S_LO]), hi = search_f64(s[SEARCH_S_HI]);
    double delta[SEARCH_K], a_max[SEARCH_K];
    search_candidates(lo, hi, ne_hi, ne_lo, a.f32, delta, a_max);
    if (a.round == 0) {
        s[SEARCH_S_NE_HI] = search_bits(ne_hi);
        s[SEARCH_S_NE_LO] = search_bits(ne_lo);
        const double top = a_max[SEARCH_K - 1];               // (no NaN: a non-NaN energy times a finite D that is not 0)
        if (top == __builtin_huge_val() || top == -__builtin_huge_val()) {
            search_finish_at_limit(a, top > 0.0 ? SEARCH_INF : SEARCH_NO_WEIGHT, 0);
            return;
        }
    }
    const unsigned long long* sums = s + SEARCH_S_HEAD + a.round * SEARCH_SUMS;
    double new_lo = lo, new_hi = hi, rho_lo = search_f64(s[SEARCH_S_RHO_LO]), rho_hi = search_f64(s[SEARCH_S_RHO_HI]);
    bool failed = false;
#pragma unroll
    for (int k = 0; k < SEARCH_K; ++k) {
        const double s1 = (double)sums[3 * k];
        const double s2 = (double)sums[3 * k + 1] * 0x1.0p30 + (double)sums[3 * k + 2];
        const double rho = (s1 * s1) / ((double)a.n_chains * s2);
        if (!failed) {
            if (rho >= a.target) {
                new_lo = delta[k];
                rho_lo = rho;
            } else {                                           // (a NaN rho fails)
                failed = true;
                new_hi = delta[k];
                rho_hi = rho;
            }
        }
    }
    s[SEARCH_S_LO] = search_bits(new_lo);
    s[SEARCH_S_HI] = search_bits(new_hi);
    s[SEARCH_S_RHO_LO] = search_bits(rho_lo);
    s[SEARCH_S_RHO_HI] = search_bits(rho_hi);
    if (!failed) {                                             // every candidate passed, hi = D among them: round 0 only
        search_finish_at_limit(a, SEARCH_LIMIT, a.round + 1);
        return;
    }
    s[SEARCH_S_ROUNDS] = (unsigned long long)(a.round + 1);
    if (a.round + 1 < a.rounds) return;
    int status = SEARCH_OK;
    double step = new_lo;
    if (new_lo == 0.0) {                                       // every candidate of every round failed: the smallest step resolved
        step = new_hi;
        status = SEARCH_BELOW_RESOLUTION;
    }
    const double from = a.f32 ? (double)(float)a.beta : a.beta;
    double beta_new = a.f32 ? (double)((float)a.beta + (float)step) : a.beta + step;
    if (beta_new == from) {
        status = SEARCH_STALLED;
        beta_new = a.beta;
    } else if (a.span > 0.0 ? beta_new > a.beta_limit : beta_new < a.beta_limit) {
        beta_new = a.beta_limit;                               // (the sum's rounding may pass the limit by a last place)
    }
    s[SEARCH_S_STATUS] = (unsigned long long)status;
    s[SEARCH_S_STEP] = search_bits(step);
    s[SEARCH_S_BETA] = search_bits(beta_new);
    s[SEARCH_S_DONE] = 1ull;
}
#endif

}  // namespace amc
