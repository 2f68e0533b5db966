// amc_anneal.h -- population annealing: one annealing step beta -> beta' resamples the whole ensemble in
// proportion to exp(-(beta' - beta) e), exactly and independent of the grid.  Five passes, each a launch of its own (no pass waits on
// another block: the multi-block prefix is the three-launch form):
//   anneal_logw_kernel<POT>   a_i = double((-e_i) delta) per chain, and the maximum over the non-NaN ones (one 64-bit atomic per block)
//   anneal_weights_kernel     W_i = floor(2^30 exp(a_i - a_max)) per chain, and the sum of every tile of ANNEAL_TILE chains
//   anneal_block_sums_kernel  only under amc_set_anneal_blocks: n_b and T_b = sum of W per block of families, the step's block record
//   anneal_total_kernel       one block: the exclusive prefix of the tile sums, T_w, the offset U, the step's record
//   anneal_prefix_kernel      C_i = tile offset + scan inside the tile, and from it N_i, the number of child slots j with
//                             j T_w + U < C_i M (128-bit integers); the children of chain i are the slots [N_(i-1), N_i)
//   anneal_gather_kernel      x'_j = x_parent(j), parent(j) = the first i with N_i > j (one binary search over N per child)
// Work is laid out by TILES of the chain index, not by blocks of the grid: a block walks tiles blockIdx.x, + gridDim.x, ..., so every
// stored word is a function of the chains alone.  The family kernels (family_count_kernel, family_stats_kernel) count the surviving
// families of amc_set_anneal_families.  The reference has no such algorithm of its own (as with replica exchange: a user would write it
// as an AriannaAlgorithm over simulation.chains); with the chains in HBM the engine provides the cross-chain move.
// Part of the kernel sources of the many-chain Metropolis engine (gfx950 / CDNA4); amc_kernels.h includes all of them, in order.
#pragma once

#include "amc_exchange.h"

#define AMC_ANNEAL_WEIGHT_BITS 30

namespace amc {

enum : uint32_t { STREAM_ANNEAL = 4 };

enum { ANNEAL_ITEMS = 4, ANNEAL_TILE = ANNEAL_ITEMS * AMC_BLOCK };      // chains per thread and per tile of the prefix passes

// The step's scratch words in device memory: the maximum as an ordered key (0: no chain had a non-NaN a), T_w, U.
enum { ANNEAL_S_KEY = 0, ANNEAL_S_TOTAL = 1, ANNEAL_S_OFFSET = 2, ANNEAL_S_WORDS = 4 };
// One record of the log, 64-bit words.
enum { ANNEAL_R_STATUS = 0, ANNEAL_R_BETA_FROM = 1, ANNEAL_R_BETA_TO = 2, ANNEAL_R_AMAX = 3, ANNEAL_R_TOTAL = 4, ANNEAL_R_OFFSET = 5,
       ANNEAL_R_PARENTS = 6, ANNEAL_R_MAX_CHILDREN = 7, ANNEAL_R_WORDS = 8 };
// Status of a step: resampled; every a_i NaN; a_max = +Inf; a_max = -Inf (every weight zero).  Anything but ANNEAL_OK leaves x alone.
enum { ANNEAL_OK = 0, ANNEAL_ALL_NAN = 1, ANNEAL_INF = 2, ANNEAL_NO_WEIGHT = 3 };
// The most blocks of families (AMC_MAX_JK_BLOCKS of include/amc.h); a block record holds n_b, then T_b: 2 B words.
enum { ANNEAL_MAX_BLOCKS = 64 };

// A non-NaN double as an unsigned key whose integer order is the order of the values (-0 below +0), never 0.
__device__ __forceinline__ uint64_t anneal_key(double a)
{
    const uint64_t b = (uint64_t)__double_as_longlong(a);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double anneal_unkey(uint64_t key)
{
    return __longlong_as_double((long long)((key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key));
}
__device__ __forceinline__ int anneal_status(uint64_t key)
{
    if (key == 0ull) return ANNEAL_ALL_NAN;
    const double a_max = anneal_unkey(key);
    if (a_max == __builtin_huge_val()) return ANNEAL_INF;
    if (a_max == -__builtin_huge_val()) return ANNEAL_NO_WEIGHT;
    return ANNEAL_OK;
}

struct AnnealLogwArgs {
    const real_t* x;              // [n_chains] positions
    unsigned long long* a;        // [n_chains] out: the bits of a_i
    unsigned long long* scratch;  // [ANNEAL_S_WORDS]; ANNEAL_S_KEY was zeroed on the stream in front of this launch
    int64_t n_chains;
    double delta;                 // T(beta_new) - T(beta), formed in T by the host: its conversion back to T is exact
};

// a_i = double((-e_i) delta), the product in T; the block's maximum goes through LDS (one ds atomic per lane that holds a value), then
// one 64-bit atomic per block.  A maximum is the same in any order.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void anneal_logw_kernel(const AnnealLogwArgs a)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_key;
    if (threadIdx.x == 0) s_key = 0ull;
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier)
    const real_t d = (real_t)a.delta;
    const int64_t stride = (int64_t)gridDim.x * AMC_BLOCK;
    unsigned long long key = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x; i < a.n_chains; i += stride) {
        const real_t ne = -potential<POT>(a.x[i], s_math);
        const double ai = (double)(ne * d);
        a.a[i] = (unsigned long long)__double_as_longlong(ai);
        if (ai == ai) {
            const unsigned long long k = anneal_key(ai);
            key = k > key ? k : key;
        }
    }
    if (key) atomicMax(&s_key, key);
    __syncthreads();
    if (threadIdx.x == 0 && s_key) atomicMax(&a.scratch[ANNEAL_S_KEY], s_key);
}

#if AMC_PLAIN_KERNELS
// Inclusive prefix of one value per thread over the block of AMC_BLOCK threads (exact: 64-bit integers), and the block's total.
// Wave scan by shuffles, then the waves' totals through LDS; s_wave holds AMC_BLOCK / 64 words.  Ends in a barrier: s_wave is free again.
__device__ __forceinline__ unsigned long long anneal_block_scan(unsigned long long v, unsigned long long* s_wave, unsigned long long* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned long long base = 0ull, all = 0ull;
#pragma unroll
    for (int w = 0; w < AMC_BLOCK / 64; ++w) {
        if (w < wave) base += s_wave[w];
        all += s_wave[w];
    }
    __syncthreads();
    *total = all;
    return inc + base;
}

// W_i over the bits of a_i (in place) and the tile sums.  Every block returns at once unless the status is ANNEAL_OK.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void anneal_weights_kernel(unsigned long long* w, int64_t n_chains, int64_t n_tiles,
                                                                                       const unsigned long long* scratch, unsigned long long* tile_sums)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned long long s_wave[AMC_BLOCK / 64];
    const unsigned long long key = scratch[ANNEAL_S_KEY];
    if (anneal_status(key) != ANNEAL_OK) return;
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier)
    const double a_max = anneal_unkey(key);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t i0 = tile * ANNEAL_TILE + (int64_t)threadIdx.x * ANNEAL_ITEMS;
        unsigned long long sum = 0ull;
#pragma unroll
        for (int k = 0; k < ANNEAL_ITEMS; ++k) {
            const int64_t i = i0 + k;
            if (i < n_chains) {
                const double ai = __longlong_as_double((long long)w[i]);
                unsigned long long wi = 0ull;
                if (ai == ai && ai != -__builtin_huge_val())
                    wi = (unsigned long long)__builtin_floor(0x1.0p30 * exp_f64(ai - a_max, s_math));
                w[i] = wi;
                sum += wi;
            }
        }
        unsigned long long total;
        (void)anneal_block_scan(sum, s_wave, &total);
        if (threadIdx.x == 0) tile_sums[tile] = total;
    }
}

// ---- weight sums per block of families (amc_set_anneal_blocks; DESIGN.md section 3.14 "Error bars") -----------------------------------
// rec[b] = n_b, the chains whose family lies in block b = (fam div chunk) mod B, and rec[B + b] = T_b, the sum of their W (rec was
// zeroed on the stream in front of this launch).  It runs behind anneal_weights_kernel and in front of anneal_prefix_kernel, which
// overwrites W with N.  w == nullptr, or a status other than ANNEAL_OK (the word then still holds a): every W reads 0, n_b is counted.
// A wave takes 64 consecutive chains per trip, four trips' loads in flight.  fam is non-decreasing after a resampling and a block of
// the default chunk a contiguous range of ids, so the 64 lanes of a trip nearly always share one block: then ONE wave total
// (wave_total_i64) and one pair of LDS atomics per wave; lanes that differ (chunk 1, uploaded ids in any order, a boundary, the ragged
// end) deposit one by one.  The cells are 64-bit in LDS, then at most 2 B 64-bit global atomics per HIP block.  Integer sums: the same in
// any order and on any grid.  chunk is the partition's, capped at 2^32 - 1 by the host (an id is below that: the quotient is 0 either way).
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void anneal_block_sums_kernel(const unsigned long long* w, const uint32_t* fam, int64_t n_chains,
                                                                                          const unsigned long long* scratch, uint32_t chunk, int n_blocks,
                                                                                          unsigned long long* rec)
{
    __shared__ unsigned long long s_cells[2 * ANNEAL_MAX_BLOCKS];
    if (threadIdx.x < 2 * n_blocks) s_cells[threadIdx.x] = 0ull;
    __syncthreads();
    const bool weigh = w != nullptr && anneal_status(scratch[ANNEAL_S_KEY]) == ANNEAL_OK;
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * AMC_BLOCK;
    // (i0 is the wave's first chain: every lane of a wave makes the same trips, so the wave total below sees all 64 lanes)
    for (int64_t i0 = (int64_t)blockIdx.x * AMC_BLOCK + (threadIdx.x - lane); i0 < n_chains; i0 += ANNEAL_ITEMS * stride) {
        int b[ANNEAL_ITEMS];
        unsigned long long wi[ANNEAL_ITEMS];
#pragma unroll
        for (int k = 0; k < ANNEAL_ITEMS; ++k) {
            const int64_t i = i0 + k * stride + lane;
            const bool in = i < n_chains;
            b[k] = in ? (int)((fam[i] / chunk) % (uint32_t)n_blocks) : -1;
            wi[k] = in && weigh ? w[i] : 0ull;
        }
#pragma unroll
        for (int k = 0; k < ANNEAL_ITEMS; ++k) {
            const int b0 = __builtin_amdgcn_readfirstlane(b[k]);
            if (__all(b[k] == b0)) {                              // wave-uniform: all 64 lanes in one block, or all past the end
                if (b0 < 0) continue;
                long long t[1] = {(long long)wi[k]};
                wave_total_i64<1>(t);
                if (lane == 0) {
                    atomicAdd(&s_cells[b0], 64ull);
                    if (t[0]) atomicAdd(&s_cells[n_blocks + b0], (unsigned long long)t[0]);
                }
            } else if (b[k] >= 0) {
                atomicAdd(&s_cells[b[k]], 1ull);
                if (wi[k]) atomicAdd(&s_cells[n_blocks + b[k]], wi[k]);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * n_blocks && s_cells[threadIdx.x]) atomicAdd(&rec[threadIdx.x], s_cells[threadIdx.x]);
}

struct AnnealTotalArgs {
    unsigned long long* tile_sums;    // [n_tiles] in: the tile sums; out: their exclusive prefix
    unsigned long long* scratch;      // [ANNEAL_S_WORDS]
    unsigned long long* rec;          // [ANNEAL_R_WORDS] the step's record in the log
    int64_t n_tiles;
    uint64_t t_a;                     // index of this annealing step
    uint64_t beta_from, beta_to;      // bits
    uint32_t key0, key1;
};

// One block: thread t owns a run of consecutive tile sums, the runs' totals are scanned across the block, and every tile sum is
// replaced by the exclusive prefix in front of it.  Thread 0 forms U = mulhi64(omega, T_w) from the step's one draw and writes the
// record (n_parents and max_children start at 0: anneal_prefix_kernel counts into them).
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void anneal_total_kernel(const AnnealTotalArgs a)
{
    __shared__ unsigned long long s_wave[AMC_BLOCK / 64];
    const unsigned long long key = a.scratch[ANNEAL_S_KEY];
    const int status = anneal_status(key);
    unsigned long long t_w = 0ull, u = 0ull;
    if (status == ANNEAL_OK) {
        const int64_t per = (a.n_tiles + AMC_BLOCK - 1) / AMC_BLOCK;
        const int64_t b = (int64_t)threadIdx.x * per;
        const int64_t e = b + per < a.n_tiles ? b + per : a.n_tiles;
        unsigned long long sum = 0ull;
        for (int64_t i = b; i < e; ++i) sum += a.tile_sums[i];
        unsigned long long run = anneal_block_scan(sum, s_wave, &t_w) - sum;
        for (int64_t i = b; i < e; ++i) {
            const unsigned long long v = a.tile_sums[i];
            a.tile_sums[i] = run;
            run += v;
        }
        const u32x4 w = philox4x32_10(draw_counter(0ull, a.t_a, 0u, STREAM_ANNEAL), a.key0, a.key1);
        const unsigned long long omega = (unsigned long long)w.x | ((unsigned long long)w.y << 32);
        u = __umul64hi(omega, t_w);
    }
    if (threadIdx.x == 0) {
        a.scratch[ANNEAL_S_TOTAL] = t_w;
        a.scratch[ANNEAL_S_OFFSET] = u;
        a.rec[ANNEAL_R_STATUS] = (unsigned long long)status;
        a.rec[ANNEAL_R_BETA_FROM] = a.beta_from;
        a.rec[ANNEAL_R_BETA_TO] = a.beta_to;
        a.rec[ANNEAL_R_AMAX] = key ? (unsigned long long)__double_as_longlong(anneal_unkey(key)) : 0x7FF8000000000000ull;
        a.rec[ANNEAL_R_TOTAL] = t_w;
        a.rec[ANNEAL_R_OFFSET] = u;
        a.rec[ANNEAL_R_PARENTS] = 0ull;
        a.rec[ANNEAL_R_MAX_CHILDREN] = 0ull;
    }
}

// N(C): the number of child slots j in [0, M) with j T_w + U < C M, for 0 <= C <= T_w.  The condition is monotone in j, so N is the
// smallest j in [0, M] with j T_w + U >= C M: a bisection in registers, both sides exact 128-bit integers (M < 2^33, T_w < 2^63).
__device__ __forceinline__ unsigned long long anneal_slots_below(unsigned long long c, unsigned long long m, unsigned long long t_w, unsigned long long u)
{
    const unsigned __int128 rhs = (unsigned __int128)c * m;
    unsigned long long lo = 0ull, hi = m;
    // A Float64 quotient lands within a slot or two of the answer; the bracket it suggests is taken only where the exact condition
    // confirms it (false at g - 3, true at g + 3), so the result is the full bisection's whatever the estimate is worth.
    double est = ((double)c * (double)m - (double)u) / (double)t_w;
    est = est > 0.0 ? est : 0.0;
    const unsigned long long g = (unsigned long long)est;
    if (g >= 3ull && g - 3ull < m && !((unsigned __int128)(g - 3ull) * t_w + u >= rhs)) lo = g - 2ull;
    if (g + 3ull < m && (unsigned __int128)(g + 3ull) * t_w + u >= rhs) hi = g + 3ull;
    while (lo < hi) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if ((unsigned __int128)mid * t_w + u >= rhs) hi = mid;
        else lo = mid + 1ull;
    }
    return lo;
}

// C_i in registers, N_i over W_i (in place), the children counted into the record.  A thread owns ANNEAL_ITEMS consecutive chains; the
// N in front of its first chain is its left neighbour's last N, through LDS (thread 0: N of the tile's offset).  A chain with W = 0
// has C_i = C_(i-1), hence N_i = N_(i-1): no bisection, no child.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void anneal_prefix_kernel(unsigned long long* w, int64_t n_chains, int64_t n_tiles,
                                                                                      const unsigned long long* scratch,
                                                                                      const unsigned long long* tile_offsets, unsigned long long* rec)
{
    __shared__ unsigned long long s_wave[AMC_BLOCK / 64];
    __shared__ unsigned long long s_last[AMC_BLOCK];
    __shared__ unsigned int s_parents;
    __shared__ unsigned long long s_most;
    if (anneal_status(scratch[ANNEAL_S_KEY]) != ANNEAL_OK) return;
    const unsigned long long t_w = scratch[ANNEAL_S_TOTAL], u = scratch[ANNEAL_S_OFFSET], m = (unsigned long long)n_chains;
    if (threadIdx.x == 0) {
        s_parents = 0u;
        s_most = 0ull;
    }
    __syncthreads();
    unsigned int parents = 0u;
    unsigned long long most = 0ull;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t i0 = tile * ANNEAL_TILE + (int64_t)threadIdx.x * ANNEAL_ITEMS;
        unsigned long long wi[ANNEAL_ITEMS], sum = 0ull;
#pragma unroll
        for (int k = 0; k < ANNEAL_ITEMS; ++k) {
            wi[k] = i0 + k < n_chains ? w[i0 + k] : 0ull;
            sum += wi[k];
        }
        unsigned long long total;
        const unsigned long long c = tile_offsets[tile] + (anneal_block_scan(sum, s_wave, &total) - sum);      // C in front of this thread's first chain
        unsigned long long n[ANNEAL_ITEMS];
        unsigned long long cc = c;
        int last = -1;
#pragma unroll
        for (int k = 0; k < ANNEAL_ITEMS; ++k) {
            cc += wi[k];
            n[k] = wi[k] ? anneal_slots_below(cc, m, t_w, u) : 0ull;      // (0: a placeholder, never read)
            if (wi[k]) last = k;
        }
        // the N in front of the first chain: the left neighbour's last one where it formed any, N(c) by a bisection of its own otherwise
        s_last[threadIdx.x] = last >= 0 ? n[last] : ~0ull;      // ~0: "none of mine" (no N is above M)
        __syncthreads();
        unsigned long long before = threadIdx.x ? s_last[threadIdx.x - 1] : ~0ull;
        if (before == ~0ull) before = anneal_slots_below(c, m, t_w, u);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ANNEAL_ITEMS; ++k) {
            if (wi[k]) {
                const unsigned long long children = n[k] - before;
                parents += children != 0ull;
                most = children > most ? children : most;
                before = n[k];
            }
            if (i0 + k < n_chains) w[i0 + k] = before;
        }
    }
    if (parents) atomicAdd(&s_parents, parents);
    if (most) atomicMax(&s_most, most);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_parents) atomicAdd(&rec[ANNEAL_R_PARENTS], (unsigned long long)s_parents);
        if (s_most) atomicMax(&rec[ANNEAL_R_MAX_CHILDREN], s_most);
    }
}

// The first i in [0, n) with N_i > j (N is non-decreasing and N_(n-1) = n > j: there is one).  Runs of equal N -- chains without a
// child, however many -- are stepped over by the bisection itself.
__device__ __forceinline__ int64_t anneal_parent(const unsigned long long* n_cum, int64_t n, unsigned long long j)
{
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (n_cum[mid] > j) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// x'_j = x_parent(j) (4-byte elements with f32), and fam'_j = fam_parent(j) when families are kept.  With a status other than
// ANNEAL_OK the copy is the identity: the host swaps the buffers in every case.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void anneal_gather_kernel(const void* x, void* x_new, int f32, const uint32_t* fam,
                                                                                      uint32_t* fam_new, const unsigned long long* n_cum, int64_t n_chains,
                                                                                      const unsigned long long* scratch)
{
    const bool resample = anneal_status(scratch[ANNEAL_S_KEY]) == ANNEAL_OK;
    const int64_t stride = (int64_t)gridDim.x * AMC_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x; j < n_chains; j += stride) {
        const int64_t p = resample ? anneal_parent(n_cum, n_chains, (unsigned long long)j) : j;
        if (f32) ((float*)x_new)[j] = ((const float*)x)[p];
        else ((double*)x_new)[j] = ((const double*)x)[p];
        if (fam) fam_new[j] = fam[p];
    }
}

// ---- families (amc_set_anneal_families; DESIGN.md section 3.14 "Families") ------------------------------------------------------------
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void family_iota_kernel(uint32_t* fam, int64_t n_chains)
{
    const int64_t stride = (int64_t)gridDim.x * AMC_BLOCK;
    for (int64_t c = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x; c < n_chains; c += stride) fam[c] = (uint32_t)c;
}

// cnt[f] = chains of family f (cnt was zeroed on the stream in front of this launch; every id is below n_chains).
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void family_count_kernel(const uint32_t* fam, int64_t n_chains, unsigned int* cnt)
{
    const int64_t stride = (int64_t)gridDim.x * AMC_BLOCK;
    for (int64_t c = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x; c < n_chains; c += stride) atomicAdd(&cnt[fam[c]], 1u);
}

// out[0] = families with a member, out[1] = sum of n_f^2, out[2] = the largest n_f (out was zeroed in front of this launch): LDS
// first, then three 64-bit atomics per block at most.  Integer sums and a maximum: the same in any order.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void family_stats_kernel(const unsigned int* cnt, int64_t n_chains, unsigned long long* out)
{
    __shared__ unsigned long long s_out[3];
    if (threadIdx.x < 3) s_out[threadIdx.x] = 0ull;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * AMC_BLOCK;
    unsigned long long alive = 0ull, sq = 0ull, largest = 0ull;
    for (int64_t f = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x; f < n_chains; f += stride) {
        const unsigned long long n = cnt[f];
        alive += n != 0ull;
        sq += n * n;
        largest = n > largest ? n : largest;
    }
    if (alive) {
        atomicAdd(&s_out[0], alive);
        atomicAdd(&s_out[1], sq);
        atomicMax(&s_out[2], largest);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_out[threadIdx.x]) atomicAdd(&out[threadIdx.x], s_out[threadIdx.x]);
    if (threadIdx.x == 2 && s_out[2]) atomicMax(&out[2], s_out[2]);
}
#endif

}  // namespace amc
