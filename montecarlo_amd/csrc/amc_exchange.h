// amc_exchange.h -- replica exchange along a temperature ladder: exchange_kernel, one step of neighbour
// swaps inside every ladder of R consecutive chains, rung_sums_kernel / rung_finish_kernel, the reproducible sums of e, x, x^2 resolved
// by rung, rung_histogram_kernel, amc_histogram's binning resolved by rung, and walker tracking: exchange_tracked_kernel, the same step
// with TRACK on -- it also moves one label byte per chain and counts trips between the ends --, rung_flow_kernel, the labels counted by
// rung and direction, and respacing: ladder_respace_kernel, new beta values for the interior rungs from the gap or the flow counts
// (the rule itself is amc_respace.h), and ladder_retile_kernel, which lays them over the chains; and tuning the widths per rung:
// rung_sigma_tune_kernel (the rule itself is amc_tune.h) and rung_window_restart_kernel; and the bridge sums: bridge_sums_kernel /
// bridge_finish_kernel, the reproducible sums of e, e^2 and the neighbour-reweighting factors by rung, accumulated over snapshots.
// The reference has no such algorithm of its own: a user writes it as an AriannaAlgorithm whose make_step! walks simulation.chains
// (the plugin protocol, src/algorithms.jl:6-37); with the chains in HBM the engine provides the cross-chain move.
// Part of the kernel sources of the many-chain Metropolis engine (gfx950 / CDNA4); amc_kernels.h includes all of them, in order.
#pragma once

#include "amc_aux_kernels.h"
#if AMC_PLAIN_KERNELS
#include "amc_respace.h"      // (the rule of ladder_respace_kernel, a plain kernel)
#include "amc_tune.h"         // (the rule of rung_sigma_tune_kernel, a plain kernel)
#endif

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

// ---- walker tracking (amc_set_tracking; DESIGN.md section 3.13 "Walker tracking") ------------------------------------------------------
// One label byte per local chain, lab = w | (d << 6): w the walker id (the rung the replica sat at when tracking was turned on), d the
// end it last visited (0 none yet, 1 "up": rung 0, 2 "down": rung R - 1; 3 never occurs).
enum : uint32_t { LAB_WALKER = 0x3Fu, LAB_UP = 1u << 6, LAB_DOWN = 2u << 6 };

struct ExchangeTrackArgs {
    ExchangeArgs step;            // the step itself, as exchange_kernel takes it
    uint8_t* lab;                 // [n_ladders * n_rungs] the labels of the local shard
    unsigned long long* trips;    // [2]: round_trips (a "down" label arrives at rung 0), up_trips (an "up" label arrives at rung R - 1)
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
// TRACK (exchange_tracked_kernel) also carries the labels: the two label bytes are loaded with x and beta, an accepted swap stores them
// crosswise (byte stores; the gaps of one parity share no chain, so no two items touch the same byte, and neighbouring lanes own
// neighbouring byte pairs), and the lanes of the first and the last gap -- a property of the lane, settled before the loop -- apply
// the end rules to the label that arrives at rung 0 / rung R - 1.  With R = 2 the one gap is both.  Trips: two registers, one LDS add
// per lane, one 64-bit atomic per block and touched counter, as the gap counts.  Without TRACK none of that is compiled: a handle
// without tracking launches exchange_kernel and nothing else.
template <int POT, bool TRACK>
__device__ __forceinline__ void exchange_step(const ExchangeArgs& a, uint8_t* lab, unsigned long long* trips)
{
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];
    __shared__ unsigned int s_cnt[2 * AMC_MAX_RUNGS];
    __shared__ unsigned int s_trips[TRACK ? 2 : 1];
    if (threadIdx.x < 2 * AMC_MAX_RUNGS) s_cnt[threadIdx.x] = 0u;
    if constexpr (TRACK)
        if (threadIdx.x < 2) s_trips[threadIdx.x] = 0u;
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier)

    const int64_t tid = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    const int64_t ladders_per_trip = ((int64_t)gridDim.x * AMC_BLOCK) / a.n_gaps;
    const int64_t l0 = tid / a.n_gaps;
    const int r = (int)(a.t_x & 1u) + 2 * (int)(tid - l0 * a.n_gaps);
    const bool at_bottom = r == 0, at_top = r + 1 == a.n_rungs - 1;
    unsigned int attempted = 0u, accepted = 0u, round_trips = 0u, up_trips = 0u;
    if (l0 < ladders_per_trip) {
        for (int64_t l = l0; l < a.n_ladders; l += ladders_per_trip) {
            const int64_t ia = l * a.n_rungs + r;                 // r + 1 < n_rungs: ia + 1 is a chain of the same ladder
            const real_t xa = a.x[ia], xb = a.x[ia + 1];
            const real_t ba = a.beta[ia], bb = a.beta[ia + 1];
            uint32_t la = 0u, lb = 0u;
            if constexpr (TRACK) {
                la = lab[ia];
                lb = lab[ia + 1];
            }
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
                if constexpr (TRACK) {
                    uint32_t na = lb, nb = la;                    // the labels now at rung r and at rung r + 1
                    if (at_bottom) {
                        round_trips += (na >> 6) == 2u;
                        na = (na & LAB_WALKER) | LAB_UP;
                    }
                    if (at_top) {
                        up_trips += (nb >> 6) == 1u;
                        nb = (nb & LAB_WALKER) | LAB_DOWN;
                    }
                    lab[ia] = (uint8_t)na;
                    lab[ia + 1] = (uint8_t)nb;
                }
            }
        }
    }
    if (attempted) atomicAdd(&s_cnt[r], attempted);
    if (accepted) atomicAdd(&s_cnt[AMC_MAX_RUNGS + r], accepted);
    if constexpr (TRACK) {
        if (round_trips) atomicAdd(&s_trips[0], round_trips);
        if (up_trips) atomicAdd(&s_trips[1], up_trips);
    }
    __syncthreads();
    flush_cells(s_cnt, a.counts, 2 * AMC_MAX_RUNGS);
    if constexpr (TRACK) flush_cells(s_trips, trips, 2);
}
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void exchange_kernel(const ExchangeArgs a)
{
    exchange_step<POT, false>(a, nullptr, nullptr);
}
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void exchange_tracked_kernel(const ExchangeTrackArgs ta)
{
    exchange_step<POT, true>(ta.step, ta.lab, ta.trips);
}

// The flow snapshot: counts[r * 3 + d] = local chains at rung r whose label has direction d, one pass over the label bytes.  A thread
// reads four labels as one 32-bit word where the buffer allows (the bytes in front of the first 4-byte boundary and behind the last go
// one by one, thread by thread); the rung of local byte c is c mod R, formed once per word and stepped along its bytes.  Counters live
// in LDS (192 cells at most), then one 64-bit atomic per block and non-zero cell, as rung_histogram_kernel does.
__device__ __forceinline__ void flow_count(unsigned int* s_flow, int r, uint32_t lab)
{
    const uint32_t d = (lab >> 6) & 3u;
    if (d < 3u) atomicAdd(&s_flow[r * 3 + (int)d], 1u);       // (d == 3 never occurs; it must not reach the next rung's cells)
}
#if AMC_PLAIN_KERNELS
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void rung_flow_kernel(const uint8_t* lab, int64_t n_chains, int n_rungs, unsigned long long* counts)
{
    __shared__ unsigned int s_flow[3 * AMC_MAX_RUNGS];
    const int cells = 3 * n_rungs;
    for (int i = threadIdx.x; i < cells; i += AMC_BLOCK) s_flow[i] = 0u;
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * AMC_BLOCK;
    int64_t head = (int64_t)((4u - (uint32_t)(uint64_t)lab) & 3u);
    if (head > n_chains) head = n_chains;
    const int64_t n_words = (n_chains - head) >> 2;
    const int64_t tail = head + 4 * n_words;
    const uint32_t* words = (const uint32_t*)(lab + head);
    for (int64_t i = tid; i < n_words; i += stride) {
        uint32_t v = words[i];
        int r = (int)((head + 4 * i) % n_rungs);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            flow_count(s_flow, r, v & 0xFFu);
            v >>= 8;
            r = r + 1 == n_rungs ? 0 : r + 1;
        }
    }
    if (tid < head) flow_count(s_flow, (int)(tid % n_rungs), lab[tid]);                                   // head <= 3
    if (tid < n_chains - tail) flow_count(s_flow, (int)((tail + tid) % n_rungs), lab[tail + tid]);       // n_chains - tail <= 3
    __syncthreads();
    flush_cells(s_flow, counts, cells);
}
#endif

// ---- respacing the ladder (amc_respace_ladder; DESIGN.md section 3.13 "Respacing") ---------------------------------------------------
// The record of a handle's respacings in device memory, 64-bit words: the status of the last one, the number of status-0 ones, and
// the ladder the last one computed (Float64 bit patterns; read by ladder_retile_kernel when the status is 0).
enum { RESPACE_STATUS = 0, RESPACE_COUNT = 1, RESPACE_OUT = 2, RESPACE_WORDS = 2 + AMC_MAX_RUNGS };

#if AMC_PLAIN_KERNELS
struct RespaceCounts {
    unsigned long long c[3 * AMC_MAX_RUNGS];      // the GLOBAL counts of a call that brings them: the rule's own layout (amc_respace.h)
};
struct RespaceArgs {
    const void* beta;                   // the per-chain beta array: doubles, or floats with f32; the first local ladder is read
    const unsigned long long* xcnt;     // local counts, RS_ACCEPTANCE: d_xcnt, attempted[AMC_MAX_RUNGS] then accepted[AMC_MAX_RUNGS]
    const unsigned long long* flow;     // local counts, RS_FLOW: the flow snapshot n[R][3] rung_flow_kernel has just left
    unsigned long long* gaps;           // d_xcnt again: zeroed with status 0
    unsigned long long* trips;          // [2] the trip counters, zeroed with status 0; nullptr without tracking
    unsigned long long* rec;            // [RESPACE_WORDS] the record above
    unsigned long long* bridge;         // [bridge_words] the accumulator of the bridge sums, zeroed with status 0; nullptr without one
    double gamma, eps;
    int32_t rule, n_rungs, f32, counts_given;
    int32_t bridge_words;               // words of `bridge` (BRIDGE_WORDS, amc_exchange.h "bridge sums")
};

// One block of 64 threads.  Lane r brings b[r] and its counts -- from device memory, or from the kernel argument when the call
// brought global counts -- into LDS; lane 0 runs the rule (serial, a few hundred Float64 operations at most: microseconds); then the
// lanes store the record and, with status 0, zero the gap and the trip counters and the accumulator of the bridge sums.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(64) void ladder_respace_kernel(const RespaceArgs a, const RespaceCounts given)
{
    __shared__ double s_b[AMC_MAX_RUNGS], s_out[AMC_MAX_RUNGS], s_w[AMC_MAX_RUNGS], s_G[AMC_MAX_RUNGS];
    __shared__ uint64_t s_c[3 * AMC_MAX_RUNGS];
    __shared__ int s_status;
    const int r = threadIdx.x, R = a.n_rungs;
    s_out[r] = 0.0;
    if (r < R) {
        s_b[r] = a.f32 ? (double)((const float*)a.beta)[r] : ((const double*)a.beta)[r];
        if (a.rule == rs::RS_ACCEPTANCE) {
            if (r < R - 1) {
                s_c[r] = a.counts_given ? given.c[r] : a.xcnt[r];
                s_c[R - 1 + r] = a.counts_given ? given.c[R - 1 + r] : a.xcnt[AMC_MAX_RUNGS + r];
            }
        } else {
#pragma unroll
            for (int d = 0; d < 3; ++d) s_c[3 * r + d] = a.counts_given ? given.c[3 * r + d] : a.flow[3 * r + d];
        }
    }
    __syncthreads();
    if (r == 0) s_status = rs::respace_rule(a.rule, R, s_b, s_c, a.gamma, a.eps, s_out, s_w, s_G);
    __syncthreads();
    const int status = s_status;
    a.rec[RESPACE_OUT + r] = (unsigned long long)__double_as_longlong(s_out[r]);
    if (r == 0) {
        a.rec[RESPACE_STATUS] = (unsigned long long)status;
        if (status == rs::RS_OK) a.rec[RESPACE_COUNT] += 1ull;
    }
    if (status == rs::RS_OK) {
        a.gaps[r] = 0ull;
        a.gaps[AMC_MAX_RUNGS + r] = 0ull;
        if (a.trips && r < 2) a.trips[r] = 0ull;
        if (a.bridge)                   // sums taken at other beta belong to another ladder
            for (int i = r; i < a.bridge_words; i += 64) a.bridge[i] = 0ull;
    }
}

// The new ladder laid over every local chain: beta_c = T(out[c mod R]), and with tracking the label byte r | (d0(r) << 6).  Returns at
// once unless the record says status 0.  Memory-bound, stores only: 8 B (4 B) per chain, 9 B (5 B) with labels.  Work items as in
// the other exchange kernels: thread id = l0 R + r, a thread keeps its rung -- its beta and its label are formed once -- and advances
// by (threads / R) ladders per trip, so the loop divides nothing and neighbouring lanes write neighbouring chains.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_BLOCK) void ladder_retile_kernel(void* beta, int f32, uint8_t* lab, int64_t n_ladders, int n_rungs,
                                                                                      const unsigned long long* rec)
{
    if (rec[RESPACE_STATUS] != 0ull) return;
    const int64_t tid = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    const int64_t ladders_per_trip = ((int64_t)gridDim.x * AMC_BLOCK) / n_rungs;
    const int64_t l0 = tid / n_rungs;
    if (l0 >= ladders_per_trip) return;
    const int r = (int)(tid - l0 * n_rungs);
    const double b = __longlong_as_double((long long)rec[RESPACE_OUT + r]);
    const float b32 = (float)b;
    const uint8_t label = (uint8_t)((uint32_t)r | (r == 0 ? LAB_UP : r == n_rungs - 1 ? LAB_DOWN : 0u));
    const int64_t step = ladders_per_trip * n_rungs, end = n_ladders * n_rungs;
    for (int64_t i = l0 * n_rungs + r; i < end; i += step) {
        if (f32) ((float*)beta)[i] = b32;
        else ((double*)beta)[i] = b;
        if (lab) lab[i] = label;
    }
}
#endif

// ---- tuning the widths per rung (amc_tune_rung_sigma; DESIGN.md section 3.13 "Tuning the widths") -------------------------------------
// The record of a handle's tunings in device memory, 64-bit words: the number of calls that tuned at least one entry (status 0 or 3)
// since the table was set, then per entry the status of the last call and the width it left (Float64 bit patterns).
enum { TUNE_COUNT = 0, TUNE_ST = 1, TUNE_SIGMA = 1 + AMC_MAX_MOVES, TUNE_WORDS = 1 + 2 * AMC_MAX_MOVES };
// The window base d_rung_base: accepted[AMC_MAX_MOVES] then total[AMC_MAX_MOVES] per entry e = k R + r, as they stood when the window began.
enum { RUNG_BASE_WORDS = 2 * AMC_MAX_MOVES };

#if AMC_PLAIN_KERNELS
struct TuneCounts {
    unsigned long long c[2 * AMC_MAX_MOVES];      // the GLOBAL window of a call that brings it: accepted[K R] then total[K R]
};
struct TuneArgs {
    double* rung_tab;                   // [RT_ROWS][AMC_MAX_MOVES] the rung table: RT_SIGMA is read, all four rows of a tuned entry are written
    const unsigned long long* cnt;      // d_rung_cnt as rung_counter_totals_kernel has just left it: accepted[K R] then total[K R] (the last
                                        // move's total cells hold nothing: it has no total array)
    unsigned long long* base;           // [RUNG_BASE_WORDS] the window base
    unsigned long long* rec;            // [TUNE_WORDS] the record above; nullptr: restart the window only
    unsigned long long steps_per_rung;  // counted steps x local ladders: the calls of all moves together at one rung
    unsigned long long min_calls;
    double target, gamma, lo, hi;
    int32_t n_moves, n_rungs, counts_given;
};

// Entry e's current totals: the accepted cell, and the total cell or -- the pool's last move -- what the other moves left of the
// rung's steps (amc_rung_counter_totals completes it the same way on the host).
__device__ __forceinline__ void rung_current_totals(const TuneArgs& a, int e, unsigned long long& acc, unsigned long long& tot)
{
    const int R = a.n_rungs, K = a.n_moves, cells = K * R;
    const int k = e / R, r = e - k * R;
    acc = a.cnt[e];
    if (k + 1 < K) {
        tot = a.cnt[cells + e];
    } else {
        unsigned long long others = 0ull;
        for (int j = 0; j + 1 < K; ++j) others += a.cnt[cells + j * R + r];
        tot = a.steps_per_rung - others;
    }
}

// One block of AMC_MAX_MOVES threads, lane e owns entry e = k R + r: its window against the base (or the given global window), the
// rule, the record, the four derived rows of the rung table (derive_move_params, as prepare_rung_params_kernel forms them; an entry
// that keeps its sigma keeps its rows), and the base moved to the current totals.  No loop over chains: the only pass over memory
// is the totals pass queued in front.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_MAX_MOVES) void rung_sigma_tune_kernel(const TuneArgs a, const TuneCounts given)
{
    __shared__ int s_any;
    const int e = (int)threadIdx.x, n = a.n_moves * a.n_rungs;
    if (e == 0) s_any = 0;
    __syncthreads();
    if (e < n) {
        unsigned long long acc, tot;
        rung_current_totals(a, e, acc, tot);
        const unsigned long long b_acc = a.base[e], b_tot = a.base[AMC_MAX_MOVES + e];
        const bool bad = !a.counts_given && (acc < b_acc || tot < b_tot);
        const uint64_t A = a.counts_given ? given.c[e] : acc - b_acc;
        const uint64_t T = a.counts_given ? given.c[n + e] : tot - b_tot;
        const double s = a.rung_tab[RT_SIGMA * AMC_MAX_MOVES + e];
        double out;
        const int st = tn::tune_rule(s, A, T, bad, a.target, a.gamma, a.min_calls, a.lo, a.hi, &out);
        a.rec[TUNE_ST + e] = (unsigned long long)st;
        a.rec[TUNE_SIGMA + e] = (unsigned long long)__double_as_longlong(out);
        if (st == tn::TN_OK || st == tn::TN_CLAMPED) {
            double d[DEF_N];
            derive_move_params(out, d);
            a.rung_tab[RT_SIGMA * AMC_MAX_MOVES + e] = d[DEF_SIGMA];
            a.rung_tab[RT_DEN * AMC_MAX_MOVES + e] = d[DEF_DEN];
            a.rung_tab[RT_RDEN * AMC_MAX_MOVES + e] = d[DEF_RDEN];
            a.rung_tab[RT_LOGC * AMC_MAX_MOVES + e] = d[DEF_LOGC];
            s_any = 1;
        }
        a.base[e] = acc;
        a.base[AMC_MAX_MOVES + e] = tot;
    }
    __syncthreads();
    if (e == 0 && s_any) a.rec[TUNE_COUNT] += 1ull;
}

// The window restarted without tuning: base = current totals.
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(AMC_MAX_MOVES) void rung_window_restart_kernel(const TuneArgs a)
{
    const int e = (int)threadIdx.x;
    if (e >= a.n_moves * a.n_rungs) return;
    unsigned long long acc, tot;
    rung_current_totals(a, e, acc, tot);
    a.base[e] = acc;
    a.base[AMC_MAX_MOVES + e] = tot;
}
#endif

// ---- per-rung reproducible sums (amc_reduce_rungs_exact; DESIGN.md section 3.13 "Per-rung sums") ------------------------------------
// S[r][c], c = sum e, sum x, sum x^2: the kind-R sum (amc_xsum.h) over the ladders l of ONE chain's summand, chain l R + r --
// double(potential_T(x)), double(x), fl(double(x) double(x)) -- its level fixed by the largest summand of that rung and column alone.
struct RungSumsArgs {
    const real_t* x;              // [n_ladders * n_rungs] positions of the local shard
    xs_word* rows;                // [gridDim.x][n_rungs][RED_COLS][XS_ROW_R]: this launch's block rows
    int64_t l_begin, l_end;       // the ladders of this launch: at most XS_LANE_CAP - 2 trips per lane (the host splits beyond)
    int32_t n_rungs;              // R
    int32_t cols;                 // RED_WANT_* bits: columns nobody asked for are neither formed nor written
};

// One memory-bound pass, 8 B per chain (4 B for Float32 state).  Work items as in exchange_kernel: thread id = l0 R + r, a thread keeps
// its rung for the whole launch and advances by (threads / R) ladders per trip, so neighbouring lanes read neighbouring chains and the
// loop divides nothing; four loads are in flight per lane.  The lanes of a wave hold DIFFERENT rungs, so each lane keeps its own
// running top (RLaneCols, amc_wave_sums.h) where the whole-ensemble sums keep a wave-uniform one.  Then the frame below.
template <int POT>
__device__ __forceinline__ void rung_add(RLaneCols<RED_COLS>& L, real_t x, const double* s_math, int cols)
{
    const double xd = (double)x;
    if (cols & RED_WANT_E) rl_deposit(L, 0, (double)potential<POT>(x, s_math));
    if (cols & RED_WANT_X) rl_deposit(L, 1, xd);
    if (cols & RED_WANT_XX) rl_deposit(L, 2, xd * xd);
    L.n += 1;
}

// ---- the frame of the sums by group (DESIGN.md section 3.13 "Per-rung sums") -----------------------------------------------------------
// The six sums kernels -- rung_sums_kernel, bridge_sums_kernel, corr_sums_kernel (amc_corr.h), the two blocked forms (amc_blocks.h) and
// chain_stats_sums_kernel (amc_chainstats.h) -- are each: the slot prologue, a loop of their own, the block end; their rows go through ONE finishing merge.  A slot is
// s = g NC + c in LDS, g the lane's group (its rung), c one of the kernel's NC columns: s_top, s_flags and s_k[s] = k1.lo, k1.hi,
// k2.lo, k2.hi (hi: two's complement).
//
// The slot prologue clears them.  THE BARRIER RULE: exactly one barrier lies between this clearing and the first LDS atomic of the
// block end.  A kernel that stages the math tables behind the prologue has it there (stage_math_tables ends in a barrier); every
// other has one __syncthreads() behind its loop, and no kernel has both.
__device__ __forceinline__ void group_slots_clear(int n_slots, int* s_top, unsigned int* s_flags, unsigned long long (*s_k)[4])
{
    for (int s = threadIdx.x; s < n_slots; s += AMC_BLOCK) {
        s_top[s] = xs::XS_LMIN;
        s_flags[s] = 0u;
        s_k[s][0] = s_k[s][1] = s_k[s][2] = s_k[s][3] = 0ull;
    }
}
__device__ __forceinline__ void rung_lds_add(unsigned long long* lo_hi, long long k)
{
    if (k == 0) return;
    atomicAdd(lo_hi, (unsigned long long)(k & 0xFFFFFFFFll));
    atomicAdd(lo_hi + 1, (unsigned long long)(k >> 32));
}
// The block end for a lane with the columns `mine` of group r on its books (0: none, as for a lane that took no summand): (1) the
// slot's top = max of its lanes' tops and the OR of their flags -- integer max / or, order-free --, barrier; (2) the level is settled:
// every lane brings its two integers (xs_r_multiples) to it (xs_r_settle's rule as the choice of the slot: at the top k1, k2 add; one
// level below k1 adds to k2; further below nothing is left) and adds them with 64-bit integer LDS atomics, low 32 bits and high parts
// apart (128 lanes x 2^62 do not fit 64 bits; k = hi 2^32 + lo), barrier; (3) the block stores its rows in the XS_ROW_R form,
// consecutive words by consecutive threads -- those of the columns in `stored` (a slot nobody deposited into is an empty row: top
// XS_LMIN, zeros).  No floating-point atomic anywhere; the rows are integers, so the finishing merge may take them in any order.
template <int NC>
__device__ __forceinline__ void group_rows_end(const RLaneCols<NC>& L, int r, int mine, int n_slots, int* s_top, unsigned int* s_flags,
                                               unsigned long long (*s_k)[4], xs_word* out, int stored = -1)
{
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if ((mine >> c) & 1) {
            atomicMax(&s_top[r * NC + c], L.top[c]);
            if (L.flags[c]) atomicOr(&s_flags[r * NC + c], L.flags[c]);
        }
    __syncthreads();                                              // the levels are settled
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if ((mine >> c) & 1) {
            const int s = r * NC + c;
            xs::RPair k = xs::xs_r_multiples(L.a1[c], L.a2[c], (uint64_t)(unsigned)L.n, L.top[c]);
            const int d = s_top[s] - L.top[c];
            if (d == 0) {
                rung_lds_add(&s_k[s][0], k.k1);
                rung_lds_add(&s_k[s][2], k.k2);
            } else if (d == 1) {
                rung_lds_add(&s_k[s][2], k.k1);
            }
        }
    __syncthreads();
    for (int w = threadIdx.x; w < n_slots * XS_ROW_R; w += AMC_BLOCK) {
        const int s = w / XS_ROW_R, j = w - s * XS_ROW_R;
        if (stored != -1 && !((stored >> (s % NC)) & 1)) continue;
        xs_word v = 0ull;
        if (j == 0) v = (xs_word)(uint32_t)s_top[s] | ((xs_word)s_flags[s] << 32);
        else if (j < 5) {
            const int which = (j - 1) >> 1;                       // k1 / k2
            const xs::i128 k = xs::i128_add(xs::i128_shl(xs::i128_of((long long)s_k[s][2 * which + 1]), 32), xs::i128{(uint64_t)s_k[s][2 * which], 0});
            v = ((j - 1) & 1) ? (xs_word)k.hi : (xs_word)k.lo;
        }
        out[w] = v;
    }
}
// The finishing merge of slot s by one block of 64 threads: lane i merges the rows first + i stride, first + (i + 64) stride, ... of
// the launches' block rows (part_r_merge: integers, so the order is immaterial), thread 0 the lanes' partials; its return value is
// the slot's sum, every other thread's a partial.
__device__ __forceinline__ xs::PartR group_rows_merge(const xs_word* rows, int n_rows, int n_slots, int s, int first, int stride)
{
    __shared__ xs::PartR s_part[64];
    xs::PartR p = xs::part_r_empty();
    for (int k = first + (int)threadIdx.x * stride; k < n_rows; k += 64 * stride)
        xs::part_r_merge(p, xs_load_r_row(rows + ((int64_t)k * n_slots + s) * XS_ROW_R));
    s_part[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < 64; ++i) xs::part_r_merge(p, s_part[i]);
    return p;
}

template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void rung_sums_kernel(const RungSumsArgs a)
{
    constexpr int MAX_SLOTS = AMC_MAX_RUNGS * RED_COLS;
    __shared__ AMC_MATH_LDS_ALIGN double s_math[POT == POT_CUSTOM ? TAB_DOUBLES : 1];      // a custom potential may call amc_exp
    __shared__ int s_top[MAX_SLOTS];
    __shared__ unsigned int s_flags[MAX_SLOTS];
    __shared__ unsigned long long s_k[MAX_SLOTS][4];
    const int n_slots = a.n_rungs * RED_COLS;
    group_slots_clear(n_slots, s_top, s_flags, s_k);
    if (POT == POT_CUSTOM) stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);        // (ends in a barrier)

    const int64_t tid = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    const int64_t ladders_per_trip = ((int64_t)gridDim.x * AMC_BLOCK) / a.n_rungs;
    const int64_t l0 = tid / a.n_rungs;
    const int r = (int)(tid - l0 * a.n_rungs);
    RLaneCols<RED_COLS> L;
    rl_init(L);
    if (l0 < ladders_per_trip) {
        const int64_t step = ladders_per_trip * a.n_rungs;        // chains per trip
        const int64_t end = a.l_end * a.n_rungs;                  // chain l R + r lies below it exactly when l < l_end
        int64_t i = (a.l_begin + l0) * a.n_rungs + r;
        for (; i + 3 * step < end; i += 4 * step) {
            const real_t x0 = a.x[i], x1 = a.x[i + step], x2 = a.x[i + 2 * step], x3 = a.x[i + 3 * step];
            rung_add<POT>(L, x0, s_math, a.cols);
            rung_add<POT>(L, x1, s_math, a.cols);
            rung_add<POT>(L, x2, s_math, a.cols);
            rung_add<POT>(L, x3, s_math, a.cols);
        }
        for (; i < end; i += step) rung_add<POT>(L, a.x[i], s_math, a.cols);
    }
    __syncthreads();                                              // the slots are cleared
    // (the rows of a column nobody asked for are not written: rung_finish_kernel does not read them)
    group_rows_end<RED_COLS>(L, r, L.n > 0 ? a.cols : 0, n_slots, s_top, s_flags, s_k, a.rows + (int64_t)blockIdx.x * n_slots * XS_ROW_R, a.cols);
}

// The records of the rung sums from the block rows of the launches: block s = r RED_COLS + c merges slot s and leaves one record of
// XS_WORDS doubles -- all zero for a column nobody asked for.
#if AMC_PLAIN_KERNELS
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(64) void rung_finish_kernel(const xs_word* rows, int n_rows, int n_rungs, int cols, double* recs)
{
    const int s = blockIdx.x;
    double* rec = recs + (int64_t)s * xs::XS_WORDS;
    if (!((cols >> (s % RED_COLS)) & 1)) {
        if (threadIdx.x < xs::XS_WORDS) rec[threadIdx.x] = 0.0;
        return;
    }
    const xs::PartR p = group_rows_merge(rows, n_rows, n_rungs * RED_COLS, s, 0, 1);
    if (threadIdx.x == 0) xs::rec_from_r(rec, p);
}
#endif

// ---- bridge sums (amc_bridge_accumulate; DESIGN.md section 3.13 "Bridge sums") ---------------------------------------------------------
// S[r][c], c = E, EE, WF, WB, MF, MB: the kind-R sum over the ladders l -- and, through the accumulator, over the snapshots -- of one
// chain's summand, chain i = l R + r, with e = potential_T(x_i) and beta the per-chain array, all products in T without contraction:
//   E  double(e)          EE  fl(double(e) double(e))
//   WF exp(double((-e) (beta_(i+1) - beta_i)))   MF min(1, WF), a NaN stays a NaN      (r + 1 < R)
//   WB exp(double((-e) (beta_(i-1) - beta_i)))   MB min(1, WB)                         (r >= 1)
// The slots without a summand -- WF, MF at rung R - 1, WB, MB at rung 0, every column nobody asked for -- are deposited into by nobody.
enum { BR_E = 1, BR_EE = 2, BR_WF = 4, BR_WB = 8, BR_MF = 16, BR_MB = 32, BR_ALL = 63, BR_COLS = 6 };
// The accumulator d_bridge: one row of XS_ROW_R words per slot s = r BR_COLS + c, AMC_MAX_RUNGS rungs of them, then the number of
// snapshots.  Word 5 of a row is 1 once a snapshot has been merged into it: memory that was zeroed holds empty rows.
enum { BRIDGE_COUNT = AMC_MAX_RUNGS * BR_COLS * XS_ROW_R, BRIDGE_WORDS = BRIDGE_COUNT + 1 };

struct BridgeArgs {
    const real_t* x;              // [n_ladders * n_rungs] positions of the local shard
    const real_t* beta;           // the per-chain beta array
    xs_word* rows;                // [gridDim.x][n_rungs][BR_COLS][XS_ROW_R]: this launch's block rows
    int64_t l_begin, l_end;       // the ladders of this launch: at most XS_LANE_CAP - 2 trips per lane (the host splits beyond)
    int32_t n_rungs;              // R
    int32_t cols;                 // BR_* bits
};

// the columns that have a summand at rung r
__host__ __device__ inline int bridge_cols_at(int cols, int r, int n_rungs)
{
    return cols & ~(r + 1 == n_rungs ? (BR_WF | BR_MF) : 0) & ~(r == 0 ? (BR_WB | BR_MB) : 0);
}
__host__ __device__ inline xs::PartR bridge_load_row(const xs_word* row) { return row[5] ? xs_load_r_row(row) : xs::part_r_empty(); }

__device__ __forceinline__ double min_one(double w) { return (w != w) ? w : (w < 1.0 ? w : 1.0); }      // Julia's min(1, w)

// One chain.  bn, bp: beta of the chains i + 1 and i - 1 (read only where mine names the direction).  exp once per direction, M from W.
template <int POT>
__device__ __forceinline__ void bridge_add(RLaneCols<BR_COLS>& L, real_t x, real_t b, real_t bn, real_t bp, const double* s_math, int mine)
{
    const real_t e = potential<POT>(x, s_math);
    const real_t ne = -e;
    const double ed = (double)e;
    if (mine & BR_E) rl_deposit(L, 0, ed);
    if (mine & BR_EE) rl_deposit(L, 1, ed * ed);
    if (mine & (BR_WF | BR_MF)) {
        const real_t d = bn - b;
        const real_t a = ne * d;
        const double w = exp_f64((double)a, s_math);
        if (mine & BR_WF) rl_deposit(L, 2, w);
        if (mine & BR_MF) rl_deposit(L, 4, min_one(w));
    }
    if (mine & (BR_WB | BR_MB)) {
        const real_t d = bp - b;
        const real_t a = ne * d;
        const double w = exp_f64((double)a, s_math);
        if (mine & BR_WB) rl_deposit(L, 3, w);
        if (mine & BR_MB) rl_deposit(L, 5, min_one(w));
    }
    L.n += 1;
}
template <int POT>
__device__ __forceinline__ void bridge_load(const BridgeArgs& a, int64_t i, bool fwd, bool bwd, real_t& x, real_t& b, real_t& bn, real_t& bp)
{
    x = a.x[i];
    b = a.beta[i];
    bn = fwd ? a.beta[i + 1] : (real_t)0;         // (fwd: r + 1 < R, so i + 1 is a chain of the same ladder; bwd likewise i - 1)
    bp = bwd ? a.beta[i - 1] : (real_t)0;
}

// One memory-bound pass in rung_sums_kernel's form: thread id = l0 R + r, a thread keeps its rung -- and with it the set `mine` of
// columns it deposits into -- for the whole launch, four loads of x in flight per lane; the neighbours' beta are the loads of the
// neighbouring lanes' own beta.  RLaneCols::n counts the summands of the columns in `mine` and of no other: the block end walks
// `mine`, so a slot an end rung has no summand for is never fed an empty sum with n > 0.
template <int POT>
__global__ __launch_bounds__(AMC_BLOCK) void bridge_sums_kernel(const BridgeArgs a)
{
    constexpr int MAX_SLOTS = AMC_MAX_RUNGS * BR_COLS;
    __shared__ AMC_MATH_LDS_ALIGN double s_math[TAB_DOUBLES];                               // exp for every potential
    __shared__ int s_top[MAX_SLOTS];
    __shared__ unsigned int s_flags[MAX_SLOTS];
    __shared__ unsigned long long s_k[MAX_SLOTS][4];
    const int n_slots = a.n_rungs * BR_COLS;
    group_slots_clear(n_slots, s_top, s_flags, s_k);
    stage_math_tables<AMC_BLOCK>(s_math, threadIdx.x);                  // (ends in a barrier: the slots are cleared too)

    const int64_t tid = (int64_t)blockIdx.x * AMC_BLOCK + threadIdx.x;
    const int64_t ladders_per_trip = ((int64_t)gridDim.x * AMC_BLOCK) / a.n_rungs;
    const int64_t l0 = tid / a.n_rungs;
    const int r = (int)(tid - l0 * a.n_rungs);
    int mine = bridge_cols_at(a.cols, r, a.n_rungs);
    RLaneCols<BR_COLS> L;
    rl_init(L);
    if (l0 < ladders_per_trip) {
        const bool fwd = (mine & (BR_WF | BR_MF)) != 0, bwd = (mine & (BR_WB | BR_MB)) != 0;
        const int64_t step = ladders_per_trip * a.n_rungs;        // chains per trip
        const int64_t end = a.l_end * a.n_rungs;                  // chain l R + r lies below it exactly when l < l_end
        int64_t i = (a.l_begin + l0) * a.n_rungs + r;
        real_t x0, x1, x2, x3, b0, b1, b2, b3, n0, n1, n2, n3, p0, p1, p2, p3;
        for (; i + 3 * step < end; i += 4 * step) {
            bridge_load<POT>(a, i, fwd, bwd, x0, b0, n0, p0);
            bridge_load<POT>(a, i + step, fwd, bwd, x1, b1, n1, p1);
            bridge_load<POT>(a, i + 2 * step, fwd, bwd, x2, b2, n2, p2);
            bridge_load<POT>(a, i + 3 * step, fwd, bwd, x3, b3, n3, p3);
            bridge_add<POT>(L, x0, b0, n0, p0, s_math, mine);
            bridge_add<POT>(L, x1, b1, n1, p1, s_math, mine);
            bridge_add<POT>(L, x2, b2, n2, p2, s_math, mine);
            bridge_add<POT>(L, x3, b3, n3, p3, s_math, mine);
        }
        for (; i < end; i += step) {
            bridge_load<POT>(a, i, fwd, bwd, x0, b0, n0, p0);
            bridge_add<POT>(L, x0, b0, n0, p0, s_math, mine);
        }
    }
    if (L.n == 0) mine = 0;
    group_rows_end<BR_COLS>(L, r, mine, n_slots, s_top, s_flags, s_k, a.rows + (int64_t)blockIdx.x * n_slots * XS_ROW_R);
}

// The launches' block rows merged into an accumulator of n_blocks x R x BR_COLS rows [b][r][c]: block (b, s), s = r BR_COLS + c,
// merges slot s of the HIP blocks b, b + B, ... (a blocked pass has grids that are multiples of B, so those are the rows k with
// k mod B == b; the unpartitioned pass is B = 1, b = 0), then the accumulator's own row, which it replaces.  A slot without a summand
// keeps its empty row.  Block 0 counts the snapshot in *count, once: the word BRIDGE_COUNT of d_bridge, the word behind the rows of
// the blocked accumulator.
#if AMC_PLAIN_KERNELS
AMC_KERNEL_LINKAGE __global__ __launch_bounds__(64) void bridge_finish_kernel(const xs_word* rows, int n_rows, int n_rungs, int cols, int n_blocks, xs_word* acc,
                                                                               xs_word* count)
{
    const int n_slots = n_rungs * BR_COLS, b = blockIdx.x / n_slots, s = blockIdx.x - b * n_slots;
    if (blockIdx.x == 0 && threadIdx.x == 0) *count += 1ull;
    if (!((bridge_cols_at(cols, s / BR_COLS, n_rungs) >> (s % BR_COLS)) & 1)) return;
    xs::PartR p = group_rows_merge(rows, n_rows, n_slots, s, b, n_blocks);
    if (threadIdx.x == 0) {
        xs_word* row = acc + ((int64_t)b * n_slots + s) * XS_ROW_R;
        xs::part_r_merge(p, bridge_load_row(row));
        xs_store_r_row(row, p);
        row[5] = 1ull;
    }
}
#endif

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
        const int b = hist_bin(x[c], lo, hi, inv_w, n_bins);
        const int cell = (int)(c % n_rungs) * (n_bins + 3) + b;
        if (lds_rows) atomicAdd(&s_rows[cell], 1u);
        else atomicAdd(&counts[cell], 1ull);
    }
    if (lds_rows) {
        __syncthreads();
        flush_cells(s_rows, counts, cells);
    }
}
#endif

}  // namespace amc
