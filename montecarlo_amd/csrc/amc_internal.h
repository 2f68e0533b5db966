// amc_internal.h -- what the host-side translation units of libamc.so share: the handle, the error convention, the RCCL and
// hiprtc surfaces resolved with dlopen.  Nothing here is part of the C ABI (include/amc.h); the functions declared here have
// hidden visibility.
//   amc_api.hip         errors, expression checks, handle creation and destruction, the knob reader (amc_knobs)
//   amc_state.hip       the ensemble's state: upload / download, histograms, step indices, stream, timing
//   amc_counters.hip    the step log and the per-chain counters (fold, totals, totals per rung, 64-bit carry, upload / download)
//   amc_sweeps.hip      sweep launches (amc_sweep*)
//   amc_exchange.hip    replica exchange along a temperature ladder (amc_set_ladder, amc_exchange, amc_sweep_exchange, gap counters,
//                       the per-rung reproducible sums: amc_reduce_rungs_exact, walker tracking: amc_set_tracking ..,
//                       proposal widths per rung: amc_set_rung_sigma / amc_get_rung_sigma, respacing: amc_respace_ladder ..,
//                       tuning the widths: amc_tune_rung_sigma .., the window of the acceptance per rung: amc_rung_window_*)
//   amc_anneal.hip      population annealing (amc_anneal, its record log, the annealing step index, amc_get_beta, the families:
//                       amc_set_anneal_families .. amc_upload_families; amc_anneal_next_beta)
//   amc_corr.hip        time correlation from one time origin (amc_corr_mark .. amc_corr_clear; per jackknife block: amc_corr_fetch_blocks;
//                       the partition itself, amc_set_blocks, and amc_bridge_fetch_blocks are with the bridge sums in amc_exchange.hip)
//   amc_ehist.hip       energy histograms per group (amc_energy_histogram_accumulate / _fetch, amc_set_energy_histogram; per jackknife
//                       block: amc_energy_histogram_accumulate_blocks / _fetch_blocks, amc_set_energy_histogram_blocks), and what the
//                       life cycle of both accumulators over the energy bins shares (bins_*: respaced, fold, checks, fetch arithmetic)
//   amc_emom.hip        moments per energy bin (amc_energy_moments_accumulate / _fetch, amc_set_energy_moments; per jackknife block:
//                       amc_energy_moments_accumulate_blocks / _fetch_blocks, amc_set_energy_moments_blocks)
//   amc_chainstats.hip  convergence per group: running sums per chain and their sums by group (amc_chain_stats_accumulate ..
//                       amc_chain_stats_clear)
//   amc_reduce.hip      callback reductions (tickets, amc_reduce*, amc_sweep_reduce_begin) and record arithmetic
//   amc_parameters.hip  the parameter table (amc_set / get_parameters, amc_parameters_begin / _end)
//   amc_pg.hip          the estimator's host side (amc_pg_*, amc_pgmc_steps*)
//   amc_rtc.hip         kernels compiled at run time for script-defined models (hiprtc, code-object cache)
//   amc_comm.hip        the engine's own RCCL communicator (amc_comm_*, amc_allreduce_*)
//   amc_selftest.hip    parity-test hooks
//   amc_pg_fused.hip    kernel instantiations built with other code-generation options
#pragma once

#include "../../include/amc.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "amc_kernels.h"
#include "amc_slices.h"

#ifndef AMC_BUILD_ARCH
#define AMC_BUILD_ARCH "gfx950"      // the Makefile passes the arch the offline kernels were compiled for
#endif

#define AMC_INTERNAL __attribute__((visibility("hidden")))

// Every C entry returns 0 or a negative amc_status and leaves its message in a thread-local string (amc_last_error()).
AMC_INTERNAL int fail(int code, const char* fmt, ...);

#define AMC_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? AMC_ERR_OOM : AMC_ERR_HIP, "%s failed: %s",    \
                        #call, hipGetErrorString(e_));                                             \
    } while (0)

// A call that returns an amc_status: anything but AMC_OK is the caller's return value too (its message is already left).
#define AMC_TRY(expr)                                                                              \
    do {                                                                                           \
        const int rc_ = (expr);                                                                    \
        if (rc_ != AMC_OK) return rc_;                                                             \
    } while (0)

// ---- environment variables --------------------------------------------------------------------------------
// Every AMC_* variable libamc.so reads is listed here and read through amc_env() (amc_api.hip), and nowhere else.  Handle knobs are
// read by amc_knobs() in one go: amc_create copies them into the handle, which keeps them for its life; amc_model_check and
// amc_potential_check read them afresh per call.  "dev": exists for A/B measurements and tests only.  Flags count as set when
// atoi(value) != 0, except where "set" says that any value, empty included, sets them.
struct AmcKnobs {
    //                                   variable                       accepted         default  purpose
    int blocks_per_cu = 0;            // AMC_BLOCKS_PER_CU              1..64            0: none  tuning: blocks per CU of every launch
    int blocks_per_cu_single = 0;     // AMC_BLOCKS_PER_CU_SINGLE       1..64            0: none  tuning: ... of single-step sweeps
    int blocks_per_cu_reduce = 0;     // AMC_BLOCKS_PER_CU_REDUCE       1..64            0: none  tuning: ... of sweeps forming the callback sums
    int log_depth = 0;                // AMC_LOG_DEPTH                  1..255           0: none  tuning: rows of the step log
    bool exact_accept = false;        // AMC_EXACT_ACCEPT               flag             off      no accept filter: the reference's arithmetic
    bool wide_counters = false;       // AMC_WIDE_COUNTERS              not "0..."       off      dev: u32 counter arrays where u16 planes do
    bool wide_red_rows = false;       // AMC_WIDE_RED_ROWS              flag             off      dev: the wide rows of the callback sums
    bool shard_route_one_rank = false;  // AMC_SHARD_ROUTE_ON_ONE_RANK  flag             off      dev: one rank takes the estimator route of several
    bool no_deferred_update = false;  // AMC_NO_DEFERRED_UPDATE         flag             off      dev: each fused time step takes its learning step
    bool class_per_move = false;      // AMC_CLASS_PER_MOVE             flag             off      dev: class pools: an estimator launch per move
    bool no_column_skip = false;      // AMC_NO_COLUMN_SKIP             flag             off      dev: fused script steps sum every column
    bool np_small_launches = false;   // AMC_NP_SMALL_LAUNCHES          flag             off      dev: P > 1, several moves: records + small launches
    bool no_sweep_estimator_fusion = false;  // AMC_NO_SWEEP_ESTIMATOR_FUSION  set       off      dev: no sweep rides in an estimator launch
    int sweep_slices = 0;             // AMC_SWEEP_SLICES               1..3             0: none  tuning: concurrent slices of a single-sweep launch (default 2)
    int sweep_slice_blocks_per_cu = 0;  // AMC_SWEEP_SLICE_BLOCKS_PER_CU  1..64          0: none  tuning: blocks per CU of each slice's launch (default 3)
    int64_t sweep_slice_min_chains = -1;  // AMC_SWEEP_SLICE_MIN_CHAINS  >= 0           -1: none tuning: smallest shard that takes the sliced route (2 500 000)
    bool debug_plan = false;          // AMC_DEBUG_PLAN                 set              off      dev: the estimator's launch plans on stderr
    std::string rtc_licm;             // AMC_RTC_LICM                   all-off, est-off, off-for-none: run-time builds without Machine LICM
    bool rtc_waves_set = false;       // AMC_RTC_WAVES                  integer          unset    dev: waves per EU of script estimator forms
    std::string rtc_waves;            //   ... its text (the cache keys carry it as given)
    bool no_gauss_class_rows = false; // AMC_NO_GAUSS_CLASS_ROWS        set              off      dev: Gaussian classes without table rows
    bool no_sigma_memo = false;       // AMC_NO_SIGMA_MEMO              set              off      dev: amc_log(sigma) per lane and step
    bool model_check_f32 = false;     // AMC_MODEL_CHECK_F32            "1..."           off      dev: amc_model_check: Float32 state
    std::string model_check_inst;     // AMC_MODEL_CHECK_INST           instantiation    ""       dev: amc_model_check builds it (tools/rtc_isa.py)
};
// Process settings: read where they are used, through amc_env().
//   AMC_RTC_CACHE_DIR     directory        none             code objects compiled at run time, kept across processes
//   AMC_RTC_WORKER        path             beside the .so   the run-time compiler's program
//   AMC_RTC_TIMEOUT_S     seconds > 0      600              time limit of one run-time build
//   AMC_RTC_IN_PROCESS    "1..."           off              dev: run-time builds inside this process (under a debugger)
//   AMC_RCCL_LIBRARY      path             librccl          that RCCL library and no other
AMC_INTERNAL const char* amc_env(const char* name);
AMC_INTERNAL AmcKnobs amc_knobs();

// Minimal RCCL surface, resolved with dlopen so the library has no link-time RCCL
// dependency and shares the instance a host process may already have loaded.
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, const void*, int) = nullptr;   // id passed by pointer (see shim)
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;       // optional: what the communicator says about itself (amc_comm_info)
    int (*CommUserRank)(void*, int*) = nullptr;
    int (*GetVersion)(int*) = nullptr;
};


static const int RED_HOST_STRIDE = amc::RED_ROW_WORDS;   // 64-bit words per row of the callback sums' block rows (red_finish)
static const int RATIO_STRIDE = 4;      // columns per row of the fold's acceptance-ratio partials (K <= 4): XS_ROW_Q words per move
static const int PG_MAX_COLS = AMC_MAX_LEARN * 4;   // GradientData columns of one estimator launch
static const int PG_NP_MAX_COLS = 1 + 2 * AMC_MAX_NP + AMC_MAX_NP * (AMC_MAX_NP + 1) / 2;   // ... of one move with AMC_MAX_NP parameters (< PG_MAX_COLS)
static const int RED_TICKETS = 2;       // reductions that may be in flight per handle (amc_reduce_begin .. amc_reduce_end)

// One reduction in flight: where its block rows land and what amc_reduce_end needs to finish it.
struct RedTicket {
    bool pending = false;
    int rows = 0;                    // block rows of the sums over x in h_rows
    int ratio_rows = 0;              // rows of h_ratio that belong to it (0: none)
    bool ratio_acc = false;          // the per-move ratio totals come from h_ratio_acc (K > 4)
    uint64_t t_counted = 0;
    int row_stride = RED_HOST_STRIDE;    // words per row of h_rows: the wide form, or amc::RED_COMPACT_WORDS (red_finish)
    int cols = amc::RED_WANT_ALL;        // the sums that were formed (amc_set_reduce_columns at the time)
    hipEvent_t ev = nullptr;
    amc::xs_word* h_rows = nullptr;      // pinned [n_slots][RED_HOST_STRIDE]
    amc::xs_word* h_ratio = nullptr;     // pinned [n_slots][RATIO_STRIDE]
    unsigned long long* d_ratio_acc = nullptr;   // [AMC_MAX_MOVES][3] (reduce_kernel, K > 4)
    unsigned long long* h_ratio_acc = nullptr;   // pinned copy
};

// A model as the run-time compiler is given it (amc_rtc.hip model_prelude): C expressions, "" where one is not given.
struct PolicyClass {
    std::string sample, logq;          // sample_action!(z, x, sigma), log_proposal_density(delta, x, sigma)
    std::vector<std::string> dlogq;    // d logq / d parameter: none (logq is differentiated, amc_dual.h) or one per parameter
    std::string perform, invert;       // the action's perform_action!(x, delta) / invert_action!(delta, x): both or neither (a displacement)
};
struct ModelSpec {
    bool f32 = false, param_f32 = false;     // Float32 state; ... and Float32 policy parameters (kernels built with AMC_PARAM_F32)
    std::string potential, reward, scale;    // "": the built-in potential / the default reward / no proposal-width scale(x)
    int n_params = 1;                        // parameters of the policy (> 1: of the one class)
    std::vector<PolicyClass> classes;        // empty: the built-in Gaussian policy; several: a pool that mixes policies / actions
    std::vector<int> class_of_move;          // ... and the class of each move (the handle's table row: no part of what is compiled)
    std::string cache_text() const;          // the model in the code-object caches' keys (amc_rtc.hip)
};

// ---- state that is owned together: declared, reset and freed together -----------------------------------------------------------------
// Plain structs the handle holds by value.  Below each is its one release function, which frees every device pointer the struct
// declares (tests/test_handle_state_static.py holds it to that); amc_destroy calls them all.

// The temperature ladder and what belongs to it (amc_exchange.hip; the totals per rung: amc_counters.hip).  amc_set_ladder forgets all
// of it but the memory (ladder_reset).
struct LadderState {
    int n_rungs = 0;            // R of the temperature ladder (amc_set_ladder); 0: none
    uint64_t t_x = 0;           // exchange steps done (their own Philox step index; its parity picks the gaps)
    unsigned long long* d_xcnt = nullptr;   // [2][AMC_MAX_RUNGS] exchange attempts and accepted swaps per gap (allocated with the ladder)
    amc::xs_word* d_rung_rows = nullptr;    // [launches * grid][n_rungs][RED_COLS][XS_ROW_R] block rows of the rung sums (amc_reduce_rungs_exact,
    size_t rung_rows_words = 0;             //   allocated at its first use, grown when a call needs more); the words it holds
    double* d_rung_recs = nullptr;          // [AMC_MAX_RUNGS][RED_COLS][XS_WORDS] their records (rung_finish_kernel)
    amc::xs_word* d_bridge = nullptr;       // [BRIDGE_WORDS] the accumulator of the bridge sums: a row per slot, then the number of snapshots
                                            //   (amc_bridge_accumulate / amc_set_bridge; allocated at its first use: a handle that never accumulates has none)
    int bridge_cols = 0;                    // the AMC_BRIDGE_* mask the accumulator was begun with; 0: free (the next amc_bridge_accumulate fixes it)
    uint8_t* d_lab = nullptr;               // [M] walker labels, w | (d << 6) per chain; allocated exactly while tracking is on (amc_set_tracking)
    unsigned long long* d_track = nullptr;  // [2 + 3 * AMC_MAX_RUNGS] round_trips, up_trips, the cells of one flow snapshot (allocated with d_lab)
    unsigned long long* d_respace = nullptr;   // [RESPACE_WORDS] status of the last respacing, the count of status-0 ones, the ladder it computed
                                               // (amc_respace_ladder; allocated at its first use, zeroed by amc_set_ladder)
    // Proposal widths per (move, rung) (amc_set_rung_sigma): a table is set exactly while rung_on; the sweeps then launch the RUNG form,
    // which reads d_rung_tab where the others read ptab's rows
    bool rung_on = false;
    double* d_rung_tab = nullptr;           // [RT_ROWS][AMC_MAX_MOVES] derived rows of entry k * n_rungs + r (allocated by the first table, kept)
    double rung_sigma[AMC_MAX_MOVES] = {0}; // the table as it was given (amc_get_rung_sigma)
    unsigned long long* d_rung_cnt = nullptr;   // [2][cells] accepted, total per (move, rung) (amc_rung_counter_totals; allocated at its first use,
    size_t rung_cnt_cells = 0;                  //   grown when a call needs more)
    // Tuning the widths (amc_tune_rung_sigma .. amc_rung_window_restart): both allocated at their first use, zeroed then; a handle that
    // never tunes and never asks for the window has neither
    unsigned long long* d_rung_base = nullptr;  // [RUNG_BASE_WORDS] accepted, total per (move, rung) at the start of the window (zeroed by amc_set_ladder)
    unsigned long long* d_tune = nullptr;       // [TUNE_WORDS] the record of the tunings (zeroed by amc_set_rung_sigma and amc_set_ladder)
    bool tune_queued = false;                   // a tuning has been queued since the table was set: the device holds the table (amc_get_rung_sigma)
};
static inline void ladder_release(LadderState& s)
{
    (void)hipFree(s.d_xcnt);
    (void)hipFree(s.d_rung_rows);
    (void)hipFree(s.d_rung_recs);
    (void)hipFree(s.d_bridge);
    (void)hipFree(s.d_lab);
    (void)hipFree(s.d_track);
    (void)hipFree(s.d_respace);
    (void)hipFree(s.d_rung_tab);
    (void)hipFree(s.d_rung_cnt);
    (void)hipFree(s.d_rung_base);
    (void)hipFree(s.d_tune);
}

// Population annealing (amc_anneal.hip): all of it allocated at its first use -- a handle that never anneals
// has none
struct AnnealState {
    uint64_t t_a = 0;                           // annealing steps done (their own Philox step index)
    double* d_x_alt = nullptr;                  // [M_pad] the second position buffer: a step gathers d_x into it, then the two change places
    unsigned long long* d_anneal_n = nullptr;   // [M] one word per chain: the bits of a_i, then W_i, then N_i (amc_anneal.h)
    unsigned long long* d_anneal_tiles = nullptr;   // [tiles] the tile sums, then their exclusive prefix
    unsigned long long* d_anneal_s = nullptr;   // [ANNEAL_S_WORDS] the step's scratch words: maximum, T_w, U
    unsigned long long* d_anneal_log = nullptr; // [AMC_ANNEAL_MAX_RECORDS][ANNEAL_R_WORDS] the records of the steps
    int anneal_n = 0;                           // records in the log
    uint32_t* d_fam = nullptr;                  // [M] family id per chain; allocated exactly while families are on (amc_set_anneal_families)
    uint32_t* d_fam_alt = nullptr;              // [M] ... and the buffer a step gathers them into
    unsigned int* d_fam_cnt = nullptr;          // [M] + 3 words: scratch of amc_anneal_family_stats (allocated at its first call)
    unsigned long long* d_anneal_search = nullptr;   // [SEARCH_S_WORDS] the words of amc_anneal_next_beta (allocated at its first call;
                                                     //   its energies go into d_anneal_n)
    // Blocks of families (amc_set_anneal_blocks; DESIGN.md section 3.14 "Error bars"): the partition is set exactly while blk_B != 0
    int blk_B = 0;                              // B; 0: no partition
    int64_t blk_chunk = 0;                      // C: block of a chain = (fam div C) mod B
    unsigned long long* d_blk_log = nullptr;    // [AMC_ANNEAL_MAX_RECORDS][2 B] the block records: n_b, then T_b (allocated by the first step under
                                                //   the partition, freed when it goes)
    int blk_n = 0;                              // block records in the log
    unsigned long long* d_blk_now = nullptr;    // [2 AMC_MAX_JK_BLOCKS] scratch of amc_anneal_block_counts (allocated at its first call)
};
static inline void anneal_release(AnnealState& s)
{
    (void)hipFree(s.d_x_alt);
    (void)hipFree(s.d_anneal_n);
    (void)hipFree(s.d_anneal_tiles);
    (void)hipFree(s.d_anneal_s);
    (void)hipFree(s.d_anneal_log);
    (void)hipFree(s.d_fam);
    (void)hipFree(s.d_fam_alt);
    (void)hipFree(s.d_fam_cnt);
    (void)hipFree(s.d_anneal_search);
    (void)hipFree(s.d_blk_log);
    (void)hipFree(s.d_blk_now);
}

// Time correlation (amc_corr.hip): both buffers allocated at their first use -- a handle that never marks has
// neither.  A mark stands exactly while observable != 0.
struct CorrState {
    int observable = 0;                         // AMC_CORR_E / AMC_CORR_X of the mark; 0: nothing is marked
    int n_samples = 0;                          // slots taken since the mark, slot 0 (the mark's own) included
    int groups = 0;                             // G at the mark (amc_set_ladder clears the mark, so it is the handle's G while the mark stands)
    uint64_t steps[AMC_CORR_MAX_LAGS] = {0};    // the MH step index at each sample
    double* d_origin = nullptr;                 // [M_pad] a_i = O(x_i) at the mark
    amc::xs_word* d_corr = nullptr;             // [CORR_ACC_WORDS] a row per (sample, group, column): the records' layout (amc_corr.h)
};
static inline void corr_release(CorrState& s)
{
    (void)hipFree(s.d_origin);
    (void)hipFree(s.d_corr);
}

// Jackknife blocks (amc_set_blocks): the partition and the blocked accumulators of the bridge sums and of the
// time correlation, each allocated at its first use for the B and G at hand -- a handle that never sets a partition has neither and
// launches what it always did.  A partition is set exactly while n_blocks != 0.
struct BlocksState {
    int n_blocks = 0;                           // B; 0: no partition
    int64_t chunk = 0;                          // C
    amc::xs_word* d_bridge_blk = nullptr;       // [B][R][BR_COLS][XS_ROW_R] rows, then the number of snapshots (amc_blocks.h)
    size_t bridge_blk_words = 0;                //   the words it holds
    amc::xs_word* d_corr_blk = nullptr;         // [samples][B][G][CORR_COLS][XS_ROW_R]
    size_t corr_blk_words = 0;
};
static inline void blocks_release(BlocksState& s)
{
    (void)hipFree(s.d_bridge_blk);
    (void)hipFree(s.d_corr_blk);
}

// The accumulators over the energy bins: what the energy histograms' and the moments' have in common, and all
// their shared life cycle works on (bins_* below; amc_ehist.hip).  An accumulator is allocated at its first use -- a handle that never
// accumulates has none -- and stands exactly while d_words != nullptr; without one the state is the default one.  Its FORM is fixed
// while it stands: the bins, and plain (blocks == 0) or blocked under the partition it was begun with (a set per jackknife block, or
// per block of families); amc_set_blocks folds a blocked one into a plain one.
struct BinsState {
    unsigned long long* d_words = nullptr;      // [blocks or 1] sets of [groups][n_bins + tail] counts, then [groups][cols][n_bins] signed 64-bit sums
    int n_bins = 0;
    int groups = 0;                             // G when it was begun (amc_set_ladder clears it, so it is the handle's G while it stands)
    int blocks = 0;                             // B of a blocked accumulator (the handle's partition while it stands); 0: plain
    bool by_family = false;                     // ... blocked under amc_set_anneal_blocks: a row per block of FAMILIES (amc_ehist.hip)
    int tail = 0;                               // cells behind the bins of a count row: 3 (below, above, NaN), 4 with "beyond x_bound"
    int cols = 0;                               // sum cells per (group, bin): none for the histograms, C = popcount(mask) for the moments
    double lo = 0.0, hi = 0.0;
};
static inline size_t bins_count_cells(const BinsState& s) { return (size_t)s.groups * (size_t)(s.n_bins + s.tail); }      // of one set
static inline size_t bins_sum_cells(const BinsState& s) { return (size_t)s.groups * (size_t)s.cols * (size_t)s.n_bins; }
static inline size_t bins_set_words(const BinsState& s) { return bins_count_cells(s) + bins_sum_cells(s); }
static inline size_t bins_words(const BinsState& s) { return bins_set_words(s) * (size_t)(s.blocks ? s.blocks : 1); }      // of all sets
static inline void bins_release(BinsState& s)
{
    (void)hipFree(s.d_words);
}

// Energy histograms per group (amc_ehist.hip): counts alone, tail = 3.
typedef BinsState EhistState;

// Moments per energy bin (amc_emom.hip; DESIGN.md section 3.17 "Moments per bin"): an accumulator of its own beside the energy
// histograms', tail = 4, with the columns and the bound in its form.
struct EmomState : BinsState {
    int mask = 0;                               // the columns kept (AMC_EMOM_*)
    double x_bound = 0.0;
    uint64_t n_snapshots = 0;                   // passes queued since the cells were last known to be zero: the capacity check's count (a
                                                // respacing taken on the device zeroes the cells without the host knowing: amc_energy_moments_fetch
                                                // brings the count back to what the rows hold)
};

// Convergence per group (amc_chainstats.hip): running sums per chain, both buffers allocated at their first
// use -- a handle that never accumulates has neither.  The accumulators stand exactly while observable != 0.
struct ChainStatsState {
    int observable = 0;                         // AMC_CORR_E / AMC_CORR_X the accumulators were begun with; 0: nothing accumulated
    uint64_t n[2] = {0, 0};                     // samples each part holds
    double* d_sums = nullptr;                   // [2 parts][S, Q][M] (amc_chainstats.h)
    amc::xs_word* d_stat_rows = nullptr;        // [AMC_MAX_RUNGS][CS_COLS][XS_ROW_R] the rows of the last fetch (chain_stats_finish_kernel)
};
static inline void chain_stats_release(ChainStatsState& s)
{
    (void)hipFree(s.d_sums);
    (void)hipFree(s.d_stat_rows);
}

struct amc_handle {
    AmcKnobs knobs;             // the environment's knobs as amc_create found them
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t M = 0, M_pad = 0, offset = 0, M_global = 0;
    int potential = 0, K = 1, sweepstep = 1;
    bool counters = false;      // per-chain counters kept
    bool beta_arr = false;
    double beta = 1.0;
    uint64_t seed = 0;
    uint64_t t = 0;             // MH steps done (Philox step index)
    uint64_t t_counted = 0;     // MH steps counted in acc/tot since creation
    uint64_t t_est = 0;         // estimator calls done
    LadderState lad;            // the temperature ladder and what hangs on it (amc_exchange.hip)
    AnnealState ann;            // population annealing (amc_anneal.hip)
    CorrState corr;             // time correlation (amc_corr.hip)
    EhistState ehist;           // energy histograms per group (amc_ehist.hip)
    EmomState emom;             // moments per energy bin (amc_emom.hip)
    ChainStatsState cstat;      // running sums per chain for the convergence diagnostics (amc_chainstats.hip)
    BlocksState blocks;         // jackknife blocks of the bridge sums and the time correlation (amc_exchange.hip, amc_corr.hip)
    double* d_x = nullptr;
    double* d_beta = nullptr;
    uint32_t* d_acc = nullptr;
    uint32_t* d_tot = nullptr;
    // K <= 4 handles (narrow == true) keep the counters as two u16 planes instead: low halves here, high halves in *_hi;
    // the high planes stay all zero, and untouched by the folds, until counter_room() sets use_high before the call that
    // would count step 65 536 (fold_log_kernel<.., HIGH>).  Exactly one of the two forms is allocated.
    uint16_t* d_acc16 = nullptr;
    uint16_t* d_tot16 = nullptr;
    uint16_t* d_acc_hi = nullptr;
    uint16_t* d_tot_hi = nullptr;
    bool narrow = false;
    bool use_high = false;
    // Counts beyond 32 bits (counter_rebase): what the arrays above have been carried into, nullptr until the first carry --
    // [K][M_pad] / [K - 1][M_pad] 64-bit integers --, the steps counted with them, and their pool totals (host side)
    unsigned long long* d_acc_base = nullptr;
    unsigned long long* d_tot_base = nullptr;
    uint64_t t_base = 0;
    unsigned long long base_acc_total[AMC_MAX_MOVES] = {0}, base_tot_total[AMC_MAX_MOVES] = {0};
    uint8_t* d_log = nullptr;   // [log_depth][M_pad / 2 or M_pad] step log: (move << 1) | accepted per chain and MH step (log_form)
    int log_depth = 32;         // rows of the step log: 2 GiB worth, between 16 and 128 (AMC_LOG_DEPTH, 1..255: the fold counts rows in bytes)
    int log_fill = 0;           // rows written since the last fold into d_acc / d_tot
    double* d_ptab = nullptr;
    uint8_t* d_pick = nullptr;  // [AMC_PICK_CELLS] move pick by the 12 leading bits of the pick uniform (K > 1)
    unsigned long long* d_totals = nullptr;   // [2*K]: accepted, total (K > 1, filled on demand)
    unsigned long long* d_acc_slots = nullptr; // [max grid]: per-block accepted counts (K == 1)
    int n_slots = 0;
    amc::xs_word* d_partials = nullptr;   // [groups][nl * 4][PG_GROUP][words per column]: block rows of the estimator's fold
    RedTicket red[RED_TICKETS];      // reductions in flight, oldest first from red_head
    int red_head = 0, red_count = 0;
    double* d_out = nullptr;    // records of the estimator's fold: [comm ranks][PG_MAX_COLS][XS_WORDS]
    int d_out_ranks = 1;
    double* h_pg_out = nullptr; // pinned: records of amc_pg_estimate
    int red_blocks = 0;
    int red_cols = amc::RED_WANT_ALL;   // the callback sums a reduction forms (amc_set_reduce_columns)
    int n_cu = 256;
    int blocks_per_cu = 8;      // grid cap = n_cu * blocks_per_cu blocks of 256, grid-stride beyond
    int blocks_per_cu_single = 8;   // ... of single-step sweep launches (6 for the K = 1 pool-wide-counter form)
    int blocks_per_cu_red = 5;      // ... of the sweep launch that also forms the callback sums (AMC_BLOCKS_PER_CU_REDUCE)
    int blocks_per_cu_pg = 0;       // ... of the estimator kernels when AMC_BLOCKS_PER_CU is given; 0: what a CU HOLDS of the kernel form at hand
                                    // (hipOccupancyMaxActiveBlocksPerMultiprocessor: 5 for the built-in forms, 4 for most hiprtc ones), see pg_plan
    int occ_query = 0;              // out-slot of a launch_pg call made with grid < 0 (a query, nothing is launched)
    std::map<int, int> pg_resident; // resident blocks per CU of the estimator kernel forms, by (nl, sweep, reduce)
    std::map<int, std::string> class_form_errors;  // pools of several classes: the several-move estimator forms (nl, sweep, reduce) that do NOT build, with
                                                   // the compiler's last words about each (amc_pg.hip class_general_route, amc_pg_route)
    std::string class_form_error;   // ... of the form the last class_general_route call asked about ("" when it builds)
    // Single-sweep launches in slices (amc_sweeps.hip sweep_launches_sliced): slice 0 runs on `stream`, the others on streams of
    // the handle's own, made at the first sliced call; forked and joined with events once per call
    // (defaults by the ladder of profiles/sliced_launches_ab.md: two slices of 3 blocks per CU each, 25.6 against 28.4 us per step at 1e7
    // chains; the smallest size of the ladder at which slices are not slower)
    int sweep_slices = 2;                // S: slices of a single-sweep launch (1: whole launches; set back to 1 for good when a stream cannot be made)
    int slice_blocks_per_cu = 3;         // blocks per CU of each slice's launch
    int64_t slice_min_chains = 2500000;  // shards below it keep whole launches
    hipStream_t slice_stream[amc::AMC_MAX_SLICES - 1] = {nullptr, nullptr};
    hipEvent_t slice_fork = nullptr, slice_join[amc::AMC_MAX_SLICES - 1] = {nullptr, nullptr};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    unsigned long long* d_hist = nullptr;   // running histogram of amc_histogram_accumulate: [hist_bins + 3]
    int hist_bins = 0;
    double hist_lo = 0.0, hist_hi = 0.0;
    hipEvent_t ev_params = nullptr;   // behind the copy queued by amc_parameters_begin
    double* h_params = nullptr;       // pinned [AMC_MAX_NP][AMC_MAX_MOVES]: its destination (row p: parameter p of every move)
    bool params_pending = false;
    bool ev1_marked = false;    // amc_timing_mark recorded the end event already
    void* comm = nullptr;
    int comm_rank = 0, comm_ranks = 1;   // this shard's slot in record gathers (amc_comm_init's arguments)
    int comm_capacity = 0;               // doubles d_comm / h_comm hold
    double* d_comm = nullptr;
    double* h_comm = nullptr;            // pinned staging of amc_allreduce_sum's values (the caller's buffer is pageable)
    hipStream_t comm_stream = nullptr;   // amc_allreduce_sum's own stream: host-side sums must not wait for the queued sweeps
    hipEvent_t ev_comm_main = nullptr;   // behind the last collective queued on the engine's stream (the estimator's all-reduce)
    bool comm_main_pending = false;      // ... which comm_stream has not been ordered behind yet
    double* d_gd_acc = nullptr;   // [AMC_MAX_MOVES][5] running GradientData per move (device-resident estimator); n_params > 1:
                                  // [AMC_MAX_MOVES][AMC_GD_STRIDE_MAX], fields as in amc::pg_np_unpack
    int* d_status = nullptr;      // [1] sticky flag: a learning step was rejected
    uint32_t* d_pg_tickets = nullptr;   // [1 + groups] arrival counters of the estimator kernel's in-kernel final reduce
    amc::xs_word* d_pg_groups = nullptr;   // [nl * 4][PG_GROUP][words per column]: group rows
    double* d_theta_ring = nullptr;     // [2][AMC_MAX_LEARN]: sigma of the learnable moves as the fused launches of even / odd estimator steps used it
    // A learning step a fused time step left to the next launch's prologue (amc::pg_apply_pending): what it needs to be taken --
    // by that launch, or by pg_resolve_kernel when anything else wants the parameter table first
    struct {
        bool active = false;
        int source = 0;                 // amc::PG_PENDING_GROUPS / _RECORDS
        int groups = 0;                 // groups of PG_GROUP blocks the launch wrote
        int n_learn = 0;
        uint64_t t_est = 0;             // the estimator step of that launch (its parity names the ring slot and the group rows)
    } pend;
    bool pend_consumed = false;         // the last estimator launch took the pending step in its prologue (pg_launch)
    uint64_t gd_nonzero = 0;            // moves whose gradients_data on the device may be non-zero (estimator steps since their last update)
    amc::PgTail* d_pg_tail = nullptr;   // the estimator kernel's per-configuration record (see amc::PgTail)
    amc::PgTail pg_tail_host;           // ... and what it holds now (rewritten only when it changes)
    bool pg_tail_valid = false;
    Rccl rccl;
    std::string arch = AMC_BUILD_ARCH;   // the device's ISA name (gcnArchName up to its first ':'): what hiprtc compiles for
    ModelSpec model;              // what the run-time compiler builds this handle's kernels from; the fields below are derived from it
    bool f32 = false;             // state_dtype == AMC_DTYPE_F32: d_x / d_beta hold floats
    bool param_f32 = false;       // param_dtype == AMC_DTYPE_F32 (needs f32): sigma, the normal variate, delta = sigma z and the quotient of
                                  // log_proposal_density are Float32 (kernels built with AMC_PARAM_F32); sweeps with the built-in policy only
    bool scaled_policy = false;   // the proposal width is sigma * scale(x) (amc_create_policy_model)
    bool script_policy = false;   // sample_action! / log_proposal_density are script-defined expressions (amc_create_proposal_model)
    bool script_dlogq = false;    // ... and so is d logq / d sigma: the estimator is available
    int n_params = 1;             // parameters of the moves' policy (amc_create_policy_model; 1: sigma)
    int n_classes = 1;            // policy / action classes of the pool (amc_create_mixed_model)
    int class_of_move[AMC_MAX_MOVES] = {0};
    bool use_rtc = false;         // custom potential or Float32 state: every kernel that touches x is compiled at run time
    double* d_x64 = nullptr;      // f32 only: [M_pad] doubles, staging for uploads / downloads / host-side readers
    std::map<std::string, hipFunction_t> rtc_fn;   // kernel instantiation -> function of a module loaded on `device`
    std::vector<hipModule_t> rtc_mods;
};

// What an entry needs of the handle's state before it does anything: a refusal with the entry's name, through AMC_TRY.  Tracking is on
// exactly while d_lab is allocated, the families exactly while d_fam is.
static inline int need_ladder(const amc_handle* h, const char* who)
{
    return h->lad.n_rungs ? AMC_OK : fail(AMC_ERR_STATE, "%s: the handle has no ladder (amc_set_ladder)", who);
}
static inline int need_tracking(const amc_handle* h, const char* who)
{
    return h->lad.d_lab ? AMC_OK : fail(AMC_ERR_STATE, "%s: tracking is off (amc_set_tracking)", who);
}
static inline int need_families(const amc_handle* h, const char* who)
{
    return h->ann.d_fam ? AMC_OK : fail(AMC_ERR_STATE, "%s: families are off (amc_set_anneal_families)", who);
}

// The chains have changed slots (an upload, a new initial ensemble, another ladder, a resampling): a product of the origin values with
// what the slots hold now has no meaning, so the mark of the time correlation goes.  Host fields only; the memory stays.
static inline void corr_forget(amc_handle* h)
{
    h->corr.observable = 0;
    h->corr.n_samples = 0;
    h->corr.groups = 0;
}

// ... and so go the running sums per chain of the convergence diagnostics (an upload, a new initial ensemble, another ladder; NOT a
// resampling, an annealing step or a respacing: the caller clears when beta moves).  Host fields only; the
// memory stays and is zeroed by the next first sample.
static inline void chain_stats_forget(amc_handle* h)
{
    h->cstat.observable = 0;
    h->cstat.n[0] = h->cstat.n[1] = 0;
}

// ---- shared between the translation units ----------------------------------------------------------------------------------------
AMC_INTERNAL int grid_for(const amc_handle* h, int64_t n_items, int blocks_per_cu = 0);   // amc_api.hip
AMC_INTERNAL hipError_t wait_stream(hipStream_t stream);                                  // amc_state.hip
AMC_INTERNAL hipError_t wait_event(hipEvent_t ev);
// A few words copied on the handle's stream, then hipStreamSynchronize: the caller's buffer is only valid during the call (to the device)
// or is read right after it (to the host).  A null d_src copies nothing and still waits: the caller's zeroed words stand for a buffer
// that was never allocated.  (The runtime's blocking wait, as these entries always used, not wait_stream's spin.)
AMC_INTERNAL int copy_to_host_sync(amc_handle* h, void* dst, const void* d_src, size_t bytes);
AMC_INTERNAL int copy_to_device_sync(amc_handle* h, void* d_dst, const void* src, size_t bytes);
// *p allocated at its first use and zeroed on the stream then; nothing when it exists
AMC_INTERNAL int zeroed_words(amc_handle* h, unsigned long long** p, size_t bytes);
AMC_INTERNAL bool hist_args_ok(const char* who, double lo, double hi, int n_bins);         // what every histogram entry asks of its bins
AMC_INTERNAL int hist_grid(const amc_handle* h);                                          // the grid of every histogram pass
AMC_INTERNAL int log_form(const amc_handle* h);                                           // amc_counters.hip
AMC_INTERNAL int log_room(amc_handle* h, int* rows);
AMC_INTERNAL int fold_log(amc_handle* h, bool with_ratio = false, int* ratio_rows = nullptr, amc::xs_word* ratio_dst = nullptr);
AMC_INTERNAL hipError_t alloc_counters(amc_handle* h, bool narrow);
AMC_INTERNAL int counter_room(amc_handle* h, const char* who, uint64_t steps);
AMC_INTERNAL int rung_totals_queue(amc_handle* h);      // the totals per (move, rung) into d_rung_cnt, nothing read back
AMC_INTERNAL amc::SweepArgs make_sweep_args(const amc_handle* h, int32_t n_steps, int grid);        // amc_sweeps.hip
AMC_INTERNAL int reduce_sweep_grid(const amc_handle* h);
AMC_INTERNAL int sweep_impl(amc_handle* h, int64_t n_sweeps, bool fuse_reduce, int* grid_out);
AMC_INTERNAL int red_form(const amc_handle* h);                                           // amc_reduce.hip
AMC_INTERNAL int red_row_stride(const amc_handle* h, int grid);
AMC_INTERNAL RedTicket* red_next(amc_handle* h);
AMC_INTERNAL int finish_fused_reduce(amc_handle* h, int grid);
AMC_INTERNAL bool reduce_fits_in_grid(const amc_handle* h, int grid);
AMC_INTERNAL int push_params(amc_handle* h, const double* sigma, const double* weight);  // amc_parameters.hip
AMC_INTERNAL int check_sigma_f32(const char* who, int k, double s);     // a sigma of a param_dtype = AMC_DTYPE_F32 handle
// The policy-gradient estimator with Float32 parameters (Dual{Float32}) does not exist yet: its entries refuse such a handle
// before any launch and any compile.
#define AMC_REFUSE_PARAM_F32(h, who)                                                                                        \
    do {                                                                                                                    \
        if ((h)->param_f32)                                                                                                 \
            return fail(AMC_ERR_STATE, "%s: not available with param_dtype = AMC_DTYPE_F32 (Float32 policy parameters: sweeps only)", (who)); \
    } while (0)
// ... and it learns one sigma per move: while a table of widths per rung is set (amc_set_rung_sigma) its entries refuse the handle too.
#define AMC_REFUSE_RUNG_SIGMA(h, who)                                                                                       \
    do {                                                                                                                    \
        if ((h)->lad.rung_on)                                                                                               \
            return fail(AMC_ERR_STATE, "%s: not available while widths per rung are set (amc_set_rung_sigma): the estimator learns one sigma per move", (who)); \
    } while (0)
AMC_INTERNAL int pg_resolve(amc_handle* h);      // takes a pending learning step now (amc_pg.hip)
// A pass over the groups of chains -- the rungs of the ladder; ONE group of all local chains without a ladder -- that ends every block
// with rows of its own, n_cols columns per group, in lad.d_rung_rows (the rung sums, the bridge sums, the time correlation): the
// launches it takes and where each one's rows go (amc_exchange.hip).  A BLOCKED pass (the caller's choice, under a partition:
// amc_set_blocks) takes the traversal of amc_blocks.h -- a grid that is a multiple of B, HIP block k serving jackknife block k mod B,
// launches split by ladder ranges that keep every lane within XS_LANE_CAP - 2 summands -- and its kernels the partition as their
// second argument.
static inline int pass_groups(const amc_handle* h) { return h->lad.n_rungs ? h->lad.n_rungs : 1; }
struct RungPass {
    int grid = 0;
    int groups = 1;                             // G: R of the ladder, 1 without one (a "ladder" of the pass is then a single chain)
    bool blocked = false;
    int64_t per_launch = 0, n_launches = 0;     // ladders per launch; launches
    size_t slot_words = 0;                      // words of one block's rows
    int n_blocks() const { return (int)(n_launches * grid); }      // block rows the finishing kernel reads
};
AMC_INTERNAL int rung_pass_plan(amc_handle* h, int n_cols, bool blocked, RungPass* p);      // ... planned, and room made for its rows
AMC_INTERNAL int rung_pass_grid(const amc_handle* h);      // the grid of an unblocked pass: what a memory-bound pass over the chains takes
// a kind-R record into words 0 .. 4 of an XS_ROW_R row, or a refusal naming who / where (amc_exchange.hip; amc_set_bridge*, amc_set_corr*)
AMC_INTERNAL int r_row_from_record(const char* who, const char* where, const double* rec, amc::xs_word* row);
AMC_INTERNAL void comm_release(amc_handle* h);   // drops the handle's communicator and its buffers (amc_comm.hip)
// kernels compiled at run time (amc_rtc.hip)
struct RtcCode { std::vector<char> code; std::string lowered; };
AMC_INTERNAL int validate_potential_expr(const char* expr, const char* what = "custom potential", const char* var = "x");
AMC_INTERNAL int rtc_compile(const ModelSpec& spec, const std::string& inst, const std::string& arch, const AmcKnobs& knobs, const RtcCode** out,
                             std::string* log_out);
AMC_INTERNAL int rtc_function(amc_handle* h, const std::string& inst, hipFunction_t* fn);
AMC_INTERNAL int rtc_launch(amc_handle* h, const std::string& inst, int grid, void** params);

// One launch of a kernel whose only template argument is the potential: the instantiation name<potential> compiled at run time
// (use_rtc), or the offline one of the built-in potential at hand.  AMC_BLOCK threads, no dynamic LDS, the handle's stream; params
// as hipLaunchKernel takes them.
static inline int launch_by_potential(amc_handle* h, const char* name, const void* double_well, const void* harmonic, int grid, void** params)
{
    if (h->use_rtc) return rtc_launch(h, std::string(name) + "<" + std::to_string(h->potential) + ">", grid, params);
    (void)hipLaunchKernel(h->potential == AMC_POTENTIAL_DOUBLE_WELL ? double_well : harmonic, dim3(grid), dim3(AMC_BLOCK), params, 0, h->stream);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

static inline amc::blk::Part blocks_part(const amc_handle* h)
{
    amc::blk::Part part = {};
    part.l_first = h->offset / pass_groups(h);
    part.chunk = h->blocks.chunk;
    part.n_blocks = h->blocks.n_blocks;
    return part;
}
// A planned pass launched: `a` comes with what only its kernel reads (the bridge sums' beta, the origin of the time correlation); x, the
// rows, the ladders, G and the columns are filled in here, and behind `a` the partition when the pass is blocked.
// (rung_pass_each: the launches of the plan one by one -- G, each launch's rows and ladders filled in, then launch(a); the sums of the
// chain statistics, whose kernel has no potential to be launched by, take it directly)
template <class Args, class Launch>
static inline int rung_pass_each(amc_handle* h, const RungPass& p, Args a, Launch launch)
{
    const int64_t n_ladders = h->M / p.groups;
    a.n_rungs = p.groups;
    for (int64_t i = 0; i < p.n_launches; ++i) {
        a.rows = h->lad.d_rung_rows + (size_t)i * (size_t)p.grid * p.slot_words;
        a.l_begin = i * p.per_launch;
        a.l_end = std::min(n_ladders, (i + 1) * p.per_launch);
        AMC_TRY(launch(a));
    }
    return AMC_OK;
}
template <class Args>
static inline int rung_pass_launch(amc_handle* h, const RungPass& p, Args a, int columns, const char* name, const void* double_well, const void* harmonic)
{
    amc::blk::Part part = blocks_part(h);
    a.x = h->d_x;
    a.cols = columns;
    return rung_pass_each(h, p, a, [&](Args& one) {
        void* params[] = {&one, p.blocked ? &part : nullptr};      // (a kernel reads as many as it has arguments)
        return launch_by_potential(h, name, double_well, harmonic, p.grid, params);
    });
}

// *p holds exactly `need` words, zeroed on the stream when it is (re)allocated: the blocked accumulators follow B and G at their first use
static inline int blocks_words(amc_handle* h, amc::xs_word** p, size_t* have, size_t need)
{
    if (*p && *have == need) return AMC_OK;
    AMC_HIP(hipStreamSynchronize(h->stream));
    (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    AMC_HIP(hipMalloc(p, need * sizeof(amc::xs_word)));
    *have = need;
    AMC_HIP(hipMemsetAsync(*p, 0, need * sizeof(amc::xs_word), h->stream));
    return AMC_OK;
}

// The life cycle of an accumulator over the energy bins, for the histograms' and the moments' alike (S: EhistState or EmomState).
// The accumulator gone, no form fixed: the default state.  hipFree waits for whatever still writes the memory.
template <class S>
static inline int bins_clear(S& s)
{
    (void)hipFree(s.d_words);
    s = S();
    return AMC_OK;
}
// Begun at its first use: room for the sets of `form`; with `zeroed`, cleared on the stream -- behind everything queued when it is
// blocked, as the other blocked accumulators wait where they allocate (blocks_words).  Otherwise the caller fills it.  A failure
// leaves nothing behind.
template <class S>
static inline int bins_begin(amc_handle* h, S& s, const S& form, const char* who, bool zeroed)
{
    if (zeroed && form.blocks) AMC_HIP(hipStreamSynchronize(h->stream));
    unsigned long long* d = nullptr;
    AMC_HIP(hipMalloc(&d, bins_words(form) * sizeof(unsigned long long)));
    s = form;
    s.d_words = d;
    if (zeroed && hipMemsetAsync(d, 0, bins_words(s) * sizeof(unsigned long long), h->stream) != hipSuccess) {
        (void)bins_clear(s);
        return fail(AMC_ERR_HIP, "%s: clearing the accumulator failed", who);
    }
    return AMC_OK;
}
// One pass launched; a first call that is refused (a run-time build that fails, say) leaves no accumulator and no form behind.
template <class S>
static inline int bins_pass(amc_handle* h, S& s, bool first, const char* name, const void* double_well, const void* harmonic, int grid, void** params)
{
    const int rc = launch_by_potential(h, name, double_well, harmonic, grid, params);
    if (rc != AMC_OK && first) (void)bins_clear(s);
    return rc;
}
// amc_ehist.hip, for both accumulators.  The words zeroed on the stream when the respacing just queued is taken (amc_respace_ladder); a
// blocked accumulator folded into a plain one on the stream (amc_set_blocks); nothing happens without one.  Then what the entries check
// and what the fetches form on the host (see there).
AMC_INTERNAL int bins_respaced(amc_handle* h, const BinsState& s);
AMC_INTERNAL int bins_fold(amc_handle* h, BinsState& s);
AMC_INTERNAL int bins_partition(const amc_handle* h, const char* who, bool families, int* n_blocks, bool* by_family);
AMC_INTERNAL int bins_u32_ok(const amc_handle* h, const char* who, int grid);
AMC_INTERNAL int bins_u32_blocked_ok(const amc_handle* h, const char* who, int n_blocks, int* grid);
AMC_INTERNAL int bins_row_sum(const char* who, const char* what, const uint64_t* row, size_t n, uint64_t want, int g, int s);
AMC_INTERNAL int bins_merge_blocks(amc_handle* h, const BinsState& s, uint64_t* set);
AMC_INTERNAL uint64_t bins_snapshots(const amc_handle* h, const BinsState& s, const uint64_t* counts, bool blocked);
// (what amc_set_ladder, amc_set_blocks, amc_set_anneal_blocks and amc_respace_ladder call)
static inline int ehist_clear(amc_handle* h) { return bins_clear(h->ehist); }
static inline int ehist_respaced(amc_handle* h) { return bins_respaced(h, h->ehist); }
static inline int ehist_fold(amc_handle* h) { return bins_fold(h, h->ehist); }
static inline int emom_clear(amc_handle* h) { return bins_clear(h->emom); }
static inline int emom_respaced(amc_handle* h) { return bins_respaced(h, h->emom); }
static inline int emom_fold(amc_handle* h) { return bins_fold(h, h->emom); }
