// amc_exchange.hip -- replica exchange along a temperature ladder: the ladder of a handle, exchange steps
// (amc_exchange, amc_sweep_exchange), the per-gap counters and the exchange step index, the per-rung reproducible sums
// (amc_reduce_rungs_exact), the bridge sums (amc_bridge_accumulate .. amc_set_bridge), walker tracking (amc_set_tracking .. amc_set_tracking_counters), proposal widths per rung
// (amc_set_rung_sigma, amc_get_rung_sigma), respacing the ladder (amc_respace_ladder .. amc_get_ladder), tuning the widths per rung
// (amc_tune_rung_sigma .. amc_set_tuned) and the window of the acceptance per rung (amc_rung_window_*).  amc_histogram_rungs is with the other
// histograms in amc_state.hip.
#define AMC_KERNEL_LINKAGE static      // template instantiations, and this object's own copies of the plain kernels it launches (rung_finish_kernel, bridge_finish_kernel, rung_flow_kernel)
#include "amc_internal.h"

// AMC_MAX_RUNGS has two definitions, include/amc.h's (the ABI) and amc_exchange.h's (the kernel sources, which the run-time compiler
// builds without amc.h); the kernel's LDS counters and the layout of d_xcnt need them equal.  This unit sees both: a later definition
// with another value is a redefinition error, and the value the kernel was written for is pinned here.
static_assert(AMC_MAX_RUNGS == 64 && sizeof(((amc::ExchangeArgs*)nullptr)->counts[0]) == 8, "AMC_MAX_RUNGS of include/amc.h and amc_exchange.h");

// Every block ends with one 64-bit atomic per touched gap on the SAME few addresses, and those serialise (~13 ns each per address,
// amc_state.hip hist_grid): with the sweeps' 8 blocks per CU that tail is as long as the pass over the chains.  10^7 chains, R = 8, even /
// odd step: 48.4 / 47.7 us with 8 blocks per CU, 42.4 / 45.8 with 4, 38.7 / 43.1 with 2 (profiles/exchange.md).  AMC_BLOCKS_PER_CU overrides.
static const int EXCHANGE_BLOCKS_PER_CU = 2;

// The rung sums end every block with its rows, R x 3 x 48 bytes of them, and rung_finish_kernel reads them all again: with the sweeps' 8
// blocks per CU and R = 64 that is a quarter of the pass's own traffic.  Four loads in flight per lane keep the memory system busy
// with fewer blocks.  AMC_BLOCKS_PER_CU overrides.
static const int RUNG_SUMS_BLOCKS_PER_CU = 4;

static const size_t XCNT_BYTES = 2 * AMC_MAX_RUNGS * sizeof(unsigned long long);   // d_xcnt: attempted[AMC_MAX_RUNGS], accepted[AMC_MAX_RUNGS]

// d_track: round_trips, up_trips, then the cells of one flow snapshot (amc_flow_rungs' scratch)
static const int TRACK_FLOW_CELLS = 3 * AMC_MAX_RUNGS;
static const size_t TRACK_BYTES = (2 + TRACK_FLOW_CELLS) * sizeof(unsigned long long);

static const size_t RESPACE_BYTES = amc::RESPACE_WORDS * sizeof(unsigned long long);   // d_respace (amc_exchange.h RESPACE_*)
static const size_t TUNE_BYTES = amc::TUNE_WORDS * sizeof(unsigned long long);            // d_tune (amc_exchange.h TUNE_*)
static const size_t RUNG_BASE_BYTES = amc::RUNG_BASE_WORDS * sizeof(unsigned long long);  // d_rung_base
static_assert(AMC_RESPACE_ACCEPTANCE == amc::rs::RS_ACCEPTANCE && AMC_RESPACE_FLOW == amc::rs::RS_FLOW, "the rules of include/amc.h and amc_respace.h");

// The record of the tunings back to "never tuned"; with_base: the window base too (zero: the window is "since the counters began").
// Memory a handle never allocated stays unallocated.
static int tune_reset(amc_handle* h, bool with_base)
{
    if (h->lad.d_tune) AMC_HIP(hipMemsetAsync(h->lad.d_tune, 0, TUNE_BYTES, h->stream));
    if (with_base && h->lad.d_rung_base) AMC_HIP(hipMemsetAsync(h->lad.d_rung_base, 0, RUNG_BASE_BYTES, h->stream));
    h->lad.tune_queued = false;
    return AMC_OK;
}

// Tracking off: the labels and the trip counters go.  Launches queued on the stream may still use them.
static int tracking_off(amc_handle* h)
{
    if (!h->lad.d_lab) return AMC_OK;
    AMC_HIP(hipStreamSynchronize(h->stream));
    (void)hipFree(h->lad.d_lab);
    (void)hipFree(h->lad.d_track);
    h->lad.d_lab = nullptr;
    h->lad.d_track = nullptr;
    return AMC_OK;
}

// d_rung_rows holds at least `need` words: the block rows of the rung sums and of the bridge sums (each call's finishing kernel has
// read them, in stream order, before the next call's launches write them).
static int rung_rows_room(amc_handle* h, size_t need)
{
    if (need <= h->lad.rung_rows_words) return AMC_OK;
    AMC_HIP(hipStreamSynchronize(h->stream));                   // (a finishing kernel queued by a bridge snapshot may still read the old rows)
    (void)hipFree(h->lad.d_rung_rows);
    h->lad.d_rung_rows = nullptr;
    h->lad.rung_rows_words = 0;
    AMC_HIP(hipMalloc(&h->lad.d_rung_rows, need * sizeof(amc::xs_word)));
    h->lad.rung_rows_words = need;
    return AMC_OK;
}

// The accumulator of the bridge sums back to "nothing accumulated", the mask free again.  Memory a handle never allocated stays unallocated.
static const size_t BRIDGE_BYTES = amc::BRIDGE_WORDS * sizeof(amc::xs_word);      // d_bridge (amc_exchange.h BRIDGE_*)
static int bridge_clear(amc_handle* h)
{
    if (h->lad.d_bridge) AMC_HIP(hipMemsetAsync(h->lad.d_bridge, 0, BRIDGE_BYTES, h->stream));
    if (h->blocks.d_bridge_blk) AMC_HIP(hipMemsetAsync(h->blocks.d_bridge_blk, 0, h->blocks.bridge_blk_words * sizeof(amc::xs_word), h->stream));
    h->lad.bridge_cols = 0;
    return AMC_OK;
}

// Another ladder, or none: everything the handle knew about the old one is forgotten -- its walkers, that it was respaced, the tunings of
// its widths and the window (another R has other cells), its bridge sums, its widths per rung (none until they are set again).  Memory
// stays, but for the labels.  The one place a feature that adds ladder state has to remember.
static int ladder_reset(amc_handle* h)
{
    AMC_TRY(tracking_off(h));
    if (h->lad.d_respace) AMC_HIP(hipMemsetAsync(h->lad.d_respace, 0, RESPACE_BYTES, h->stream));
    AMC_TRY(tune_reset(h, true));
    AMC_TRY(bridge_clear(h));
    AMC_TRY(ehist_clear(h));        // (the energy histograms' groups are the rungs)
    AMC_TRY(emom_clear(h));         // (... and the moments per bin's)
    corr_forget(h);                 // (no ladder state, but its groups are the rungs: the chains' slots mean something else now)
    chain_stats_forget(h);          // (likewise the running sums per chain)
    h->blocks.n_blocks = 0;         // (the jackknife partition counts ladders: another R has other ladders)
    h->blocks.chunk = 0;
    h->lad.rung_on = false;
    return AMC_OK;
}

// The flow snapshot of this handle's labels queued into the cells behind the trip counters (tracking is on: the caller has checked).
static int flow_snapshot_queue(amc_handle* h)
{
    unsigned long long* d_flow = h->lad.d_track + 2;
    AMC_HIP(hipMemsetAsync(d_flow, 0, (size_t)(3 * h->lad.n_rungs) * sizeof(unsigned long long), h->stream));
    const int grid = grid_for(h, (h->M + 3) / 4, h->knobs.blocks_per_cu ? 0 : EXCHANGE_BLOCKS_PER_CU);     // a thread per 4 labels; the atomics' tail again
    hipLaunchKernelGGL(amc::rung_flow_kernel, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, (const uint8_t*)h->lad.d_lab, h->M, h->lad.n_rungs, d_flow);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

// A pass over the groups (RungPass, amc_internal.h) planned, and room made for its rows.  Blocked: the same grid rounded up to a
// multiple of B, and the ladders per launch by the traversal's own bound.
int rung_pass_grid(const amc_handle* h) { return grid_for(h, h->M, h->knobs.blocks_per_cu ? 0 : RUNG_SUMS_BLOCKS_PER_CU); }

int rung_pass_plan(amc_handle* h, int n_cols, bool blocked, RungPass* p)
{
    const int R = pass_groups(h);
    p->groups = R;
    p->blocked = blocked;
    p->grid = rung_pass_grid(h);
    if (blocked) p->grid = amc::blk::grid_round(p->grid, h->blocks.n_blocks);
    // a lane adds one summand per trip and column and holds XS_LANE_CAP of them (amc_xsum.h): ensembles beyond that many trips of the
    // grid (2^28 chains and more) take several launches, each with block rows of its own
    const int64_t cap = amc::xs::XS_LANE_CAP - 2;
    p->per_launch = blocked ? amc::blk::ladders_per_launch(h->M / R, h->blocks.n_blocks, h->blocks.chunk, R, p->grid, AMC_BLOCK, cap)
                            : (((int64_t)p->grid * AMC_BLOCK) / R) * cap;
    p->n_launches = (h->M / R + p->per_launch - 1) / p->per_launch;
    p->slot_words = (size_t)R * (size_t)n_cols * amc::XS_ROW_R;
    return rung_rows_room(h, (size_t)p->n_launches * (size_t)p->grid * p->slot_words);
}

// A kind-R record, as a fetch gives it, into words 0 .. 4 of a row of XS_ROW_R words (word 5 is the caller's): the kind, an integer
// level within the levels, an integer flag word within the flags, integers below 2^53.  Anything else is refused, named by who / where.
int r_row_from_record(const char* who, const char* where, const double* rec, amc::xs_word* row)
{
    if (rec[0] != (double)amc::xs::XS_R || !(rec[1] >= amc::xs::XS_LMIN && rec[1] <= amc::xs::XS_LMAX) || rec[1] != std::floor(rec[1]) ||
        !(rec[2] >= 0.0 && rec[2] <= 7.0) || rec[2] != std::floor(rec[2]))
        return fail(AMC_ERR_BAD_ARG, "%s: record of %s is no kind-R record", who, where);
    for (int i = 3; i < amc::xs::XS_WORDS; ++i)
        if (!(std::fabs(rec[i]) < 9007199254740992.0) || rec[i] != std::floor(rec[i]))
            return fail(AMC_ERR_BAD_ARG, "%s: record of %s: word %d is no integer below 2^53", who, where, i);
    const amc::xs::PartR p = amc::xs::rec_to_r(rec);
    row[0] = (amc::xs_word)(uint32_t)p.top | ((amc::xs_word)p.flags << 32);
    row[1] = (amc::xs_word)p.k1.lo; row[2] = (amc::xs_word)p.k1.hi;
    row[3] = (amc::xs_word)p.k2.lo; row[4] = (amc::xs_word)p.k2.hi;
    return AMC_OK;
}

// The blocked accumulator of the bridge sums on the host: the rows [b][r][c], then the number of snapshots (all zero while nothing has
// been accumulated since the partition was set).  Waits for the stream.
static int bridge_blocks_host(amc_handle* h, std::vector<amc::xs_word>* rows)
{
    const size_t words = (size_t)h->blocks.n_blocks * h->lad.n_rungs * amc::BR_COLS * amc::XS_ROW_R + 1;
    rows->assign(words, 0ull);
    const bool have = h->blocks.d_bridge_blk && h->blocks.bridge_blk_words == words;
    return copy_to_host_sync(h, rows->data(), have ? h->blocks.d_bridge_blk : nullptr, words * sizeof(amc::xs_word));
}

// One exchange step on the stream: the gaps r with r mod 2 == t_x mod 2 of every local ladder.  A parity without gaps (R = 2, odd
// steps) launches nothing and still counts as a step.
static int exchange_step(amc_handle* h)
{
    // (what a sweep does before it launches: a learning step left pending by a fused time step is taken now -- it belongs in front
    // of this point of the stream; reductions in flight were queued on the same stream and have read x before this launch writes it)
    AMC_TRY(pg_resolve(h));
    if (h->lad.t_x >> 48) return fail(AMC_ERR_STATE, "amc_exchange: the exchange step index has reached 2^48");
    const int parity = (int)(h->lad.t_x & 1u);
    const int n_gaps = (h->lad.n_rungs - parity) / 2;
    if (n_gaps > 0) {
        amc::ExchangeArgs a;
        a.x = h->d_x;
        a.beta = h->d_beta;
        a.counts = h->lad.d_xcnt;
        a.n_ladders = h->M / h->lad.n_rungs;
        a.chain0 = (uint64_t)h->offset;
        a.t_x = h->lad.t_x;
        a.n_rungs = h->lad.n_rungs;
        a.n_gaps = n_gaps;
        a.key0 = (uint32_t)h->seed;
        a.key1 = (uint32_t)(h->seed >> 32);
        const int grid = grid_for(h, a.n_ladders * n_gaps, h->knobs.blocks_per_cu ? 0 : EXCHANGE_BLOCKS_PER_CU);
        amc::ExchangeTrackArgs ta;        // tracking on: the same step by the kernel that carries the labels along
        ta.step = a;
        ta.lab = h->lad.d_lab;
        ta.trips = h->lad.d_track;
        const bool track = h->lad.d_lab != nullptr;
        void* params[] = {track ? (void*)&ta : (void*)&a};
        AMC_TRY(track ? launch_by_potential(h, "amc::exchange_tracked_kernel", (const void*)amc::exchange_tracked_kernel<amc::POT_DOUBLE_WELL>,
                                            (const void*)amc::exchange_tracked_kernel<amc::POT_HARMONIC>, grid, params)
                      : launch_by_potential(h, "amc::exchange_kernel", (const void*)amc::exchange_kernel<amc::POT_DOUBLE_WELL>,
                                            (const void*)amc::exchange_kernel<amc::POT_HARMONIC>, grid, params));
    }
    h->lad.t_x += 1;
    return AMC_OK;
}

extern "C" {

int amc_set_ladder(amc_handle* h, int n_rungs)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_ladder: NULL handle");
    if (n_rungs == 0) {
        AMC_HIP(hipSetDevice(h->device));
        AMC_TRY(ladder_reset(h));
        h->lad.n_rungs = 0;
        return AMC_OK;
    }
    if (n_rungs < 2 || n_rungs > AMC_MAX_RUNGS)
        return fail(AMC_ERR_BAD_ARG, "amc_set_ladder: n_rungs = %d must be 0 (no ladder) or in [2, %d]", n_rungs, AMC_MAX_RUNGS);
    if (!h->beta_arr)
        return fail(AMC_ERR_STATE, "amc_set_ladder: a ladder of %d rungs needs a per-chain beta array (amc_upload_state with beta)", n_rungs);
    if (h->M_global % n_rungs)
        return fail(AMC_ERR_BAD_ARG, "amc_set_ladder: n_chains_global = %lld is no multiple of n_rungs = %d", (long long)h->M_global, n_rungs);
    if (h->offset % n_rungs)
        return fail(AMC_ERR_BAD_ARG, "amc_set_ladder: chain_offset = %lld is no multiple of n_rungs = %d (no ladder may straddle a shard)",
                    (long long)h->offset, n_rungs);
    if (h->M % n_rungs)
        return fail(AMC_ERR_BAD_ARG, "amc_set_ladder: n_chains = %lld is no multiple of n_rungs = %d (no ladder may straddle a shard)",
                    (long long)h->M, n_rungs);
    AMC_HIP(hipSetDevice(h->device));
    if (!h->lad.d_xcnt) AMC_HIP(hipMalloc(&h->lad.d_xcnt, XCNT_BYTES));
    AMC_HIP(hipMemsetAsync(h->lad.d_xcnt, 0, XCNT_BYTES, h->stream));      // the gaps of another ladder are other gaps
    AMC_TRY(ladder_reset(h));                                              // ... and the rest of what was known about the old one goes
    h->lad.n_rungs = n_rungs;
    return AMC_OK;
}

// ---- proposal widths per rung (DESIGN.md section 3.13 "Widths per rung") --------------------------------------------------------------
int amc_set_rung_sigma(amc_handle* h, const double* sigma, int n)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_rung_sigma: NULL handle");
    if (!sigma || n == 0) {              // no table: the sweeps read the pool's sigma_k again
        // Host state only, so no hipSetDevice: the next sweep picks its form from this flag when it is queued, and the table's
        // memory stays for the sweeps already queued.  No pg_resolve either: every estimator entry is refused while a table is
        // set, and setting it took the step that was pending then, so none can be pending here.
        h->lad.rung_on = false;
        h->lad.tune_queued = false;          // (the record itself is zeroed when the next table is set)
        return AMC_OK;
    }
    if (!h->model.classes.empty() || h->script_policy || h->scaled_policy || h->n_params > 1 || h->n_classes > 1)
        return fail(AMC_ERR_STATE, "amc_set_rung_sigma: widths per rung belong to the built-in Gaussian policy; this handle has a script-defined policy, "
                                   "class or action");
    if (h->param_f32)
        return fail(AMC_ERR_STATE, "amc_set_rung_sigma: not available with param_dtype = AMC_DTYPE_F32 (the rung table holds Float64 widths)");
    AMC_TRY(need_ladder(h, "amc_set_rung_sigma"));
    if (!h->counters)
        return fail(AMC_ERR_STATE, "amc_set_rung_sigma: handle was created with per_chain_counters = 0 (the acceptance per rung needs them)");
    const int R = h->lad.n_rungs;
    if (h->K * R > AMC_MAX_MOVES)
        return fail(AMC_ERR_BAD_ARG, "amc_set_rung_sigma: %d moves x %d rungs = %d entries, the table holds %d", h->K, R, h->K * R, AMC_MAX_MOVES);
    if (n != h->K * R)
        return fail(AMC_ERR_BAD_ARG, "amc_set_rung_sigma: n = %d, the table of %d moves x %d rungs has %d entries", n, h->K, R, h->K * R);
    for (int e = 0; e < n; ++e)
        if (!(std::isfinite(sigma[e]) && sigma[e] >= 1e-100 && sigma[e] <= 1e100))
            return fail(AMC_ERR_BAD_ARG, "amc_set_rung_sigma: sigma[%d] (move %d, rung %d) = %g is not a finite value in [1e-100, 1e100]", e, e / R, e % R,
                        sigma[e]);
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of a sweep: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    if (!h->lad.d_rung_tab) AMC_HIP(hipMalloc(&h->lad.d_rung_tab, (size_t)amc::RT_ROWS * AMC_MAX_MOVES * sizeof(double)));
    amc::RungSigma s;
    for (int e = 0; e < AMC_MAX_MOVES; ++e) s.sigma[e] = e < n ? sigma[e] : 1.0;
    // on the stream, behind the sweeps that read the rows as they are
    hipLaunchKernelGGL(amc::prepare_rung_params_kernel, dim3(1), dim3(AMC_MAX_MOVES), 0, h->stream, h->lad.d_rung_tab, s, n);
    AMC_HIP(hipGetLastError());
    std::memcpy(h->lad.rung_sigma, s.sigma, sizeof(h->lad.rung_sigma));
    h->lad.rung_on = true;
    return tune_reset(h, false);         // a table that was given has not been tuned; the window is left alone
}

int amc_get_rung_sigma(amc_handle* h, double* sigma, int n)
{
    if (!h || !sigma) return fail(AMC_ERR_BAD_ARG, "amc_get_rung_sigma: NULL argument");
    if (!h->lad.rung_on) return fail(AMC_ERR_STATE, "amc_get_rung_sigma: no widths per rung are set (amc_set_rung_sigma)");
    if (n != h->K * h->lad.n_rungs)
        return fail(AMC_ERR_BAD_ARG, "amc_get_rung_sigma: n = %d, the table of %d moves x %d rungs has %d entries", n, h->K, h->lad.n_rungs, h->K * h->lad.n_rungs);
    if (!h->lad.tune_queued) {               // the table as it was given
        std::memcpy(sigma, h->lad.rung_sigma, (size_t)n * sizeof(double));
        return AMC_OK;
    }
    // tuned since: the table is the device's (the record holds every entry's width as the last tuning left it)
    AMC_HIP(hipSetDevice(h->device));
    unsigned long long host[AMC_MAX_MOVES];
    AMC_TRY(copy_to_host_sync(h, host, h->lad.d_tune + amc::TUNE_SIGMA, (size_t)n * sizeof(unsigned long long)));
    std::memcpy(sigma, host, (size_t)n * sizeof(double));
    return AMC_OK;
}

int amc_exchange(amc_handle* h, int64_t n_steps)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_exchange: NULL handle");
    AMC_TRY(need_ladder(h, "amc_exchange"));
    if (n_steps < 0) return fail(AMC_ERR_BAD_ARG, "amc_exchange: n_steps < 0");
    AMC_HIP(hipSetDevice(h->device));
    for (int64_t i = 0; i < n_steps; ++i) {
        AMC_TRY(exchange_step(h));
    }
    return AMC_OK;
}

int amc_sweep_exchange(amc_handle* h, int64_t n_rounds, int64_t sweeps_per_round)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_sweep_exchange: NULL handle");
    AMC_TRY(need_ladder(h, "amc_sweep_exchange"));
    if (n_rounds < 0 || sweeps_per_round < 0) return fail(AMC_ERR_BAD_ARG, "amc_sweep_exchange: n_rounds < 0 or sweeps_per_round < 0");
    AMC_HIP(hipSetDevice(h->device));
    for (int64_t i = 0; i < n_rounds; ++i) {
        if (sweeps_per_round > 0) {
            AMC_TRY(sweep_impl(h, sweeps_per_round, false, nullptr));
        }
        AMC_TRY(exchange_step(h));
    }
    return AMC_OK;
}

int amc_exchange_counters(amc_handle* h, int64_t* accepted, int64_t* attempted)
{
    if (!h || !accepted || !attempted) return fail(AMC_ERR_BAD_ARG, "amc_exchange_counters: NULL argument");
    AMC_TRY(need_ladder(h, "amc_exchange_counters"));
    AMC_HIP(hipSetDevice(h->device));
    unsigned long long host[2 * AMC_MAX_RUNGS];
    AMC_TRY(copy_to_host_sync(h, host, h->lad.d_xcnt, XCNT_BYTES));
    for (int r = 0; r + 1 < h->lad.n_rungs; ++r) {
        attempted[r] = (int64_t)host[r];
        accepted[r] = (int64_t)host[AMC_MAX_RUNGS + r];
    }
    return AMC_OK;
}

int amc_set_exchange_counters(amc_handle* h, const int64_t* accepted, const int64_t* attempted)
{
    if (!h || !accepted || !attempted) return fail(AMC_ERR_BAD_ARG, "amc_set_exchange_counters: NULL argument");
    AMC_TRY(need_ladder(h, "amc_set_exchange_counters"));
    unsigned long long host[2 * AMC_MAX_RUNGS] = {0};
    for (int r = 0; r + 1 < h->lad.n_rungs; ++r) {
        if (accepted[r] < 0 || attempted[r] < accepted[r])
            return fail(AMC_ERR_BAD_ARG, "amc_set_exchange_counters: gap %d: need 0 <= accepted <= attempted", r);
        host[r] = (unsigned long long)attempted[r];
        host[AMC_MAX_RUNGS + r] = (unsigned long long)accepted[r];
    }
    AMC_HIP(hipSetDevice(h->device));
    return copy_to_device_sync(h, h->lad.d_xcnt, host, XCNT_BYTES);      // `host` is only valid during the call
}

int amc_reduce_rungs_exact(amc_handle* h, int columns, double* records)
{
    if (!h || !records) return fail(AMC_ERR_BAD_ARG, "amc_reduce_rungs_exact: NULL argument");
    AMC_TRY(need_ladder(h, "amc_reduce_rungs_exact"));
    if (columns <= 0 || (columns & ~AMC_REDUCE_ALL))
        return fail(AMC_ERR_BAD_ARG, "amc_reduce_rungs_exact: columns = %d must be a non-empty combination of AMC_REDUCE_E / _X / _XX", columns);
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of an exchange step: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    RungPass p;
    AMC_TRY(rung_pass_plan(h, amc::RED_COLS, false, &p));      // (unpartitioned under a partition too)
    if (!h->lad.d_rung_recs) AMC_HIP(hipMalloc(&h->lad.d_rung_recs, (size_t)AMC_MAX_RUNGS * amc::RED_COLS * amc::xs::XS_WORDS * sizeof(double)));
    AMC_TRY(rung_pass_launch(h, p, amc::RungSumsArgs(), columns, "amc::rung_sums_kernel", (const void*)amc::rung_sums_kernel<amc::POT_DOUBLE_WELL>,
                             (const void*)amc::rung_sums_kernel<amc::POT_HARMONIC>));
    const int R = h->lad.n_rungs, n_slots = R * amc::RED_COLS;
    hipLaunchKernelGGL(amc::rung_finish_kernel, dim3(n_slots), dim3(64), 0, h->stream, (const amc::xs_word*)h->lad.d_rung_rows, p.n_blocks(), R, columns,
                       h->lad.d_rung_recs);
    AMC_HIP(hipGetLastError());
    return copy_to_host_sync(h, records, h->lad.d_rung_recs, (size_t)n_slots * amc::xs::XS_WORDS * sizeof(double));
}

// ---- bridge sums (DESIGN.md section 3.13 "Bridge sums") --------------------------------------------------------------------------------
static_assert(AMC_BRIDGE_E == amc::BR_E && AMC_BRIDGE_EE == amc::BR_EE && AMC_BRIDGE_WF == amc::BR_WF && AMC_BRIDGE_WB == amc::BR_WB &&
              AMC_BRIDGE_MF == amc::BR_MF && AMC_BRIDGE_MB == amc::BR_MB && AMC_BRIDGE_ALL == amc::BR_ALL, "the columns of include/amc.h and amc_exchange.h");

int amc_bridge_accumulate(amc_handle* h, int columns)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_bridge_accumulate: NULL handle");
    AMC_TRY(need_ladder(h, "amc_bridge_accumulate"));
    if (columns <= 0 || (columns & ~AMC_BRIDGE_ALL))
        return fail(AMC_ERR_BAD_ARG, "amc_bridge_accumulate: columns = %d must be a non-empty combination of the AMC_BRIDGE_* bits", columns);
    if (h->lad.bridge_cols && h->lad.bridge_cols != columns)
        return fail(AMC_ERR_STATE, "amc_bridge_accumulate: columns = %d, the accumulator was begun with %d (amc_bridge_fetch with reset frees the mask)", columns,
                    h->lad.bridge_cols);
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of an exchange step: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    // with a partition a row per (block, rung, column), the number of snapshots behind them: the traversal of amc_blocks.h
    const int B = h->blocks.n_blocks, R = h->lad.n_rungs, n_slots = R * amc::BR_COLS;
    RungPass p;
    amc::BridgeArgs a = {};
    a.beta = h->d_beta;
    AMC_TRY(rung_pass_plan(h, amc::BR_COLS, B != 0, &p));
    if (B) {
        AMC_TRY(blocks_words(h, &h->blocks.d_bridge_blk, &h->blocks.bridge_blk_words, (size_t)B * n_slots * amc::XS_ROW_R + 1));
        AMC_TRY(rung_pass_launch(h, p, a, columns, "amc::bridge_sums_blocks_kernel", (const void*)amc::bridge_sums_blocks_kernel<amc::POT_DOUBLE_WELL>,
                                 (const void*)amc::bridge_sums_blocks_kernel<amc::POT_HARMONIC>));
    } else {
        AMC_TRY(zeroed_words(h, &h->lad.d_bridge, BRIDGE_BYTES));
        AMC_TRY(rung_pass_launch(h, p, a, columns, "amc::bridge_sums_kernel", (const void*)amc::bridge_sums_kernel<amc::POT_DOUBLE_WELL>,
                                 (const void*)amc::bridge_sums_kernel<amc::POT_HARMONIC>));
    }
    amc::xs_word* acc = B ? h->blocks.d_bridge_blk : h->lad.d_bridge;
    hipLaunchKernelGGL(amc::bridge_finish_kernel, dim3((B ? B : 1) * n_slots), dim3(64), 0, h->stream, (const amc::xs_word*)h->lad.d_rung_rows, p.n_blocks(), R,
                       columns, B ? B : 1, acc, acc + (B ? (size_t)B * n_slots * amc::XS_ROW_R : (size_t)amc::BRIDGE_COUNT));
    AMC_HIP(hipGetLastError());
    h->lad.bridge_cols = columns;
    return AMC_OK;
}

int amc_bridge_fetch(amc_handle* h, double* records, uint64_t* n_snapshots, int reset)
{
    if (!h || !records || !n_snapshots) return fail(AMC_ERR_BAD_ARG, "amc_bridge_fetch: NULL argument");
    AMC_TRY(need_ladder(h, "amc_bridge_fetch"));
    AMC_HIP(hipSetDevice(h->device));
    const int R = h->lad.n_rungs, n_slots = R * amc::BR_COLS;
    if (h->blocks.n_blocks) {           // the merge over the blocks: integers, the records of a handle without a partition
        std::vector<amc::xs_word> rows;
        AMC_TRY(bridge_blocks_host(h, &rows));
        *n_snapshots = (uint64_t)rows.back();
        for (int s = 0; s < n_slots; ++s) {
            amc::xs::PartR p = amc::xs::part_r_empty();
            bool any = false;
            for (int b = 0; b < h->blocks.n_blocks; ++b) {
                const amc::xs_word* row = rows.data() + ((size_t)b * n_slots + s) * amc::XS_ROW_R;
                if (!row[5]) continue;
                any = true;
                amc::xs::part_r_merge(p, amc::xs_load_r_row(row));
            }
            double* rec = records + (size_t)s * amc::xs::XS_WORDS;
            if (any) amc::xs::rec_from_r(rec, p);
            else amc::xs::rec_clear(rec);
        }
        if (reset) return bridge_clear(h);
        return AMC_OK;
    }
    std::vector<amc::xs_word> host(amc::BRIDGE_WORDS, 0ull);
    AMC_TRY(copy_to_host_sync(h, host.data(), h->lad.d_bridge, BRIDGE_BYTES));
    *n_snapshots = (uint64_t)host[amc::BRIDGE_COUNT];
    for (int s = 0; s < n_slots; ++s) {
        double* rec = records + (size_t)s * amc::xs::XS_WORDS;
        const amc::xs_word* row = host.data() + (size_t)s * amc::XS_ROW_R;
        if (row[5]) amc::xs::rec_from_r(rec, amc::xs_load_r_row(row));
        else amc::xs::rec_clear(rec);                  // no summand: an end rung's missing slot, a column outside the mask, nothing accumulated
    }
    if (reset) return bridge_clear(h);
    return AMC_OK;
}

// The rows of one accumulator's records (amc_bridge_fetch's layout, R x BR_COLS of them) as amc_set_bridge checks them; *cols: the mask
// read off them, 0 when every record is all zero.  The mask is read off the records: a slot that had a summand is a kind-R record, every
// other is all zero, and a column is in the mask exactly when its interior slots are records (E and EE have a summand at every rung, the
// W and M columns at all but one end).
static int bridge_rows_from_records(const char* who, const double* records, int R, amc::xs_word* rows, int* cols_out)
{
    const int n_slots = R * amc::BR_COLS;
    int cols = 0;
    for (int s = 0; s < n_slots; ++s) {
        const double* rec = records + (size_t)s * amc::xs::XS_WORDS;
        const int r = s / amc::BR_COLS, c = s % amc::BR_COLS;
        bool zero = true;
        for (int i = 0; i < amc::xs::XS_WORDS; ++i) zero = zero && rec[i] == 0.0;
        if (zero) continue;
        char where[48];
        std::snprintf(where, sizeof where, "rung %d, column %d", r, c);
        amc::xs_word* row = rows + (size_t)s * amc::XS_ROW_R;
        AMC_TRY(r_row_from_record(who, where, rec, row));
        if (!((amc::bridge_cols_at(AMC_BRIDGE_ALL, r, R) >> c) & 1))
            return fail(AMC_ERR_BAD_ARG, "%s: rung %d has no summand for column %d, its record must be all zero", who, r, c);
        cols |= 1 << c;
        row[5] = 1ull;
    }
    for (int s = 0; cols && s < n_slots; ++s)
        if (((amc::bridge_cols_at(cols, s / amc::BR_COLS, R) >> (s % amc::BR_COLS)) & 1) && !rows[(size_t)s * amc::XS_ROW_R + 5])
            return fail(AMC_ERR_BAD_ARG, "%s: column %d has records at some rungs and none at rung %d", who, s % amc::BR_COLS, s / amc::BR_COLS);
    *cols_out = cols;
    return AMC_OK;
}

int amc_set_bridge(amc_handle* h, const double* records, uint64_t n_snapshots)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_bridge: NULL handle");
    AMC_TRY(need_ladder(h, "amc_set_bridge"));
    AMC_HIP(hipSetDevice(h->device));
    if (!records || n_snapshots == 0) return bridge_clear(h);
    // (the accumulator in use is the blocked one, which merged records cannot fill: taking them would drop them silently)
    if (h->blocks.n_blocks)
        return fail(AMC_ERR_STATE, "amc_set_bridge: a partition is set (amc_set_blocks): merged records cannot be split into its blocks, "
                                   "amc_set_bridge_blocks restores them");
    std::vector<amc::xs_word> host(amc::BRIDGE_WORDS, 0ull);
    int cols = 0;
    AMC_TRY(bridge_rows_from_records("amc_set_bridge", records, h->lad.n_rungs, host.data(), &cols));
    if (!cols) return fail(AMC_ERR_BAD_ARG, "amc_set_bridge: n_snapshots = %llu with all-zero records", (unsigned long long)n_snapshots);
    host[amc::BRIDGE_COUNT] = (amc::xs_word)n_snapshots;
    if (!h->lad.d_bridge) AMC_HIP(hipMalloc(&h->lad.d_bridge, BRIDGE_BYTES));
    AMC_TRY(copy_to_device_sync(h, h->lad.d_bridge, host.data(), BRIDGE_BYTES));      // `host` is only valid during the call
    h->lad.bridge_cols = cols;
    return AMC_OK;
}

// ---- jackknife blocks --------------------------------------------------------------------------------------
static_assert(AMC_MAX_JK_BLOCKS == amc::blk::BLK_MAX_BLOCKS, "the blocks of include/amc.h and amc_blocks.h");

int amc_set_blocks(amc_handle* h, int n_blocks, int64_t chunk)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_blocks: NULL handle");
    if (n_blocks != 0 && (n_blocks < 2 || n_blocks > AMC_MAX_JK_BLOCKS))
        return fail(AMC_ERR_BAD_ARG, "amc_set_blocks: n_blocks = %d must be 0 (no partition) or lie in [2, %d]", n_blocks, AMC_MAX_JK_BLOCKS);
    if (chunk < 0 || chunk > AMC_MAX_JK_CHUNK)      // (the traversal adds a chunk to a global ladder index: both stay far from 2^63)
        return fail(AMC_ERR_BAD_ARG, "amc_set_blocks: chunk = %lld must lie in [1, 2^40], or be 0 for the default", (long long)chunk);
    if (n_blocks && h->ann.blk_B)
        return fail(AMC_ERR_STATE, "amc_set_blocks: a partition over the annealing families is set (amc_set_anneal_blocks); the two exclude each other");
    AMC_HIP(hipSetDevice(h->device));
    // energy histograms kept under the partition that goes: their blocks' rows are added up on the stream, nothing is lost
    if (!h->ehist.by_family) AMC_TRY(ehist_fold(h));      // (one kept per block of families stays: that partition is not this call's)
    AMC_TRY(emom_fold(h));          // ... and the moments per bin's sets
    // one full block-width of contiguous chains: every lane of a HIP block has a ladder of the chunk, in one trip
    if (n_blocks && chunk == 0) chunk = std::max(1, AMC_BLOCK / pass_groups(h));
    h->blocks.n_blocks = n_blocks;
    h->blocks.chunk = n_blocks ? chunk : 0;
    // sums kept under another partition (or under none) are not sums of these blocks
    AMC_TRY(bridge_clear(h));
    corr_forget(h);
    return AMC_OK;
}

int amc_bridge_fetch_blocks(amc_handle* h, double* records, int capacity_blocks, int* n_blocks, uint64_t* n_snapshots, int reset)
{
    if (!h || !records || !n_blocks || !n_snapshots) return fail(AMC_ERR_BAD_ARG, "amc_bridge_fetch_blocks: NULL argument");
    AMC_TRY(need_ladder(h, "amc_bridge_fetch_blocks"));
    const int B = h->blocks.n_blocks;
    if (!B) return fail(AMC_ERR_STATE, "amc_bridge_fetch_blocks: no partition is set (amc_set_blocks)");
    if (capacity_blocks < B) return fail(AMC_ERR_BAD_ARG, "amc_bridge_fetch_blocks: capacity_blocks = %d, the partition has %d blocks", capacity_blocks, B);
    AMC_HIP(hipSetDevice(h->device));
    const int R = h->lad.n_rungs, n_slots = R * amc::BR_COLS;
    std::vector<amc::xs_word> rows;
    AMC_TRY(bridge_blocks_host(h, &rows));
    const amc::blk::Part part = blocks_part(h);
    for (int b = 0; b < B; ++b) {
        const bool empty = amc::blk::ladders_in_block(part, b, h->M / R) == 0;      // a block without a local ladder: all-zero records
        for (int s = 0; s < n_slots; ++s) {
            double* rec = records + ((size_t)b * n_slots + s) * amc::xs::XS_WORDS;
            const amc::xs_word* row = rows.data() + ((size_t)b * n_slots + s) * amc::XS_ROW_R;
            if (!empty && row[5]) amc::xs::rec_from_r(rec, amc::xs_load_r_row(row));
            else amc::xs::rec_clear(rec);
        }
    }
    *n_blocks = B;
    *n_snapshots = (uint64_t)rows.back();
    if (reset) return bridge_clear(h);
    return AMC_OK;
}

int amc_set_bridge_blocks(amc_handle* h, const double* records, int n_blocks, uint64_t n_snapshots)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_bridge_blocks: NULL handle");
    AMC_TRY(need_ladder(h, "amc_set_bridge_blocks"));
    const int B = h->blocks.n_blocks;
    if (!B) return fail(AMC_ERR_STATE, "amc_set_bridge_blocks: no partition is set (amc_set_blocks)");
    AMC_HIP(hipSetDevice(h->device));
    if (!records || n_snapshots == 0) return bridge_clear(h);
    if (n_blocks != B) return fail(AMC_ERR_BAD_ARG, "amc_set_bridge_blocks: n_blocks = %d, the partition has %d blocks", n_blocks, B);
    // every block's records as amc_set_bridge checks one accumulator's; the blocks with a local ladder share one mask, the others are all zero
    const int R = h->lad.n_rungs, n_slots = R * amc::BR_COLS;
    const size_t words = (size_t)B * n_slots * amc::XS_ROW_R + 1;
    std::vector<amc::xs_word> host(words, 0ull);
    const amc::blk::Part part = blocks_part(h);
    int cols = 0;
    for (int b = 0; b < B; ++b) {
        int cols_b = 0;
        AMC_TRY(bridge_rows_from_records("amc_set_bridge_blocks", records + (size_t)b * n_slots * amc::xs::XS_WORDS, R,
                                         host.data() + (size_t)b * n_slots * amc::XS_ROW_R, &cols_b));
        if (amc::blk::ladders_in_block(part, b, h->M / R) == 0) {
            if (cols_b) return fail(AMC_ERR_BAD_ARG, "amc_set_bridge_blocks: block %d has no local ladder, its records must be all zero", b);
            continue;
        }
        if (!cols_b) return fail(AMC_ERR_BAD_ARG, "amc_set_bridge_blocks: n_snapshots = %llu with all-zero records in block %d", (unsigned long long)n_snapshots, b);
        if (cols && cols_b != cols) return fail(AMC_ERR_BAD_ARG, "amc_set_bridge_blocks: block %d holds the columns %d, the blocks below it %d", b, cols_b, cols);
        cols = cols_b;
    }
    host[words - 1] = (amc::xs_word)n_snapshots;
    AMC_TRY(blocks_words(h, &h->blocks.d_bridge_blk, &h->blocks.bridge_blk_words, words));
    AMC_TRY(copy_to_device_sync(h, h->blocks.d_bridge_blk, host.data(), words * sizeof(amc::xs_word)));      // `host` is only valid during the call
    h->lad.bridge_cols = cols;
    return AMC_OK;
}

int amc_get_exchange_step(amc_handle* h, uint64_t* t)
{
    if (!h || !t) return fail(AMC_ERR_BAD_ARG, "amc_get_exchange_step: NULL argument");
    AMC_TRY(need_ladder(h, "amc_get_exchange_step"));
    *t = h->lad.t_x;
    return AMC_OK;
}

int amc_set_exchange_step(amc_handle* h, uint64_t t)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_exchange_step: NULL handle");
    AMC_TRY(need_ladder(h, "amc_set_exchange_step"));
    if (t >> 48) return fail(AMC_ERR_BAD_ARG, "amc_set_exchange_step: step index must fit 48 bits");
    h->lad.t_x = t;
    return AMC_OK;
}

// ---- walker tracking (DESIGN.md section 3.13 "Walker tracking") ---------------------------------------------------------------------
int amc_set_tracking(amc_handle* h, int on)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_tracking: NULL handle");
    AMC_HIP(hipSetDevice(h->device));
    if (!on) return tracking_off(h);
    AMC_TRY(need_ladder(h, "amc_set_tracking"));
    if (!h->lad.d_lab) {
        AMC_HIP(hipMalloc(&h->lad.d_lab, (size_t)h->M));
        const hipError_t e = hipMalloc(&h->lad.d_track, TRACK_BYTES);
        if (e != hipSuccess) {
            (void)hipFree(h->lad.d_lab);
            h->lad.d_lab = nullptr;
            h->lad.d_track = nullptr;
            return fail(e == hipErrorOutOfMemory ? AMC_ERR_OOM : AMC_ERR_HIP, "amc_set_tracking: %s", hipGetErrorString(e));
        }
    }
    const int R = h->lad.n_rungs;
    std::vector<uint8_t> lab((size_t)h->M);
    for (int64_t c = 0; c < h->M; ++c) {
        const int r = (int)(c % R);
        lab[(size_t)c] = (uint8_t)(r | (r == 0 ? amc::LAB_UP : r == R - 1 ? amc::LAB_DOWN : 0u));
    }
    AMC_HIP(hipMemcpyAsync(h->lad.d_lab, lab.data(), (size_t)h->M, hipMemcpyHostToDevice, h->stream));
    AMC_HIP(hipMemsetAsync(h->lad.d_track, 0, TRACK_BYTES, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));      // `lab` is only valid during the call
    return AMC_OK;
}

int amc_download_labels(amc_handle* h, uint8_t* labels)
{
    if (!h || !labels) return fail(AMC_ERR_BAD_ARG, "amc_download_labels: NULL argument");
    AMC_TRY(need_tracking(h, "amc_download_labels"));
    AMC_HIP(hipSetDevice(h->device));
    return copy_to_host_sync(h, labels, h->lad.d_lab, (size_t)h->M);
}

int amc_upload_labels(amc_handle* h, const uint8_t* labels)
{
    if (!h || !labels) return fail(AMC_ERR_BAD_ARG, "amc_upload_labels: NULL argument");
    AMC_TRY(need_tracking(h, "amc_upload_labels"));
    const int R = h->lad.n_rungs;
    for (int64_t c0 = 0; c0 < h->M; c0 += R) {
        uint64_t seen = 0;
        for (int r = 0; r < R; ++r) {
            const int64_t c = c0 + r;
            const int w = labels[c] & amc::LAB_WALKER, d = labels[c] >> 6;
            if (w >= R) return fail(AMC_ERR_BAD_ARG, "amc_upload_labels: chain %lld: walker id %d >= n_rungs = %d", (long long)c, w, R);
            if (d == 3) return fail(AMC_ERR_BAD_ARG, "amc_upload_labels: chain %lld: direction 3", (long long)c);
            if (r == 0 && d != 1) return fail(AMC_ERR_BAD_ARG, "amc_upload_labels: chain %lld sits at rung 0, its direction must be 1, not %d", (long long)c, d);
            if (r == R - 1 && d != 2)
                return fail(AMC_ERR_BAD_ARG, "amc_upload_labels: chain %lld sits at rung %d, its direction must be 2, not %d", (long long)c, R - 1, d);
            if ((seen >> w) & 1u)
                return fail(AMC_ERR_BAD_ARG, "amc_upload_labels: chain %lld: walker id %d occurs twice in its ladder (not a permutation)", (long long)c, w);
            seen |= (uint64_t)1 << w;
        }
    }
    AMC_HIP(hipSetDevice(h->device));
    return copy_to_device_sync(h, h->lad.d_lab, labels, (size_t)h->M);      // `labels` is only valid during the call
}

int amc_flow_rungs(amc_handle* h, uint64_t* counts)
{
    if (!h || !counts) return fail(AMC_ERR_BAD_ARG, "amc_flow_rungs: NULL argument");
    AMC_TRY(need_tracking(h, "amc_flow_rungs"));
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of an exchange step: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    AMC_TRY(flow_snapshot_queue(h));
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "counts are copied as they are");
    return copy_to_host_sync(h, counts, h->lad.d_track + 2, (size_t)(3 * h->lad.n_rungs) * sizeof(unsigned long long));
}

int amc_tracking_counters(amc_handle* h, int64_t* round_trips, int64_t* up_trips)
{
    if (!h || !round_trips || !up_trips) return fail(AMC_ERR_BAD_ARG, "amc_tracking_counters: NULL argument");
    AMC_TRY(need_tracking(h, "amc_tracking_counters"));
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));
    unsigned long long host[2];
    AMC_TRY(copy_to_host_sync(h, host, h->lad.d_track, sizeof host));
    *round_trips = (int64_t)host[0];
    *up_trips = (int64_t)host[1];
    return AMC_OK;
}

int amc_set_tracking_counters(amc_handle* h, int64_t round_trips, int64_t up_trips)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_tracking_counters: NULL handle");
    AMC_TRY(need_tracking(h, "amc_set_tracking_counters"));
    if (round_trips < 0 || up_trips < 0) return fail(AMC_ERR_BAD_ARG, "amc_set_tracking_counters: need round_trips >= 0 and up_trips >= 0");
    const unsigned long long host[2] = {(unsigned long long)round_trips, (unsigned long long)up_trips};
    AMC_HIP(hipSetDevice(h->device));
    return copy_to_device_sync(h, h->lad.d_track, host, sizeof host);      // `host` is only valid during the call
}

// ---- respacing the ladder (DESIGN.md section 3.13 "Respacing") -----------------------------------------------------------------------
int amc_respace_ladder(amc_handle* h, int rule, double gamma, double eps, const uint64_t* counts)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_respace_ladder: NULL handle");
    AMC_TRY(need_ladder(h, "amc_respace_ladder"));
    if (rule != AMC_RESPACE_ACCEPTANCE && rule != AMC_RESPACE_FLOW)
        return fail(AMC_ERR_BAD_ARG, "amc_respace_ladder: rule = %d must be AMC_RESPACE_ACCEPTANCE (%d) or AMC_RESPACE_FLOW (%d)", rule,
                    AMC_RESPACE_ACCEPTANCE, AMC_RESPACE_FLOW);
    if (!(gamma > 0.0 && gamma <= 1.0)) return fail(AMC_ERR_BAD_ARG, "amc_respace_ladder: gamma = %g must lie in (0, 1]", gamma);
    if (!(eps >= 0.0 && eps < 1.0)) return fail(AMC_ERR_BAD_ARG, "amc_respace_ladder: eps = %g must lie in [0, 1)", eps);
    if (rule == AMC_RESPACE_FLOW && !counts && !h->lad.d_lab)
        return fail(AMC_ERR_STATE, "amc_respace_ladder: rule AMC_RESPACE_FLOW with counts == NULL reads this handle's labels, and tracking is off "
                                   "(amc_set_tracking)");
    const int R = h->lad.n_rungs;
    amc::RespaceCounts given;
    std::memset(&given, 0, sizeof given);
    if (counts) {
        if (rule == AMC_RESPACE_ACCEPTANCE)
            for (int j = 0; j < R - 1; ++j)
                if (counts[R - 1 + j] > counts[j])
                    return fail(AMC_ERR_BAD_ARG, "amc_respace_ladder: counts: gap %d has more accepted swaps than attempted ones", j);
        const int n = rule == AMC_RESPACE_ACCEPTANCE ? 2 * (R - 1) : 3 * R;
        for (int i = 0; i < n; ++i) given.c[i] = (unsigned long long)counts[i];
    }
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of an exchange step: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    AMC_TRY(zeroed_words(h, &h->lad.d_respace, RESPACE_BYTES));
    unsigned long long* d_flow = h->lad.d_lab ? h->lad.d_track + 2 : nullptr;
    if (rule == AMC_RESPACE_FLOW && !counts) AMC_TRY(flow_snapshot_queue(h));      // of this handle's labels, into amc_flow_rungs' scratch
    amc::RespaceArgs a;
    a.beta = h->d_beta;
    a.xcnt = h->lad.d_xcnt;
    a.flow = d_flow;
    a.gaps = h->lad.d_xcnt;
    a.trips = h->lad.d_lab ? h->lad.d_track : nullptr;
    a.rec = h->lad.d_respace;
    a.bridge = h->lad.d_bridge;
    a.bridge_words = amc::BRIDGE_WORDS;
    if (h->blocks.n_blocks) {           // the accumulator in use is the blocked one: every block's rows go
        a.bridge = h->blocks.d_bridge_blk;
        a.bridge_words = (int32_t)h->blocks.bridge_blk_words;
    }
    a.gamma = gamma;
    a.eps = eps;
    a.rule = rule;
    a.n_rungs = R;
    a.f32 = h->f32 ? 1 : 0;
    a.counts_given = counts ? 1 : 0;
    hipLaunchKernelGGL(amc::ladder_respace_kernel, dim3(1), dim3(64), 0, h->stream, a, given);
    AMC_HIP(hipGetLastError());
    AMC_TRY(ehist_respaced(h));         // the energy histograms' cells go with status 0, as the bridge records do
    AMC_TRY(emom_respaced(h));          // ... and the moments per bin's
    hipLaunchKernelGGL(amc::ladder_retile_kernel, dim3(grid_for(h, h->M)), dim3(AMC_BLOCK), 0, h->stream, (void*)h->d_beta, a.f32, h->lad.d_lab, h->M / R, R,
                       (const unsigned long long*)h->lad.d_respace);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

int amc_respace_status(amc_handle* h, int* status, int64_t* n_respaced)
{
    if (!h || !status || !n_respaced) return fail(AMC_ERR_BAD_ARG, "amc_respace_status: NULL argument");
    AMC_TRY(need_ladder(h, "amc_respace_status"));
    unsigned long long host[2] = {0ull, 0ull};
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(copy_to_host_sync(h, host, h->lad.d_respace, sizeof host));
    *status = (int)host[amc::RESPACE_STATUS];
    *n_respaced = (int64_t)host[amc::RESPACE_COUNT];
    return AMC_OK;
}

int amc_set_respaced(amc_handle* h, int64_t n_respaced)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_respaced: NULL handle");
    AMC_TRY(need_ladder(h, "amc_set_respaced"));
    if (n_respaced < 0) return fail(AMC_ERR_BAD_ARG, "amc_set_respaced: n_respaced < 0");
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(zeroed_words(h, &h->lad.d_respace, RESPACE_BYTES));
    const unsigned long long host = (unsigned long long)n_respaced;
    return copy_to_device_sync(h, h->lad.d_respace + amc::RESPACE_COUNT, &host, sizeof host);      // `host` is only valid during the call
}

int amc_get_ladder(amc_handle* h, double* betas)
{
    if (!h || !betas) return fail(AMC_ERR_BAD_ARG, "amc_get_ladder: NULL argument");
    AMC_TRY(need_ladder(h, "amc_get_ladder"));
    AMC_HIP(hipSetDevice(h->device));
    double host[AMC_MAX_RUNGS];      // the first local ladder as the device holds it
    float host32[AMC_MAX_RUNGS];
    const int R = h->lad.n_rungs;
    AMC_TRY(h->f32 ? copy_to_host_sync(h, host32, h->d_beta, (size_t)R * sizeof(float)) : copy_to_host_sync(h, host, h->d_beta, (size_t)R * sizeof(double)));
    for (int r = 0; r < R; ++r) betas[r] = h->f32 ? (double)host32[r] : host[r];
    return AMC_OK;
}

// ---- tuning the widths per rung (DESIGN.md section 3.13 "Tuning the widths") -----------------------------------------------------------
// What every entry of the window needs: a ladder, per-chain counters, cells that fit the base.
static int window_state(amc_handle* h, const char* who)
{
    AMC_TRY(need_ladder(h, who));
    if (!h->counters) return fail(AMC_ERR_STATE, "%s: handle was created with per_chain_counters = 0", who);
    if (h->K * h->lad.n_rungs > AMC_MAX_MOVES)
        return fail(AMC_ERR_STATE, "%s: %d moves x %d rungs = %d cells, the window holds %d", who, h->K, h->lad.n_rungs, h->K * h->lad.n_rungs, AMC_MAX_MOVES);
    return AMC_OK;
}

static amc::TuneArgs tune_args(const amc_handle* h)
{
    amc::TuneArgs a;
    std::memset(&a, 0, sizeof a);
    a.rung_tab = h->lad.d_rung_tab;
    a.cnt = h->lad.d_rung_cnt;
    a.base = h->lad.d_rung_base;
    a.rec = h->lad.d_tune;
    a.steps_per_rung = (h->t_base + h->t_counted) * (uint64_t)(h->M / h->lad.n_rungs);
    a.n_moves = h->K;
    a.n_rungs = h->lad.n_rungs;
    return a;
}

int amc_tune_rung_sigma(amc_handle* h, double target, double gamma, int64_t min_calls, double sigma_lo, double sigma_hi, const int64_t* counts)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_tune_rung_sigma: NULL handle");
    AMC_TRY(need_ladder(h, "amc_tune_rung_sigma"));
    if (!h->counters) return fail(AMC_ERR_STATE, "amc_tune_rung_sigma: handle was created with per_chain_counters = 0");
    if (!h->lad.rung_on) return fail(AMC_ERR_STATE, "amc_tune_rung_sigma: no widths per rung are set (amc_set_rung_sigma)");
    if (!(target > 0.0 && target < 1.0)) return fail(AMC_ERR_BAD_ARG, "amc_tune_rung_sigma: target = %g must lie in (0, 1)", target);
    if (!(gamma > 0.0 && gamma <= 1.0)) return fail(AMC_ERR_BAD_ARG, "amc_tune_rung_sigma: gamma = %g must lie in (0, 1]", gamma);
    if (min_calls < 1) return fail(AMC_ERR_BAD_ARG, "amc_tune_rung_sigma: min_calls = %lld must be at least 1", (long long)min_calls);
    if (!(sigma_lo >= 1e-100 && sigma_lo <= 1e100)) return fail(AMC_ERR_BAD_ARG, "amc_tune_rung_sigma: sigma_lo = %g must lie in [1e-100, 1e100]", sigma_lo);
    if (!(sigma_hi >= 1e-100 && sigma_hi <= 1e100)) return fail(AMC_ERR_BAD_ARG, "amc_tune_rung_sigma: sigma_hi = %g must lie in [1e-100, 1e100]", sigma_hi);
    if (sigma_lo > sigma_hi) return fail(AMC_ERR_BAD_ARG, "amc_tune_rung_sigma: sigma_lo = %g is above sigma_hi = %g", sigma_lo, sigma_hi);
    const int R = h->lad.n_rungs, n = h->K * R;      // (n <= AMC_MAX_MOVES: amc_set_rung_sigma)
    amc::TuneCounts given;
    std::memset(&given, 0, sizeof given);
    if (counts) {
        for (int e = 0; e < n; ++e) {
            if (counts[e] < 0 || counts[n + e] < 0)
                return fail(AMC_ERR_BAD_ARG, "amc_tune_rung_sigma: counts: entry %d (move %d, rung %d) is negative", e, e / R, e % R);
            if (counts[e] > counts[n + e])
                return fail(AMC_ERR_BAD_ARG, "amc_tune_rung_sigma: counts: entry %d (move %d, rung %d) has more accepted calls than calls", e, e / R, e % R);
            given.c[e] = (unsigned long long)counts[e];
            given.c[n + e] = (unsigned long long)counts[n + e];
        }
    }
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of amc_set_rung_sigma: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    AMC_TRY(zeroed_words(h, &h->lad.d_rung_base, RUNG_BASE_BYTES));
    AMC_TRY(zeroed_words(h, &h->lad.d_tune, TUNE_BYTES));
    AMC_TRY(rung_totals_queue(h));
    amc::TuneArgs a = tune_args(h);
    a.min_calls = (unsigned long long)min_calls;
    a.target = target;
    a.gamma = gamma;
    a.lo = sigma_lo;
    a.hi = sigma_hi;
    a.counts_given = counts ? 1 : 0;
    hipLaunchKernelGGL(amc::rung_sigma_tune_kernel, dim3(1), dim3(AMC_MAX_MOVES), 0, h->stream, a, given);
    AMC_HIP(hipGetLastError());
    h->lad.tune_queued = true;
    return AMC_OK;
}

int amc_tune_status(amc_handle* h, int* st, int n, int64_t* n_tuned)
{
    if (!h || !st || !n_tuned) return fail(AMC_ERR_BAD_ARG, "amc_tune_status: NULL argument");
    if (!h->lad.rung_on) return fail(AMC_ERR_STATE, "amc_tune_status: no widths per rung are set (amc_set_rung_sigma)");
    if (n != h->K * h->lad.n_rungs)
        return fail(AMC_ERR_BAD_ARG, "amc_tune_status: n = %d, the table of %d moves x %d rungs has %d entries", n, h->K, h->lad.n_rungs, h->K * h->lad.n_rungs);
    unsigned long long host[1 + AMC_MAX_MOVES] = {0ull};
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(copy_to_host_sync(h, host, h->lad.d_tune, (size_t)(1 + n) * sizeof(unsigned long long)));
    *n_tuned = (int64_t)host[amc::TUNE_COUNT];
    for (int e = 0; e < n; ++e) st[e] = (int)host[amc::TUNE_ST + e];
    return AMC_OK;
}

int amc_set_tuned(amc_handle* h, int64_t n_tuned)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_tuned: NULL handle");
    if (!h->lad.rung_on) return fail(AMC_ERR_STATE, "amc_set_tuned: no widths per rung are set (amc_set_rung_sigma)");
    if (n_tuned < 0) return fail(AMC_ERR_BAD_ARG, "amc_set_tuned: n_tuned < 0");
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(zeroed_words(h, &h->lad.d_tune, TUNE_BYTES));
    const unsigned long long host = (unsigned long long)n_tuned;
    return copy_to_device_sync(h, h->lad.d_tune + amc::TUNE_COUNT, &host, sizeof host);      // `host` is only valid during the call
}

int amc_rung_window_restart(amc_handle* h)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_rung_window_restart: NULL handle");
    AMC_TRY(window_state(h, "amc_rung_window_restart"));
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(zeroed_words(h, &h->lad.d_rung_base, RUNG_BASE_BYTES));
    AMC_TRY(rung_totals_queue(h));
    const amc::TuneArgs a = tune_args(h);
    hipLaunchKernelGGL(amc::rung_window_restart_kernel, dim3(1), dim3(AMC_MAX_MOVES), 0, h->stream, a);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

int amc_rung_window_base(amc_handle* h, int64_t* accepted, int64_t* total)
{
    if (!h || !accepted || !total) return fail(AMC_ERR_BAD_ARG, "amc_rung_window_base: NULL argument");
    AMC_TRY(window_state(h, "amc_rung_window_base"));
    const int n = h->K * h->lad.n_rungs;
    unsigned long long host[amc::RUNG_BASE_WORDS] = {0ull};
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(copy_to_host_sync(h, host, h->lad.d_rung_base, RUNG_BASE_BYTES));
    for (int e = 0; e < n; ++e) {
        accepted[e] = (int64_t)host[e];
        total[e] = (int64_t)host[AMC_MAX_MOVES + e];
    }
    return AMC_OK;
}

int amc_set_rung_window_base(amc_handle* h, const int64_t* accepted, const int64_t* total)
{
    if (!h || !accepted || !total) return fail(AMC_ERR_BAD_ARG, "amc_set_rung_window_base: NULL argument");
    AMC_TRY(window_state(h, "amc_set_rung_window_base"));
    const int R = h->lad.n_rungs, n = h->K * R;
    unsigned long long host[amc::RUNG_BASE_WORDS] = {0ull};
    for (int e = 0; e < n; ++e) {
        if (accepted[e] < 0 || total[e] < 0)
            return fail(AMC_ERR_BAD_ARG, "amc_set_rung_window_base: entry %d (move %d, rung %d) is negative", e, e / R, e % R);
        host[e] = (unsigned long long)accepted[e];
        host[AMC_MAX_MOVES + e] = (unsigned long long)total[e];
    }
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(zeroed_words(h, &h->lad.d_rung_base, RUNG_BASE_BYTES));
    return copy_to_device_sync(h, h->lad.d_rung_base, host, RUNG_BASE_BYTES);      // `host` is only valid during the call
}

int amc_rung_window_counts(amc_handle* h, int64_t* accepted, int64_t* total)
{
    if (!h || !accepted || !total) return fail(AMC_ERR_BAD_ARG, "amc_rung_window_counts: NULL argument");
    AMC_TRY(window_state(h, "amc_rung_window_counts"));
    const int n = h->K * h->lad.n_rungs;
    int64_t base_acc[AMC_MAX_MOVES], base_tot[AMC_MAX_MOVES];
    AMC_TRY(amc_rung_window_base(h, base_acc, base_tot));
    AMC_TRY(amc_rung_counter_totals(h, accepted, total));
    for (int e = 0; e < n; ++e) {
        if (accepted[e] < base_acc[e] || total[e] < base_tot[e]) {      // counters uploaded or restored behind the base
            accepted[e] = total[e] = -1;
        } else {
            accepted[e] -= base_acc[e];
            total[e] -= base_tot[e];
        }
    }
    return AMC_OK;
}

}  // extern "C"
