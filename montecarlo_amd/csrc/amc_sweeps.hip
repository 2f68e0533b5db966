// amc_sweeps.hip -- sweep launches: n_sweeps x sweepstep MH steps in launches of at most 2^20 steps (amc_sweep, amc_sweep_launches),
// the last of them forming the callback sums when asked (sweep_impl, for amc_sweep_reduce_begin).
#define AMC_KERNEL_LINKAGE static      // the plain kernels are amc_api.hip's: this object launches template instantiations only
#include "amc_internal.h"

// sweep_kernel<POT, MULTI, LOG, BETA, SINGLE, FORM>, BETA the handle's (an array of betas or one); on `stream`: the handle's, or
// the stream of a slice (sweep_launches_sliced)
template <int POT, bool MULTI, int LOG, bool SINGLE, int FORM>
int launch_sweep_beta(amc_handle* h, const amc::SweepArgs& a, int grid, hipStream_t stream)
{
    if (h->beta_arr)
        hipLaunchKernelGGL((amc::sweep_kernel<POT, MULTI, LOG, true, SINGLE, FORM>), dim3(grid), dim3(AMC_BLOCK), 0, stream, a);
    else
        hipLaunchKernelGGL((amc::sweep_kernel<POT, MULTI, LOG, false, SINGLE, FORM>), dim3(grid), dim3(AMC_BLOCK), 0, stream, a);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

// sweep_kernel<POT, MULTI, LOG, true, SINGLE, RED_FORM_NONE, true>: the form that takes its widths from the rung table
template <int POT, bool MULTI, int LOG>
int launch_sweep_rung(const amc::SweepArgs& a, int grid, hipStream_t stream)
{
    if (a.n_steps == 1)
        hipLaunchKernelGGL((amc::sweep_kernel<POT, MULTI, LOG, true, true, amc::RED_FORM_NONE, true>), dim3(grid), dim3(AMC_BLOCK), 0, stream, a);
    else
        hipLaunchKernelGGL((amc::sweep_kernel<POT, MULTI, LOG, true, false, amc::RED_FORM_NONE, true>), dim3(grid), dim3(AMC_BLOCK), 0, stream, a);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

template <int POT, int FORM>
int launch_sweep_form(amc_handle* h, const amc::SweepArgs& a, int grid, hipStream_t stream)
{
    if (h->lad.rung_on) {
        // widths per rung (amc_set_rung_sigma): a ladder and per-chain counters are given; the callback sums come from a pass of their own
        if (FORM != amc::RED_FORM_NONE) return fail(AMC_ERR_STATE, "sweep: no launch forms the callback sums while widths per rung are set");
        if (h->K > 1 && log_form(h) == AMC_LOG_PACKED) return launch_sweep_rung<POT, true, AMC_LOG_PACKED>(a, grid, stream);
        if (h->K > 1) return launch_sweep_rung<POT, true, AMC_LOG_BYTES>(a, grid, stream);
        return launch_sweep_rung<POT, false, AMC_LOG_PACKED>(a, grid, stream);
    }
#define AMC_SWEEP(MULTI, LOG)                                                                                                 \
    (a.n_steps == 1 ? launch_sweep_beta<POT, MULTI, LOG, true, FORM>(h, a, grid, stream) : launch_sweep_beta<POT, MULTI, LOG, false, FORM>(h, a, grid, stream))
    // K > 1 always keeps per-chain counters (callback_acceptance is a mean of per-chain ratios); the step log's form is
    // part of the instantiation (log_form)
    if (h->K > 1 && log_form(h) == AMC_LOG_PACKED) return AMC_SWEEP(true, AMC_LOG_PACKED);
    if (h->K > 1) return AMC_SWEEP(true, AMC_LOG_BYTES);
    if (h->counters) return AMC_SWEEP(false, AMC_LOG_PACKED);
    return AMC_SWEEP(false, AMC_LOG_NONE);
#undef AMC_SWEEP
}

// reduce: the launch also forms the callback sums, in the form red_form picks
template <int POT>
int launch_sweep(amc_handle* h, const amc::SweepArgs& a, int grid, bool reduce, hipStream_t stream)
{
    if (!reduce) return launch_sweep_form<POT, amc::RED_FORM_NONE>(h, a, grid, stream);
    return red_form(h) == amc::RED_FORM_E ? launch_sweep_form<POT, amc::RED_FORM_E>(h, a, grid, stream) : launch_sweep_form<POT, amc::RED_FORM_COLS>(h, a, grid, stream);
}

static const char* tf(bool b) { return b ? "true" : "false"; }

// sweep_kernel<POT_CUSTOM, MULTI, LOG, BETA, SINGLE, REDUCE> with the flags launch_sweep picks
static int launch_sweep_custom(amc_handle* h, amc::SweepArgs& a, int grid, bool reduce)
{
    const bool multi = h->K > 1;
    const std::string inst = "amc::sweep_kernel<" + std::to_string(h->potential) + "," + tf(multi) + "," + std::to_string(log_form(h)) + "," + tf(h->beta_arr) + "," +
                             tf(a.n_steps == 1) + "," + std::to_string(reduce ? red_form(h) : (int)amc::RED_FORM_NONE) + (h->lad.rung_on ? ",true>" : ">");
    if (h->lad.rung_on && reduce) return fail(AMC_ERR_STATE, "sweep: no launch forms the callback sums while widths per rung are set");
    void* params[] = {&a};
    return rtc_launch(h, inst, grid, params);
}

// grid: the grid of the sweep_kernel launch the arguments are for (its trip count depends on it); 0: no such launch (the estimator
// kernels take SweepArgs too and have loops of their own)
amc::SweepArgs make_sweep_args(const amc_handle* h, int32_t n_steps, int grid)
{
    amc::SweepArgs a;
    a.x = h->d_x;
    a.beta_arr = h->beta_arr ? h->d_beta : nullptr;
    a.log = h->d_log;
    a.log_pos = h->log_fill;
    a.ptab = h->d_ptab;
    a.pick_tab = h->d_pick;
    a.acc_total = h->d_acc_slots;
    a.n_chains = h->M;
    a.m_stride = h->M_pad;
    a.pair0 = (uint64_t)h->offset >> 1;
    a.t0 = h->t;
    a.n_steps = n_steps;
    a.n_moves = h->K;
    a.key0 = (uint32_t)h->seed;
    a.key1 = (uint32_t)(h->seed >> 32);
    a.beta = h->beta;
    a.red_partials = h->red[(h->red_head + h->red_count) % RED_TICKETS].h_rows;   // the ticket a REDUCE launch would fill
    a.red_stride = RED_HOST_STRIDE;
    a.red_cols = h->red_cols;
    a.exact_accept = h->knobs.exact_accept ? 1 : 0;
    a.n_slots = h->n_slots;
    if (h->lad.rung_on) a.rung_tab = h->lad.d_rung_tab;       // (in red_partials' place: no launch of such a handle forms the callback sums)
    a.n_rungs = h->lad.n_rungs;
    a.full_rounds = a.tail_pairs = 0;
    if (grid > 0) {
        const int64_t n_pairs = (h->M + 1) / 2, round = (int64_t)grid * AMC_BLOCK;
        a.full_rounds = (int32_t)(n_pairs / round);
        a.tail_pairs = (int32_t)(n_pairs % round);
    }
    return a;
}

// the grid of the sweep launch that also forms the callback sums (sweep_impl)
int reduce_sweep_grid(const amc_handle* h)
{
    return grid_for(h, (h->M + 1) / 2, h->blocks_per_cu_pg ? h->blocks_per_cu_pg : h->blocks_per_cu_red);
}

// n_sweeps x sweepstep MH steps in launches of at most 2^20 steps; when fuse_reduce is set (streamed form
// only) the LAST launch also leaves the callback partial sums of the final state in h_partials[grid][8].
int sweep_impl(amc_handle* h, int64_t n_sweeps, bool fuse_reduce, int* grid_out)
{
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));      // the sweep kernels read sigma from the parameter table
    int64_t remaining = n_sweeps * (int64_t)h->sweepstep;
    // one grid for the whole call (the caller of a fused reduction sums `grid` rows)
    // (a call whose last launch also forms the callback sums: that form holds 5 blocks per CU -- 89 VGPRs -- and runs one round of
    // them, 49 -> 45 us per callback at K = 2 and 1e7 chains; plain sweeps are indifferent between 5 and 8)
    const int grid = fuse_reduce ? reduce_sweep_grid(h) : grid_for(h, (h->M + 1) / 2, remaining == 1 ? h->blocks_per_cu_single : 0);
    if (fuse_reduce && grid > h->n_slots) return fail(AMC_ERR_STATE, "sweep_impl: a grid of %d blocks has no rows to leave its callback sums in (%d)", grid, h->n_slots);
    if (grid_out) *grid_out = grid;
    if (h->knobs.debug_plan)
        std::fprintf(stderr, "[amc] sweep: %lld pairs in a grid of %d blocks, %lld pairs per round\n", (long long)((h->M + 1) / 2), grid, (long long)grid * AMC_BLOCK);
    while (remaining > 0) {
        int32_t chunk = remaining > (1 << 20) ? (1 << 20) : (int32_t)remaining;
        if (h->d_log) {      // per-chain counters: one log row per MH step; a full log is folded before it is reused
            int room = 0;
            AMC_TRY(log_room(h, &room));
            if (chunk > room) chunk = room;
        }
        AMC_TRY(counter_room(h, "amc_sweep", (uint64_t)chunk));      // (may carry the counters: arrays restart at zero)
        amc::SweepArgs a = make_sweep_args(h, chunk, grid);
        a.red_stride = red_row_stride(h, grid);
        const bool last = remaining == chunk;
        const bool reduce = fuse_reduce && last;
        const int rc = h->use_rtc ? launch_sweep_custom(h, a, grid, reduce)
                       : (h->potential == AMC_POTENTIAL_DOUBLE_WELL) ? launch_sweep<amc::POT_DOUBLE_WELL>(h, a, grid, reduce, h->stream)
                                                                     : launch_sweep<amc::POT_HARMONIC>(h, a, grid, reduce, h->stream);
        if (rc != AMC_OK) return rc;
        h->t += (uint64_t)chunk;
        h->t_counted += (uint64_t)chunk;
        if (h->d_log) h->log_fill += chunk;
        remaining -= chunk;
    }
    return AMC_OK;
}

// ---- single-sweep launches in slices ---------------------------------------------------------------------------------------------
// A single-sweep launch spends a good part of its time at its two ends (the launch boundary, the ramp into cold caches, the drain of
// the last trip's stores), during which the whole device's vector units idle.  Chains are independent, the Philox counter is keyed
// by global pair id and step, and the pool-wide accepted count is an integer sum over atomics: the ensemble can be cut into slices
// (amc_slices.h) whose launches run on streams of their own, the ends of one under the middle of the others.  Every chain takes the
// same steps with the same draws; only the schedule changes.

// The slices a call of n single-sweep launches runs in; count <= 1: the plain route.
static amc::SlicePlan sliced_route_plan(const amc_handle* h, int64_t n_launches)
{
    amc::SlicePlan none;
    // K == 1 with the pool-wide counter only (no step log), one step per launch, offline kernels (a run-time compiled kernel's launch
    // takes the handle's stream, rtc_launch)
    if (h->sweep_slices <= 1 || n_launches < 2 || h->sweepstep != 1 || h->K != 1 || h->d_log || h->knobs.exact_accept || h->use_rtc) return none;
    if (h->M < h->slice_min_chains) return none;
    const amc::SlicePlan plan = amc::plan_slices(h->M, AMC_BLOCK, h->sweep_slices, h->n_cu, h->slice_blocks_per_cu, h->n_slots);
    return plan.count > 1 ? plan : none;
}

// The side streams and the events of the fork and the joins, made once.  A handle that cannot have them takes the plain route for good.
static bool slice_streams_ready(amc_handle* h, int n_side)
{
    hipError_t e = hipSuccess;
    if (!h->slice_fork) e = hipEventCreateWithFlags(&h->slice_fork, hipEventDisableTiming);
    for (int i = 0; i < n_side && e == hipSuccess; ++i) {
        if (!h->slice_stream[i]) e = hipStreamCreateWithFlags(&h->slice_stream[i], hipStreamNonBlocking);
        if (e == hipSuccess && !h->slice_join[i]) e = hipEventCreateWithFlags(&h->slice_join[i], hipEventDisableTiming);
    }
    if (e == hipSuccess) return true;
    (void)hipGetLastError();
    h->sweep_slices = 1;
    if (h->knobs.debug_plan) std::fprintf(stderr, "[amc] sweep slices: %s; single-sweep launches stay whole from here on\n", hipGetErrorString(e));
    return false;
}

// The arguments of slice `sl`'s launch: the slice is that launch's whole ensemble.
static amc::SweepArgs slice_sweep_args(const amc::SweepArgs& whole, const amc::Slice& sl)
{
    amc::SweepArgs a = whole;
    a.x = whole.x + 2 * sl.first_pair;
    if (whole.beta_arr) a.beta_arr = whole.beta_arr + 2 * sl.first_pair;
    a.pair0 = whole.pair0 + (uint64_t)sl.first_pair;
    a.n_chains = sl.n_chains;
    a.full_rounds = sl.full_rounds;
    a.tail_pairs = sl.tail_pairs;
    return a;
}

// n single-sweep launches of every slice, back to back on the slice's stream: one fork behind what the handle's stream holds, one
// join per side stream at the end, so whatever is queued on the handle's stream afterwards finds every slice finished.
static int sweep_launches_sliced(amc_handle* h, int64_t n_launches, const amc::SlicePlan& plan)
{
    AMC_TRY(pg_resolve(h));
    AMC_TRY(counter_room(h, "amc_sweep_launches", (uint64_t)n_launches));
    if (h->knobs.debug_plan)
        for (int s = 0; s < plan.count; ++s)
            std::fprintf(stderr, "[amc] sweep slice %d of %d: pairs from %lld, %lld chains in a grid of %d blocks\n", s, plan.count,
                         (long long)plan.s[s].first_pair, (long long)plan.s[s].n_chains, plan.s[s].grid);
    const amc::SweepArgs whole = make_sweep_args(h, 1, 0);
    AMC_HIP(hipEventRecord(h->slice_fork, h->stream));
    int rc = AMC_OK;
    hipError_t err = hipSuccess;
    auto note = [&](hipError_t e) { if (e != hipSuccess && err == hipSuccess) err = e; };
    amc::SweepArgs a[amc::AMC_MAX_SLICES];
    hipStream_t stream[amc::AMC_MAX_SLICES];
    for (int s = 0; s < plan.count; ++s) {
        a[s] = slice_sweep_args(whole, plan.s[s]);
        stream[s] = s == 0 ? h->stream : h->slice_stream[s - 1];
        if (s > 0) note(hipStreamWaitEvent(stream[s], h->slice_fork, 0));
    }
    // step by step on the host, so that the slices' queues fill together; on the device each stream runs its launches back to back,
    // with no event between the steps
    for (int64_t i = 0; i < n_launches && rc == AMC_OK && err == hipSuccess; ++i)
        for (int s = 0; s < plan.count && rc == AMC_OK; ++s) {
            a[s].t0 = h->t + (uint64_t)i;
            rc = h->potential == AMC_POTENTIAL_DOUBLE_WELL ? launch_sweep<amc::POT_DOUBLE_WELL>(h, a[s], plan.s[s].grid, false, stream[s])
                                                           : launch_sweep<amc::POT_HARMONIC>(h, a[s], plan.s[s].grid, false, stream[s]);
        }
    // the joins come whatever happened: nothing of this call may still run when the handle's stream goes on
    for (int s = 1; s < plan.count; ++s) {
        note(hipEventRecord(h->slice_join[s - 1], stream[s]));
        note(hipStreamWaitEvent(h->stream, h->slice_join[s - 1], 0));
    }
    if (rc != AMC_OK) return rc;
    AMC_HIP(err);
    h->t += (uint64_t)n_launches;
    h->t_counted += (uint64_t)n_launches;
    return AMC_OK;
}

extern "C" {

int amc_sweep(amc_handle* h, int64_t n_sweeps)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_sweep: NULL handle");
    if (n_sweeps < 0) return fail(AMC_ERR_BAD_ARG, "amc_sweep: n_sweeps < 0");
    if (n_sweeps == 0) return AMC_OK;
    return sweep_impl(h, n_sweeps, false, nullptr);
}

int amc_sweep_launches(amc_handle* h, int64_t n_launches)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_sweep_launches: NULL handle");
    if (n_launches < 0) return fail(AMC_ERR_BAD_ARG, "amc_sweep_launches: n_launches < 0");
    {
        const amc::SlicePlan plan = sliced_route_plan(h, n_launches);
        if (plan.count > 1) {
            AMC_HIP(hipSetDevice(h->device));
            if (slice_streams_ready(h, plan.count - 1)) return sweep_launches_sliced(h, n_launches, plan);
        }
    }
    for (int64_t i = 0; i < n_launches; ++i) {
        AMC_TRY(sweep_impl(h, 1, false, nullptr));
    }
    return AMC_OK;
}

}  // extern "C"
