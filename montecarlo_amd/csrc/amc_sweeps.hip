// amc_sweeps.hip -- sweep launches: n_sweeps x sweepstep MH steps in launches of at most 2^20 steps (amc_sweep, amc_sweep_launches),
// the last of them forming the callback sums when asked (sweep_impl, for amc_sweep_reduce_begin).
#define AMC_KERNEL_LINKAGE static      // the plain kernels are amc_api.hip's: this object launches template instantiations only
#include "amc_internal.h"

// sweep_kernel<POT, MULTI, LOG, BETA, SINGLE, FORM>, BETA the handle's (an array of betas or one)
template <int POT, bool MULTI, int LOG, bool SINGLE, int FORM>
int launch_sweep_beta(amc_handle* h, const amc::SweepArgs& a, int grid)
{
    if (h->beta_arr)
        hipLaunchKernelGGL((amc::sweep_kernel<POT, MULTI, LOG, true, SINGLE, FORM>), dim3(grid), dim3(AMC_BLOCK), 0, h->stream, a);
    else
        hipLaunchKernelGGL((amc::sweep_kernel<POT, MULTI, LOG, false, SINGLE, FORM>), dim3(grid), dim3(AMC_BLOCK), 0, h->stream, a);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

template <int POT, int FORM>
int launch_sweep_form(amc_handle* h, const amc::SweepArgs& a, int grid)
{
#define AMC_SWEEP(MULTI, LOG)                                                                                                 \
    (a.n_steps == 1 ? launch_sweep_beta<POT, MULTI, LOG, true, FORM>(h, a, grid) : launch_sweep_beta<POT, MULTI, LOG, false, FORM>(h, a, grid))
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
int launch_sweep(amc_handle* h, const amc::SweepArgs& a, int grid, bool reduce)
{
    if (!reduce) return launch_sweep_form<POT, amc::RED_FORM_NONE>(h, a, grid);
    return red_form(h) == amc::RED_FORM_E ? launch_sweep_form<POT, amc::RED_FORM_E>(h, a, grid) : launch_sweep_form<POT, amc::RED_FORM_COLS>(h, a, grid);
}

static const char* tf(bool b) { return b ? "true" : "false"; }

// sweep_kernel<POT_CUSTOM, MULTI, LOG, BETA, SINGLE, REDUCE> with the flags launch_sweep picks
static int launch_sweep_custom(amc_handle* h, amc::SweepArgs& a, int grid, bool reduce)
{
    const bool multi = h->K > 1;
    const std::string inst = "amc::sweep_kernel<" + std::to_string(h->potential) + "," + tf(multi) + "," + std::to_string(log_form(h)) + "," + tf(h->beta_arr) + "," +
                             tf(a.n_steps == 1) + "," + std::to_string(reduce ? red_form(h) : (int)amc::RED_FORM_NONE) + ">";
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
    { const int rc = pg_resolve(h); if (rc != AMC_OK) return rc; }      // the sweep kernels read sigma from the parameter table
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
            const int rc = log_room(h, &room);
            if (rc != AMC_OK) return rc;
            if (chunk > room) chunk = room;
        }
        { const int rc = counter_room(h, "amc_sweep", (uint64_t)chunk); if (rc != AMC_OK) return rc; }      // (may carry the counters: arrays restart at zero)
        amc::SweepArgs a = make_sweep_args(h, chunk, grid);
        a.red_stride = red_row_stride(h, grid);
        const bool last = remaining == chunk;
        const bool reduce = fuse_reduce && last;
        const int rc = h->use_rtc ? launch_sweep_custom(h, a, grid, reduce)
                       : (h->potential == AMC_POTENTIAL_DOUBLE_WELL) ? launch_sweep<amc::POT_DOUBLE_WELL>(h, a, grid, reduce)
                                                                     : launch_sweep<amc::POT_HARMONIC>(h, a, grid, reduce);
        if (rc != AMC_OK) return rc;
        h->t += (uint64_t)chunk;
        h->t_counted += (uint64_t)chunk;
        if (h->d_log) h->log_fill += chunk;
        remaining -= chunk;
    }
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
    for (int64_t i = 0; i < n_launches; ++i) {
        const int rc = sweep_impl(h, 1, false, nullptr);
        if (rc != AMC_OK) return rc;
    }
    return AMC_OK;
}

}  // extern "C"
