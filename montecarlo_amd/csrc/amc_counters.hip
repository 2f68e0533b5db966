// amc_counters.hip -- the step log and the per-chain counters: folding the log into the counters, pool totals, the carry into
// 64-bit bases, and the counters' upload / download (amc_download_counters, amc_counter_totals, amc_upload_counters,
// amc_set_counter_totals).
#define AMC_KERNEL_LINKAGE static      // the plain kernels are amc_api.hip's: this object launches template instantiations only
#include "amc_internal.h"

// The step log's form (store_log_pair): none without per-chain counters, two chains per byte while the move index fits three
// bits, one byte per chain beyond.
int log_form(const amc_handle* h)
{
    return !h->counters ? AMC_LOG_NONE : (h->K <= AMC_PACKED_LOG_MOVES ? AMC_LOG_PACKED : AMC_LOG_BYTES);
}

// Adds the pending rows of the step log into the per-chain counters (on the stream).  Everything that reads or
// replaces d_acc / d_tot calls this first.
// with_ratio (K <= 4): the launch also leaves callback_acceptance's per-move sums as block partials in h_ratio
// (rows = its grid; *ratio_rows receives the count) and runs even when no log row is pending.
// (Round 3 measured the callback's fold on a second stream beside the sweeps queued after it, the log a ring of rows:
// no gain -- config 3: 37.3 against 37.6 us per time step with the callback read a period late, 41.0 against 38.9 read at
// once; config 5: 72.7 against 70.7 either way.  The fold's waves do not fit beside five 96-register waves of the fused
// kernel, so they take whole wave slots from it, and the cross-stream events cost more than the overlap returns.)
int fold_log(amc_handle* h, bool with_ratio, int* ratio_rows, amc::xs_word* ratio_dst)
{
    if (!h->d_log || (h->log_fill == 0 && !with_ratio)) return AMC_OK;
    // tiles of AMC_FOLD_TILE chains, dealt evenly: every block takes the same number of tiles (a grid of 2048 over 2442
    // tiles would leave 80 % of the blocks idle for the second half of the launch)
    const int64_t n_tiles = (h->M + AMC_FOLD_TILE - 1) / AMC_FOLD_TILE;
    const int64_t cap = (int64_t)h->n_cu * h->blocks_per_cu;
    const int64_t rounds = (n_tiles + cap - 1) / cap;
    const int grid = (int)((n_tiles + rounds - 1) / rounds);
    uint16_t* const no_hi = nullptr;
#define AMC_FOLD_W(KS, RATIO)                                                                                         \
    hipLaunchKernelGGL((amc::fold_log_kernel<KS, RATIO, uint32_t, false>), dim3(grid), dim3(AMC_BLOCK), 0, h->stream, \
                       h->d_log, h->log_fill, h->d_acc, h->d_tot, no_hi, no_hi, h->M, h->M_pad, 0, h->t_counted, ratio_dst, RATIO_STRIDE)
#define AMC_FOLD_N(KS, RATIO, HIGH)                                                                                   \
    hipLaunchKernelGGL((amc::fold_log_kernel<KS, RATIO, uint16_t, HIGH>), dim3(grid), dim3(AMC_BLOCK), 0, h->stream, \
                       h->d_log, h->log_fill, h->d_acc16, h->d_tot16, h->d_acc_hi, h->d_tot_hi, h->M, h->M_pad, 0, h->t_counted, \
                       ratio_dst, RATIO_STRIDE)
#define AMC_FOLD(KS, RATIO)                                                                                           \
    do {                                                                                                              \
        if (!h->narrow) AMC_FOLD_W(KS, RATIO);                                                                        \
        else if (h->use_high) AMC_FOLD_N(KS, RATIO, true);                                                            \
        else AMC_FOLD_N(KS, RATIO, false);                                                                            \
    } while (0)
    if (with_ratio) {
        switch (h->K) {
        case 1: AMC_FOLD(1, true); break;
        case 2: AMC_FOLD(2, true); break;
        case 3: AMC_FOLD(3, true); break;
        case 4: AMC_FOLD(4, true); break;
        default: return fail(AMC_ERR_STATE, "fold_log: ratio sums ride on the K <= 4 fold only");
        }
        if (ratio_rows) *ratio_rows = grid;
    } else {
        switch (h->K) {
        case 1: AMC_FOLD(1, false); break;
        case 2: AMC_FOLD(2, false); break;
        case 3: AMC_FOLD(3, false); break;
        case 4: AMC_FOLD(4, false); break;
        default: {
            // more than four moves: ceil(K / 4) passes of the four-move form, one per group of moves (fold_log_kernel<.., GROUP>)
            const bool bytes = log_form(h) == AMC_LOG_BYTES;
            const int n_groups = (h->K + 3) / 4;
#define AMC_FOLD_GROUP(KS, GROUP, BYTES)                                                                              \
    hipLaunchKernelGGL((amc::fold_log_kernel<KS, false, uint32_t, false, GROUP, BYTES>), dim3(grid), dim3(AMC_BLOCK), 0, h->stream, \
                       h->d_log, h->log_fill, acc_g, tot_g, no_hi, no_hi, h->M, h->M_pad, g, h->t_counted, ratio_dst, RATIO_STRIDE)
#define AMC_FOLD_GROUPS(BYTES)                                                                                        \
    for (int g = 0; g < n_groups; ++g) {                                                                              \
        uint32_t* const acc_g = h->d_acc + 4 * (size_t)g * (size_t)h->M_pad;                                          \
        uint32_t* const tot_g = h->d_tot + 4 * (size_t)g * (size_t)h->M_pad;                                          \
        if (g + 1 < n_groups) AMC_FOLD_GROUP(4, 1, BYTES);                                                            \
        else switch (h->K - 4 * g) {                                                                                  \
            case 1: AMC_FOLD_GROUP(1, 2, BYTES); break;                                                               \
            case 2: AMC_FOLD_GROUP(2, 2, BYTES); break;                                                               \
            case 3: AMC_FOLD_GROUP(3, 2, BYTES); break;                                                               \
            default: AMC_FOLD_GROUP(4, 2, BYTES); break;                                                              \
        }                                                                                                             \
    }
            if (bytes) { AMC_FOLD_GROUPS(true) } else { AMC_FOLD_GROUPS(false) }
#undef AMC_FOLD_GROUPS
#undef AMC_FOLD_GROUP
            break;
        }
        }
    }
#undef AMC_FOLD
#undef AMC_FOLD_N
#undef AMC_FOLD_W
    AMC_HIP(hipGetLastError());
    h->log_fill = 0;
    return AMC_OK;
}

// Allocates the per-chain counter arrays, zeroed: two u16 planes per counter (narrow) or u32 arrays.
hipError_t alloc_counters(amc_handle* h, bool narrow)
{
    const size_t n = (size_t)h->K * (size_t)h->M_pad;
    const size_t nt = (size_t)(h->K - 1) * (size_t)h->M_pad;      // K - 1 rows: the last move's total_calls is the step count
    h->narrow = narrow;                                            // minus the others (fold_log_kernel)
    h->use_high = false;
    auto zeroed = [&](void** p, size_t bytes) {
        if (bytes == 0) return hipSuccess;
        const hipError_t e = hipMalloc(p, bytes);
        return e != hipSuccess ? e : hipMemsetAsync(*p, 0, bytes, h->stream);
    };
    hipError_t e;
    if (!narrow) {
        if ((e = zeroed((void**)&h->d_acc, n * sizeof(uint32_t))) != hipSuccess) return e;
        return zeroed((void**)&h->d_tot, nt * sizeof(uint32_t));
    }
    if ((e = zeroed((void**)&h->d_acc16, n * sizeof(uint16_t))) != hipSuccess) return e;
    if ((e = zeroed((void**)&h->d_acc_hi, n * sizeof(uint16_t))) != hipSuccess) return e;
    if ((e = zeroed((void**)&h->d_tot16, nt * sizeof(uint16_t))) != hipSuccess) return e;
    return zeroed((void**)&h->d_tot_hi, nt * sizeof(uint16_t));
}

// Makes room for at least one more row of the step log (a full log is folded first); *rows = how many fit.
int log_room(amc_handle* h, int* rows)
{
    if (h->log_fill == h->log_depth) {
        AMC_TRY(fold_log(h));
    }
    *rows = h->log_depth - h->log_fill;
    return AMC_OK;
}

// Pool-wide accepted total (K == 1): sum of the per-block slots the sweep kernel maintains.
static int sum_acc_slots(amc_handle* h, unsigned long long* out)
{
    std::vector<unsigned long long> slots((size_t)h->n_slots);
    AMC_HIP(hipMemcpyAsync(slots.data(), h->d_acc_slots, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));
    unsigned long long t = 0;
    for (unsigned long long v : slots) t += v;
    *out = t;
    return AMC_OK;
}

// pool totals of the counter ARRAYS (K > 1; without their 64-bit bases): host[k] accepted, host[AMC_MAX_MOVES + k] total of move k < K - 1
static int array_totals(amc_handle* h, unsigned long long (&host)[2 * AMC_MAX_MOVES])
{
    AMC_TRY(fold_log(h));
    if (h->K > 1) {
        AMC_HIP(hipMemsetAsync(h->d_totals, 0, 2 * AMC_MAX_MOVES * sizeof(unsigned long long), h->stream));
        if (h->narrow)
            hipLaunchKernelGGL(amc::counter_totals_kernel<uint16_t>, dim3(grid_for(h, (h->M + 3) / 4)), dim3(AMC_BLOCK), 0, h->stream,
                               h->d_acc16, h->d_tot16, h->use_high ? h->d_acc_hi : nullptr, h->use_high ? h->d_tot_hi : nullptr, h->M,
                               h->M_pad, h->K, h->d_totals, h->d_totals + AMC_MAX_MOVES);
        else
            hipLaunchKernelGGL(amc::counter_totals_kernel<uint32_t>, dim3(grid_for(h, (h->M + 3) / 4)), dim3(AMC_BLOCK), 0, h->stream,
                               h->d_acc, h->d_tot, (const uint16_t*)nullptr, (const uint16_t*)nullptr, h->M, h->M_pad, h->K, h->d_totals,
                               h->d_totals + AMC_MAX_MOVES);
        AMC_HIP(hipGetLastError());
    }
    AMC_HIP(hipMemcpyAsync(host, h->d_totals, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));
    return AMC_OK;
}

// Carries the 32-bit counter arrays into their 64-bit bases and restarts them at zero (see counter_rebase_kernel): pending log
// rows are folded first, the pool totals of what is carried are kept on the host (amc_counter_totals), and a handle with u16
// planes goes on with u32 arrays -- the same bytes per counter, and the pass that forms the acceptance ratios from arrays plus
// bases (reduce_kernel) reads those.
static int counter_rebase(amc_handle* h)
{
    unsigned long long host[2 * AMC_MAX_MOVES];
    AMC_TRY(array_totals(h, host));         // folds the log
    const size_t n = (size_t)h->K * (size_t)h->M_pad, nt = (size_t)(h->K - 1) * (size_t)h->M_pad;
    if (!h->d_acc_base) {
        AMC_HIP(hipMalloc(&h->d_acc_base, n * sizeof(unsigned long long)));
        AMC_HIP(hipMemsetAsync(h->d_acc_base, 0, n * sizeof(unsigned long long), h->stream));
        if (nt) {
            AMC_HIP(hipMalloc(&h->d_tot_base, nt * sizeof(unsigned long long)));
            AMC_HIP(hipMemsetAsync(h->d_tot_base, 0, nt * sizeof(unsigned long long), h->stream));
        }
    }
    const int grid = grid_for(h, (int64_t)n);
    if (h->narrow) {
        hipLaunchKernelGGL(amc::counter_rebase_kernel<uint16_t>, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, h->d_acc16,
                           h->use_high ? h->d_acc_hi : nullptr, (int64_t)n, h->d_acc_base);
        if (nt) hipLaunchKernelGGL(amc::counter_rebase_kernel<uint16_t>, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, h->d_tot16,
                                   h->use_high ? h->d_tot_hi : nullptr, (int64_t)nt, h->d_tot_base);
    } else {
        hipLaunchKernelGGL(amc::counter_rebase_kernel<uint32_t>, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, h->d_acc, (uint16_t*)nullptr,
                           (int64_t)n, h->d_acc_base);
        if (nt) hipLaunchKernelGGL(amc::counter_rebase_kernel<uint32_t>, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, h->d_tot,
                                   (uint16_t*)nullptr, (int64_t)nt, h->d_tot_base);
    }
    AMC_HIP(hipGetLastError());
    if (h->narrow) {                 // u32 arrays from here on
        AMC_HIP(hipStreamSynchronize(h->stream));
        (void)hipFree(h->d_acc16); (void)hipFree(h->d_tot16); (void)hipFree(h->d_acc_hi); (void)hipFree(h->d_tot_hi);
        h->d_acc16 = h->d_tot16 = h->d_acc_hi = h->d_tot_hi = nullptr;
        const hipError_t e = alloc_counters(h, false);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? AMC_ERR_OOM : AMC_ERR_HIP, "counter_rebase: %s", hipGetErrorString(e));
    }
    if (h->K > 1)
        for (int k = 0; k < h->K; ++k) {
            h->base_acc_total[k] += host[k];
            if (k + 1 < h->K) h->base_tot_total[k] += host[AMC_MAX_MOVES + k];
        }
    h->t_base += h->t_counted;
    h->t_counted = 0;
    h->use_high = false;
    return AMC_OK;
}

// Move.accepted_calls / total_calls are Int (Int64) in the reference (src/metropolis.jl:145-146); the per-chain arrays on
// the device count in 32 bits.  No chain's counter can exceed the number of counted steps, so before the launch that would take
// that number past 2^32 - 1 the arrays are carried into 64-bit bases (counter_rebase) and the count goes on -- round 5; until
// round 4 that call was refused.  `steps`: what the next LAUNCH counts (at most 2^20).  The pool-wide counter of a K = 1 handle
// without per-chain counters is 64-bit anyway.
// Handles with u16 planes bring the high planes into play here, before the call that would count past 65 535 steps (rows
// still waiting in the log are then folded by the carrying form as well: it starts from high halves that are zero).
int counter_room(amc_handle* h, const char* who, uint64_t steps)
{
    (void)who;
    if (!h->counters) return AMC_OK;
    if (h->t_counted + steps > 0xFFFFFFFFull) {
        AMC_TRY(counter_rebase(h));
    }
    if (h->narrow && h->t_counted + steps > 0xFFFFull) h->use_high = true;
    return AMC_OK;
}

// The totals per (move, rung) queued into d_rung_cnt -- accepted[K R] then total[K R], the last move's total cells left at zero (it has
// no total array; amc_rung_counter_totals completes it on the host, rung_sigma_tune_kernel on the device) -- behind a fold of the
// pending log rows.  Nothing is read back.  The caller has checked the ladder and the counters and set the device.
int rung_totals_queue(amc_handle* h)
{
    AMC_TRY(fold_log(h));
    const int R = h->lad.n_rungs;
    const size_t cells = (size_t)h->K * (size_t)R;
    if (cells > h->lad.rung_cnt_cells) {
        AMC_HIP(hipStreamSynchronize(h->stream));               // (nothing queued reads the old cells after this call's predecessor returned)
        (void)hipFree(h->lad.d_rung_cnt);
        h->lad.d_rung_cnt = nullptr;
        h->lad.rung_cnt_cells = 0;
        AMC_HIP(hipMalloc(&h->lad.d_rung_cnt, 2 * cells * sizeof(unsigned long long)));
        h->lad.rung_cnt_cells = cells;
    }
    unsigned long long* out_acc = h->lad.d_rung_cnt;
    unsigned long long* out_tot = h->lad.d_rung_cnt + cells;
    AMC_HIP(hipMemsetAsync(h->lad.d_rung_cnt, 0, 2 * cells * sizeof(unsigned long long), h->stream));
    const int grid = grid_for(h, h->M);
    if (h->narrow)
        hipLaunchKernelGGL(amc::rung_counter_totals_kernel<uint16_t>, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, (const uint16_t*)h->d_acc16,
                           (const uint16_t*)h->d_tot16, (const uint16_t*)(h->use_high ? h->d_acc_hi : nullptr),
                           (const uint16_t*)(h->use_high ? h->d_tot_hi : nullptr), (const unsigned long long*)h->d_acc_base,
                           (const unsigned long long*)h->d_tot_base, h->M, h->M_pad, h->K, R, out_acc, out_tot);
    else
        hipLaunchKernelGGL(amc::rung_counter_totals_kernel<uint32_t>, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, (const uint32_t*)h->d_acc,
                           (const uint32_t*)h->d_tot, (const uint16_t*)nullptr, (const uint16_t*)nullptr, (const unsigned long long*)h->d_acc_base,
                           (const unsigned long long*)h->d_tot_base, h->M, h->M_pad, h->K, R, out_acc, out_tot);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

extern "C" {

int amc_download_counters(amc_handle* h, int64_t* accepted, int64_t* total)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_download_counters: NULL handle");
    if (!h->counters)
        return fail(AMC_ERR_STATE, "amc_download_counters: handle was created with per_chain_counters = 0");
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(fold_log(h));
    std::vector<uint32_t> buf((size_t)h->M);
    // one row of counters, whatever their width on the device, as int64
    auto fetch_row = [&](const uint32_t* wide, const uint16_t* narrow, const uint16_t* high, int k, int64_t* out) -> int {
        if (h->narrow) {
            uint16_t* b16 = reinterpret_cast<uint16_t*>(buf.data());
            AMC_HIP(hipMemcpyAsync(b16, narrow + (size_t)k * h->M_pad, (size_t)h->M * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
            AMC_HIP(hipStreamSynchronize(h->stream));
            for (int64_t c = 0; c < h->M; ++c) out[c] = b16[(size_t)c];
            if (h->use_high) {
                AMC_HIP(hipMemcpyAsync(b16, high + (size_t)k * h->M_pad, (size_t)h->M * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
                AMC_HIP(hipStreamSynchronize(h->stream));
                for (int64_t c = 0; c < h->M; ++c) out[c] |= (int64_t)b16[(size_t)c] << 16;
            }
        } else {
            AMC_HIP(hipMemcpyAsync(buf.data(), wide + (size_t)k * h->M_pad, (size_t)h->M * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
            AMC_HIP(hipStreamSynchronize(h->stream));
            for (int64_t c = 0; c < h->M; ++c) out[c] = buf[(size_t)c];
        }
        return AMC_OK;
    };
    // what the arrays have been carried into (counter_rebase): 64-bit bases, added in
    std::vector<unsigned long long> bbuf(h->d_acc_base ? (size_t)h->M : 0);
    auto add_base = [&](const unsigned long long* base, int k, int64_t* out) -> int {
        if (!base) return AMC_OK;
        AMC_HIP(hipMemcpyAsync(bbuf.data(), base + (size_t)k * h->M_pad, (size_t)h->M * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        AMC_HIP(hipStreamSynchronize(h->stream));
        for (int64_t c = 0; c < h->M; ++c) out[c] += (int64_t)bbuf[(size_t)c];
        return AMC_OK;
    };
    for (int k = 0; k < h->K; ++k) {
        if (accepted) {
            int rc = fetch_row(h->d_acc, h->d_acc16, h->d_acc_hi, k, accepted + (int64_t)k * h->M);
            if (rc == AMC_OK) rc = add_base(h->d_acc_base, k, accepted + (int64_t)k * h->M);
            if (rc != AMC_OK) return rc;
        }
        if (total) {
            if (k + 1 < h->K) {
                int rc = fetch_row(h->d_tot, h->d_tot16, h->d_tot_hi, k, total + (int64_t)k * h->M);
                if (rc == AMC_OK) rc = add_base(h->d_tot_base, k, total + (int64_t)k * h->M);
                if (rc != AMC_OK) return rc;
            } else {
                // the last move: every chain has taken the same number of steps, its total_calls is what the other moves left
                for (int64_t c = 0; c < h->M; ++c) {
                    int64_t others = 0;
                    for (int j = 0; j + 1 < h->K; ++j) others += total[(int64_t)j * h->M + c];
                    total[(int64_t)k * h->M + c] = (int64_t)(h->t_base + h->t_counted) - others;
                }
            }
        }
    }
    return AMC_OK;
}

int amc_counter_totals(amc_handle* h, int64_t* accepted, int64_t* total)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_counter_totals: NULL handle");
    AMC_HIP(hipSetDevice(h->device));
    unsigned long long host[2 * AMC_MAX_MOVES];
    AMC_TRY(array_totals(h, host));
    if (h->K == 1) {
        unsigned long long acc = 0;
        AMC_TRY(sum_acc_slots(h, &acc));         // (the pool-wide slots are 64-bit and never carried)
        host[0] = acc;
    }
    unsigned long long others = 0;
    for (int k = 0; k < h->K; ++k) {
        if (accepted) accepted[k] = (int64_t)(host[k] + (h->K > 1 ? h->base_acc_total[k] : 0ull));
        // the last move's total: all counted steps of all chains minus the other moves' (its per-chain array does not exist)
        const unsigned long long tk = (k + 1 < h->K) ? host[AMC_MAX_MOVES + k] + h->base_tot_total[k]
                                                     : (h->t_base + h->t_counted) * (uint64_t)h->M - others;
        others += tk;
        if (total) total[k] = (int64_t)tk;
    }
    return AMC_OK;
}

int amc_rung_counter_totals(amc_handle* h, int64_t* accepted, int64_t* total)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_rung_counter_totals: NULL handle");
    AMC_TRY(need_ladder(h, "amc_rung_counter_totals"));
    if (!h->counters) return fail(AMC_ERR_STATE, "amc_rung_counter_totals: handle was created with per_chain_counters = 0");
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(rung_totals_queue(h));
    const int R = h->lad.n_rungs;
    const size_t cells = (size_t)h->K * (size_t)R;
    std::vector<unsigned long long> host(2 * cells);
    AMC_TRY(copy_to_host_sync(h, host.data(), h->lad.d_rung_cnt, 2 * cells * sizeof(unsigned long long)));
    // the last move's total: every chain of a rung has taken all counted steps, what the other moves left is its own
    const unsigned long long steps_per_rung = (h->t_base + h->t_counted) * (uint64_t)(h->M / R);
    for (int r = 0; r < R; ++r) {
        unsigned long long others = 0;
        for (int k = 0; k < h->K; ++k) {
            const size_t e = (size_t)k * (size_t)R + (size_t)r;
            const unsigned long long tk = (k + 1 < h->K) ? host[cells + e] : steps_per_rung - others;
            others += tk;
            if (accepted) accepted[e] = (int64_t)host[e];
            if (total) total[e] = (int64_t)tk;
        }
    }
    return AMC_OK;
}

int amc_upload_counters(amc_handle* h, const int64_t* accepted, const int64_t* total)
{
    if (!h || !accepted) return fail(AMC_ERR_BAD_ARG, "amc_upload_counters: NULL argument");
    if (!h->counters)
        return fail(AMC_ERR_STATE, "amc_upload_counters: handle was created with per_chain_counters = 0 "
                                   "(use amc_set_counter_totals)");
    if (h->K > 1 && !total) return fail(AMC_ERR_BAD_ARG, "amc_upload_counters: total is required when K > 1");
    // Every chain takes the same number of MH steps (mc_sweep!, metropolis.jl:205-210), so sum_k total_calls_ck is ONE number
    // for all chains: the count of steps taken.  The device keeps that number and K - 1 of the K total arrays.
    const int64_t LIMIT = (int64_t)1 << 52;          // counts are divided as Float64s (callback_acceptance): exact below 2^53
    uint64_t steps = h->t_base + h->t_counted;
    if (total) {
        for (int64_t c = 0; c < h->M; ++c) {
            int64_t sum = 0;
            for (int k = 0; k < h->K; ++k) {
                const int64_t v = total[(int64_t)k * h->M + c];
                if (v < 0 || v > LIMIT) return fail(AMC_ERR_BAD_ARG, "amc_upload_counters: counter out of range [0, 2^52]");
                sum += v;
            }
            if (c == 0) steps = (uint64_t)sum;
            else if ((uint64_t)sum != steps)
                return fail(AMC_ERR_BAD_ARG, "amc_upload_counters: the total_calls of a chain must add up to the same step count on "
                                             "every chain (chain 0: %llu, chain %lld: %lld)", (unsigned long long)steps, (long long)c, (long long)sum);
        }
        if (steps > (uint64_t)LIMIT) return fail(AMC_ERR_BAD_ARG, "amc_upload_counters: step count out of range [0, 2^52]");
    }
    int64_t acc_max = 0;
    for (int64_t i = 0; i < (int64_t)h->K * h->M; ++i) {
        if (accepted[i] < 0 || accepted[i] > LIMIT) return fail(AMC_ERR_BAD_ARG, "amc_upload_counters: counter out of range [0, 2^52]");
        acc_max = std::max(acc_max, accepted[i]);
    }
    AMC_HIP(hipSetDevice(h->device));
    if (steps > 0xFFFFFFFFull || (uint64_t)acc_max > 0xFFFFFFFFull || h->d_acc_base) {
        // counts beyond 32 bits (or a handle that has carried before): everything goes into the 64-bit bases, the arrays restart
        // at zero (counter_rebase does the allocating and the switch to u32 arrays; what it carries is overwritten next)
        h->log_fill = 0;
        AMC_TRY(counter_rebase(h));
        std::vector<unsigned long long> b((size_t)h->M);
        for (int k = 0; k < h->K; ++k) {
            h->base_acc_total[k] = h->base_tot_total[k] = 0ull;
            for (int pass = 0; pass < 2; ++pass) {
                const int64_t* src = pass == 0 ? accepted : total;
                if (!src || (pass == 1 && k + 1 == h->K)) continue;
                unsigned long long sum = 0;
                for (int64_t c = 0; c < h->M; ++c) { b[(size_t)c] = (unsigned long long)src[(int64_t)k * h->M + c]; sum += b[(size_t)c]; }
                (pass == 0 ? h->base_acc_total[k] : h->base_tot_total[k]) = sum;
                unsigned long long* dst = (pass == 0 ? h->d_acc_base : h->d_tot_base) + (size_t)k * h->M_pad;
                AMC_HIP(hipMemcpyAsync(dst, b.data(), (size_t)h->M * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
                AMC_HIP(hipStreamSynchronize(h->stream));
            }
        }
        if (h->K == 1) {
            const unsigned long long acc_sum = h->base_acc_total[0];
            AMC_HIP(hipMemsetAsync(h->d_acc_slots, 0, (size_t)h->n_slots * sizeof(unsigned long long), h->stream));
            AMC_HIP(hipMemcpyAsync(h->d_acc_slots, &acc_sum, sizeof(acc_sum), hipMemcpyHostToDevice, h->stream));
            AMC_HIP(hipStreamSynchronize(h->stream));
        }
        h->t_base = steps;
        h->t_counted = 0;
        return AMC_OK;
    }
    // (the handle's own bookkeeping -- log_fill, use_high, t_counted -- changes only once every plane has been copied: a copy
    // that fails leaves the handle counting as before)
    std::vector<uint32_t> buf((size_t)h->M);
    unsigned long long acc_sum = 0;
    for (int k = 0; k < h->K; ++k) {
        for (int pass = 0; pass < 2; ++pass) {
            const int64_t* src = pass == 0 ? accepted : total;
            if (!src || (pass == 1 && k + 1 == h->K)) continue;             // the last move's totals have no array
            uint16_t* b16 = reinterpret_cast<uint16_t*>(buf.data());
            for (int64_t c = 0; c < h->M; ++c) {
                const int64_t v = src[(int64_t)k * h->M + c];
                if (h->narrow) b16[(size_t)c] = (uint16_t)(v & 0xFFFF); else buf[(size_t)c] = (uint32_t)v;
                if (pass == 0) acc_sum += (unsigned long long)v;
            }
            if (h->narrow) {
                uint16_t* dst = (pass == 0 ? h->d_acc16 : h->d_tot16) + (size_t)k * h->M_pad;
                AMC_HIP(hipMemcpyAsync(dst, b16, (size_t)h->M * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
                AMC_HIP(hipStreamSynchronize(h->stream));
                for (int64_t c = 0; c < h->M; ++c) b16[(size_t)c] = (uint16_t)(src[(int64_t)k * h->M + c] >> 16);
                dst = (pass == 0 ? h->d_acc_hi : h->d_tot_hi) + (size_t)k * h->M_pad;
                AMC_HIP(hipMemcpyAsync(dst, b16, (size_t)h->M * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
            } else {
                uint32_t* dst = (pass == 0 ? h->d_acc : h->d_tot) + (size_t)k * h->M_pad;
                AMC_HIP(hipMemcpyAsync(dst, buf.data(), (size_t)h->M * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            }
            AMC_HIP(hipStreamSynchronize(h->stream));
        }
    }
    if (h->K == 1) {
        AMC_HIP(hipMemsetAsync(h->d_acc_slots, 0, (size_t)h->n_slots * sizeof(unsigned long long), h->stream));
        AMC_HIP(hipMemcpyAsync(h->d_acc_slots, &acc_sum, sizeof(acc_sum), hipMemcpyHostToDevice, h->stream));
        AMC_HIP(hipStreamSynchronize(h->stream));
    }
    h->log_fill = 0;            // every counter is replaced: steps still waiting in the log are dropped with the old values
    // u16 planes: the high halves take part from now on unless no counter can have reached 2^16 (see counter_room); both
    // planes are always written, so that halves which do not take part yet are zero when they do
    if (h->narrow) h->use_high = steps > 0xFFFFull || (uint64_t)acc_max > steps;
    h->t_counted = steps;
    return AMC_OK;
}

int amc_set_counter_totals(amc_handle* h, const int64_t* accepted, uint64_t steps_counted)
{
    if (!h || !accepted) return fail(AMC_ERR_BAD_ARG, "amc_set_counter_totals: NULL argument");
    if (h->K != 1 || h->counters)
        return fail(AMC_ERR_STATE, "amc_set_counter_totals: only for K = 1 handles without per-chain counters");
    if (accepted[0] < 0) return fail(AMC_ERR_BAD_ARG, "amc_set_counter_totals: negative count");
    AMC_HIP(hipSetDevice(h->device));
    const unsigned long long acc = (unsigned long long)accepted[0];
    AMC_HIP(hipMemsetAsync(h->d_acc_slots, 0, (size_t)h->n_slots * sizeof(unsigned long long), h->stream));
    AMC_HIP(hipMemcpyAsync(h->d_acc_slots, &acc, sizeof(acc), hipMemcpyHostToDevice, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));
    h->t_counted = steps_counted;
    return AMC_OK;
}

}  // extern "C"
