// amc_reduce.hip -- callback reductions: the tickets of the sums in flight (amc_reduce_begin / _end, the sums a sweep launch forms
// on its way: amc_sweep_reduce_begin), their records, and the host-side arithmetic on records (amc_xsum_*).
#define AMC_KERNEL_LINKAGE static      // the plain kernels are amc_api.hip's: this object launches template instantiations only
#include "amc_internal.h"

// The form of a launch that also leaves the callback sums (amc::RED_FORM_*): the one with sum e alone compiled in when the
// callbacks read nothing else (amc_set_reduce_columns; harmonic potential, Float64 state: sum x^2 is the same sum), else the one
// that forms whatever SweepArgs.red_cols names.
int red_form(const amc_handle* h)
{
    const int e_alone = (h->potential == AMC_POTENTIAL_HARMONIC && !h->f32) ? (amc::RED_WANT_E | amc::RED_WANT_XX) : amc::RED_WANT_E;
    return (h->red_cols & ~e_alone) == 0 ? amc::RED_FORM_E : amc::RED_FORM_COLS;
}

// The form of the rows a launch of `grid` blocks leaves its callback sums in (amc::red_finish): the compact 64-byte row while a
// lane adds at most RED_COMPACT_TRIPS summands per column -- one per trip --, the wide one beyond.
int red_row_stride(const amc_handle* h, int grid)
{
    const int64_t pairs = (h->M + 1) / 2, lanes = (int64_t)grid * AMC_BLOCK;
    return (!h->knobs.wide_red_rows && (pairs + lanes - 1) / lanes <= amc::RED_COMPACT_TRIPS) ? (int)amc::RED_COMPACT_WORDS : RED_HOST_STRIDE;
}

// The ticket a new reduction fills (tickets complete in the order they were begun), or nullptr when RED_TICKETS are in flight.
RedTicket* red_next(amc_handle* h) { return h->red_count == RED_TICKETS ? nullptr : &h->red[(h->red_head + h->red_count) % RED_TICKETS]; }

static int red_commit(amc_handle* h, RedTicket* t, int rows)
{
    AMC_HIP(hipEventRecord(t->ev, h->stream));
    t->pending = true;
    t->rows = rows;
    t->row_stride = red_row_stride(h, rows);       // (rows = the grid of the launch that wrote them)
    t->cols = h->red_cols;
    t->t_counted = h->t_base + h->t_counted;
    h->red_count += 1;
    return AMC_OK;
}

// Second half of a reduction whose sums over x were formed by the launch that has just been queued (rows in the next ticket's
// h_rows[grid][RED_HOST_STRIDE], make_sweep_args): with per-chain counters the fold of the step log (pending rows incl. that
// launch's) forms the ratio sums -- no pass re-reads x or the counters.
int finish_fused_reduce(amc_handle* h, int grid)
{
    RedTicket* t = red_next(h);
    if (!t) return fail(AMC_ERR_STATE, "finish_fused_reduce: no free reduction ticket");
    t->ratio_rows = 0;
    t->ratio_acc = false;
    if (h->counters) {
        AMC_TRY(fold_log(h, true, &t->ratio_rows, t->h_ratio));
    }
    return red_commit(h, t, grid);
}

// A launch that forms the callback sums adds ONE summand per trip and column (a chain pair's sum) into each lane's accumulators,
// and those hold XS_LANE_CAP of them (amc_xsum.h); a launch of `grid` blocks makes ceil(pairs / (grid 256)) trips per lane.
// Beyond that (ensembles of more than 2e9 chains) the sums are formed by the pass of their own, which flushes as it goes.
bool reduce_fits_in_grid(const amc_handle* h, int grid)
{
    const int64_t pairs = (h->M + 1) / 2, lanes = (int64_t)grid * AMC_BLOCK;
    return (pairs + lanes - 1) / lanes <= amc::xs::XS_LANE_CAP - 2;
}

// Finishes the OLDEST reduction in flight: its columns as records (amc_xsum.h): AMC_RED_HEADER + K of them.
static int reduce_end_records(amc_handle* h, const char* who, double* recs, uint64_t* steps_counted)
{
    if (h->red_count == 0) return fail(AMC_ERR_STATE, "%s: no reduction in flight (call amc_reduce_begin)", who);
    AMC_HIP(hipSetDevice(h->device));
    RedTicket* t = &h->red[h->red_head];
    AMC_HIP(wait_event(t->ev));                  // waits for that reduction only, not for work queued after it
    t->pending = false;
    h->red_head = (h->red_head + 1) % RED_TICKETS;
    h->red_count -= 1;
    namespace xs = amc::xs;
    xs::PartR col[amc::RED_COLS];
    for (int c = 0; c < amc::RED_COLS; ++c) col[c] = xs::part_r_empty();
    double slot_total = 0.0;
    const bool compact = t->row_stride == amc::RED_COMPACT_WORDS;
    const bool with_slot = h->K == 1 && !h->counters;       // the row's last word is written by those launches only
    for (int r = 0; r < t->rows; ++r) {
        const amc::xs_word* row = t->h_rows + (size_t)r * t->row_stride;
        for (int c = 0; c < amc::RED_COLS; ++c)
            xs::part_r_merge(col[c], compact ? amc::xs_load_compact_row(row, c) : amc::xs_load_r_row(row + c * amc::XS_ROW_R));
        if (with_slot) {
            double v;
            std::memcpy(&v, row + (compact ? (int)amc::RED_COMPACT_SLOT : (int)amc::RED_ROW_SLOT), sizeof(double));
            slot_total += v;                                // integers: exact in any order
        }
    }
    // a sum nobody asked for (amc_set_reduce_columns) was not formed: its record stays empty
    static const int want[amc::RED_COLS] = {amc::RED_WANT_E, amc::RED_WANT_X, amc::RED_WANT_XX};
    for (int c = 0; c < amc::RED_COLS; ++c) {
        if (t->cols & want[c]) xs::rec_from_r(recs + (size_t)c * xs::XS_WORDS, col[c]);
        else xs::rec_clear(recs + (size_t)c * xs::XS_WORDS);
    }
    // the rows of a reduction cover the handle's chains
    xs::rec_from_plain(recs + (size_t)AMC_RED_COUNT * xs::XS_WORDS, (double)h->M);
    for (int k = 0; k < h->K; ++k) {
        xs::PartQ q = xs::PartQ{xs::i128{0, 0}, 0u};
        int e = xs::XS_E_RATIO;
        if (t->ratio_rows > 0) {
            for (int r = 0; r < t->ratio_rows; ++r) {
                const xs::PartQ b = amc::xs_load_q_row(t->h_ratio + ((size_t)r * RATIO_STRIDE + k) * amc::XS_ROW_Q);
                q.k = xs::i128_add(q.k, b.k);
                q.flags |= b.flags;
            }
        } else if (t->ratio_acc) {
            const unsigned long long* a = t->h_ratio_acc + 3 * k;
            if (a[2] != 0) q.flags |= xs::XS_F_NAN;
            // low 32-bit halves and high parts were added separately: k = hi 2^32 + lo
            q.k = xs::i128_add(xs::i128_shl(xs::i128_of((long long)a[1]), 32), xs::i128{a[0], 0});
        } else {
            // K == 1 without per-chain counters: total_calls is the same on every chain, so sum_c accepted_c / total is
            // (sum_c accepted_c) / total up to rounding: the record is the pool-wide accepted TOTAL
            // (an integer, quantum 2^0); whoever rounds it divides by steps_counted
            q.k = xs::i128_of((long long)slot_total);
            e = 0;
        }
        xs::rec_from_q(recs + (size_t)(AMC_RED_HEADER + k) * xs::XS_WORDS, q, e);
    }
    if (steps_counted) *steps_counted = t->t_counted;
    return AMC_OK;
}

extern "C" {

int amc_reduce_begin(amc_handle* h)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_reduce_begin: NULL handle");
    RedTicket* t = red_next(h);
    if (!t) return fail(AMC_ERR_STATE, "amc_reduce_begin: %d reductions are already in flight (call amc_reduce_end)", RED_TICKETS);
    AMC_HIP(hipSetDevice(h->device));
    int ratio_mode = (h->K > 1) ? 2 : (h->counters ? 1 : 0);
    t->ratio_rows = 0;
    t->ratio_acc = false;
    if (ratio_mode != 0 && h->K <= 4 && !h->d_acc_base) {
        // per-chain counters, few moves: the fold of the step log forms the acceptance-ratio sums while the counters
        // are in its registers (rows in h_ratio); the pass below then reads x only
        AMC_TRY(fold_log(h, true, &t->ratio_rows, t->h_ratio));
        ratio_mode = 0;
    } else if (ratio_mode != 0) {
        AMC_TRY(fold_log(h));
        AMC_HIP(hipMemsetAsync(t->d_ratio_acc, 0, (size_t)AMC_MAX_MOVES * 3 * sizeof(unsigned long long), h->stream));
        t->ratio_acc = true;
    }
    // The blocks store their rows straight into pinned, device-mapped host memory and the HOST adds them up in
    // amc_reduce_end (integers: amc_xsum.h) -- no final-pass launches (~5 us each even when empty) and no D2H copy in
    // stream order (which would hold the next sweep back for a copy-engine round trip).
    amc::xs_word* rows = t->h_rows;
    int stride = red_row_stride(h, h->red_blocks);
    int cols = h->red_cols;
    const unsigned long long* slots = (ratio_mode == 0 && t->ratio_rows == 0) ? h->d_acc_slots : nullptr;
    unsigned long long* racc = t->d_ratio_acc;
    void* params[] = {&h->d_x, &h->d_acc, &h->d_tot, &h->M, &h->M_pad, &h->K, &ratio_mode, &h->t_counted, &rows, &stride, &slots, &h->n_slots, &racc, &cols,
                      &h->d_acc_base, &h->d_tot_base, &h->t_base};
    AMC_TRY(launch_by_potential(h, "amc::reduce_kernel", (const void*)amc::reduce_kernel<amc::POT_DOUBLE_WELL>, (const void*)amc::reduce_kernel<amc::POT_HARMONIC>,
                                h->red_blocks, params));
    if (t->ratio_acc)
        AMC_HIP(hipMemcpyAsync(t->h_ratio_acc, t->d_ratio_acc, (size_t)h->K * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               h->stream));
    return red_commit(h, t, h->red_blocks);
}

int amc_sweep_reduce_begin(amc_handle* h, int64_t n_sweeps)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_sweep_reduce_begin: NULL handle");
    if (n_sweeps < 1) return fail(AMC_ERR_BAD_ARG, "amc_sweep_reduce_begin: n_sweeps must be >= 1");
    if (!red_next(h))
        return fail(AMC_ERR_STATE, "amc_sweep_reduce_begin: %d reductions are already in flight (call amc_reduce_end)", RED_TICKETS);
    // the ratio sums need the counters of every move (K > 4), or arrays plus their 64-bit bases (a handle that has counted past
    // 2^32 steps): sweep, then the reduction pass
    // (and so does a handle with widths per rung: its sweep form carries no sums -- reproducible sums, the same bits either way)
    if (h->K > 4 || h->d_acc_base || h->lad.rung_on || !reduce_fits_in_grid(h, reduce_sweep_grid(h))) {
        const int rc = sweep_impl(h, n_sweeps, false, nullptr);
        return rc != AMC_OK ? rc : amc_reduce_begin(h);
    }
    int grid = 0;
    AMC_TRY(sweep_impl(h, n_sweeps, true, &grid));     // the last launch wrote the sums over x to the ticket's rows
    return finish_fused_reduce(h, grid);
}

int amc_reduce_end_exact(amc_handle* h, double* records, uint64_t* steps_counted)
{
    if (!h || !records) return fail(AMC_ERR_BAD_ARG, "amc_reduce_end_exact: NULL argument");
    return reduce_end_records(h, "amc_reduce_end_exact", records, steps_counted);
}

int amc_reduce_end(amc_handle* h, double* out)
{
    if (!h || !out) return fail(AMC_ERR_BAD_ARG, "amc_reduce_end: NULL argument");
    double recs[(AMC_RED_HEADER + AMC_MAX_MOVES) * amc::xs::XS_WORDS];
    uint64_t steps = 0;
    AMC_TRY(reduce_end_records(h, "amc_reduce_end", recs, &steps));
    for (int i = 0; i < AMC_RED_HEADER + h->K; ++i)
        out[i] = recs[(size_t)i * amc::xs::XS_WORDS] == (double)amc::xs::XS_EMPTY ? std::nan("") : amc::xs::rec_round(recs + (size_t)i * amc::xs::XS_WORDS);
    if (h->K == 1 && !h->counters) out[AMC_RED_SUM_RATIO0] = out[AMC_RED_SUM_RATIO0] / (double)steps;
    return AMC_OK;
}

int amc_reduce(amc_handle* h, double* out)
{
    if (!h || !out) return fail(AMC_ERR_BAD_ARG, "amc_reduce: NULL argument");
    if (h->red_count != 0) return fail(AMC_ERR_STATE, "amc_reduce: a reduction is in flight (call amc_reduce_end first)");
    const int rc = amc_reduce_begin(h);
    return rc != AMC_OK ? rc : amc_reduce_end(h, out);
}

int amc_set_reduce_columns(amc_handle* h, int columns)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_reduce_columns: NULL handle");
    if (columns < 0 || columns > AMC_REDUCE_ALL) return fail(AMC_ERR_BAD_ARG, "amc_set_reduce_columns: columns must be a combination of AMC_REDUCE_E / _X / _XX");
    h->red_cols = columns;
    return AMC_OK;
}

// Host-side arithmetic on records (no device involved): into[i] += from[i]; out[i] = the Float64 of records[i].
int amc_xsum_merge(double* into, const double* from, int n_records)
{
    if (!into || !from || n_records < 0) return fail(AMC_ERR_BAD_ARG, "amc_xsum_merge: bad argument");
    for (int i = 0; i < n_records; ++i) amc::xs::rec_merge(into + (size_t)i * amc::xs::XS_WORDS, from + (size_t)i * amc::xs::XS_WORDS);
    return AMC_OK;
}

int amc_xsum_round(const double* records, int n_records, double* out)
{
    if (!records || !out || n_records < 0) return fail(AMC_ERR_BAD_ARG, "amc_xsum_round: bad argument");
    for (int i = 0; i < n_records; ++i) out[i] = amc::xs::rec_round(records + (size_t)i * amc::xs::XS_WORDS);
    return AMC_OK;
}

}  // extern "C"
