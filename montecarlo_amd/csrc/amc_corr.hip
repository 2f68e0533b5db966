// amc_corr.hip -- time correlation from one time origin: the mark (amc_corr_mark), the samples
// (amc_corr_sample), their records (amc_corr_fetch), the checkpoint pair (amc_corr_download_origin, amc_set_corr) and amc_corr_clear.
// The passes are rung passes (RungPass, amc_internal.h) with G = 1 where the handle has no ladder; their block rows share
// lad.d_rung_rows with the rung and the bridge sums.  Everything here is allocated at its first use: a handle that never marks has
// none of it and launches what it always did.
#define AMC_KERNEL_LINKAGE static      // template instantiations, and this object's own copy of the plain kernel it launches (corr_finish_kernel)
#include "amc_internal.h"

static_assert(AMC_CORR_E == amc::CORR_E && AMC_CORR_X == amc::CORR_X && AMC_CORR_COLS == amc::CORR_COLS && AMC_CORR_MAX_LAGS == amc::CORR_MAX_LAGS &&
              AMC_XSUM_WORDS == amc::xs::XS_WORDS, "the time correlation of include/amc.h and amc_corr.h");

static const size_t CORR_BYTES = (size_t)amc::CORR_ACC_WORDS * sizeof(amc::xs_word);      // d_corr (amc_corr.h CORR_ACC_WORDS)

// words of one sample's rows: with a partition a row per (block, group, column)
static inline size_t corr_sample_words(const amc_handle* h)
{
    return (size_t)std::max(1, h->blocks.n_blocks) * pass_groups(h) * amc::CORR_COLS * amc::XS_ROW_R;
}

static int corr_room(amc_handle* h)
{
    if (!h->corr.d_origin) {
        AMC_HIP(hipMalloc(&h->corr.d_origin, (size_t)h->M_pad * sizeof(double)));
        AMC_HIP(hipMemsetAsync(h->corr.d_origin, 0, (size_t)h->M_pad * sizeof(double), h->stream));
    }
    return zeroed_words(h, &h->corr.d_corr, CORR_BYTES);
}

// The blocked accumulator (a partition is set): rows [sample][b][g][c], room for slot `slot`, so that its size follows B, G and the
// lags in use.  keep: what the slots below it hold is kept, and the room doubles (16 samples at a mark); otherwise a restore is
// about to write slots 0 .. slot, and the room is theirs (16 at least).
static int corr_blocks_room(amc_handle* h, int slot, bool keep)
{
    const size_t spw = corr_sample_words(h);
    if ((size_t)(slot + 1) * spw <= h->blocks.corr_blk_words) return AMC_OK;
    const size_t need = (size_t)(keep ? std::min<int>(AMC_CORR_MAX_LAGS, std::max(16, 2 * slot)) : std::max(16, slot + 1)) * spw;
    amc::xs_word* grown = nullptr;
    AMC_HIP(hipMalloc(&grown, need * sizeof(amc::xs_word)));
    if (keep && slot && h->blocks.d_corr_blk)
        (void)hipMemcpyAsync(grown, h->blocks.d_corr_blk, (size_t)slot * spw * sizeof(amc::xs_word), hipMemcpyDeviceToDevice, h->stream);
    const hipError_t e = hipStreamSynchronize(h->stream);      // (a finishing kernel queued earlier may still write the old rows)
    (void)hipFree(h->blocks.d_corr_blk);
    h->blocks.d_corr_blk = grown;
    h->blocks.corr_blk_words = need;
    AMC_HIP(e);
    return AMC_OK;
}

// One pass into slot `slot`: the sums of the sample, and with `mark` the origin values too.  With a partition the traversal of
// amc_blocks.h into the blocked accumulator.
static int corr_pass(amc_handle* h, int observable, int slot, bool mark)
{
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of a bridge snapshot: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    const int B = h->blocks.n_blocks;
    RungPass p;
    amc::CorrArgs a = {};
    a.mark = mark ? 1 : 0;
    AMC_TRY(rung_pass_plan(h, amc::CORR_COLS, B != 0, &p));
    AMC_TRY(corr_room(h));
    if (B) AMC_TRY(corr_blocks_room(h, slot, true));
    a.origin = h->corr.d_origin;
    if (B)
        AMC_TRY(rung_pass_launch(h, p, a, observable, "amc::corr_sums_blocks_kernel", (const void*)amc::corr_sums_blocks_kernel<amc::POT_DOUBLE_WELL>,
                                 (const void*)amc::corr_sums_blocks_kernel<amc::POT_HARMONIC>));
    else
        AMC_TRY(rung_pass_launch(h, p, a, observable, "amc::corr_sums_kernel", (const void*)amc::corr_sums_kernel<amc::POT_DOUBLE_WELL>,
                                 (const void*)amc::corr_sums_kernel<amc::POT_HARMONIC>));
    hipLaunchKernelGGL(amc::corr_finish_kernel, dim3((B ? B : 1) * p.groups * amc::CORR_COLS), dim3(64), 0, h->stream, (const amc::xs_word*)h->lad.d_rung_rows,
                       p.n_blocks(), p.groups, B ? B : 1, (B ? h->blocks.d_corr_blk : h->corr.d_corr) + (size_t)slot * corr_sample_words(h));
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

// A mark adopted (amc_corr_mark, the setters), and reported (the fetches).
static void corr_adopt(amc_handle* h, int observable, const uint64_t* steps, int n_samples)
{
    h->corr.observable = observable;
    h->corr.groups = pass_groups(h);
    h->corr.n_samples = n_samples;
    for (int s = 0; s < n_samples; ++s) h->corr.steps[s] = steps[s];
}
static void corr_report(const amc_handle* h, int n, uint64_t* steps, int* n_samples, int* observable)
{
    for (int s = 0; steps && s < n; ++s) steps[s] = h->corr.steps[s];
    *n_samples = n;
    *observable = h->corr.observable;
}

extern "C" {

int amc_corr_mark(amc_handle* h, int observable)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_corr_mark: NULL handle");
    if (observable != AMC_CORR_E && observable != AMC_CORR_X)
        return fail(AMC_ERR_BAD_ARG, "amc_corr_mark: observable = %d must be AMC_CORR_E or AMC_CORR_X", observable);
    AMC_TRY(corr_pass(h, observable, 0, true));
    corr_adopt(h, observable, &h->t, 1);
    return AMC_OK;
}

int amc_corr_sample(amc_handle* h)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_corr_sample: NULL handle");
    if (!h->corr.observable) return fail(AMC_ERR_STATE, "amc_corr_sample: nothing is marked (amc_corr_mark)");
    if (h->corr.n_samples >= AMC_CORR_MAX_LAGS)
        return fail(AMC_ERR_STATE, "amc_corr_sample: all %d slots of the mark are used", AMC_CORR_MAX_LAGS);
    AMC_TRY(corr_pass(h, h->corr.observable, h->corr.n_samples, false));
    h->corr.steps[h->corr.n_samples] = h->t;
    h->corr.n_samples += 1;
    return AMC_OK;
}

int amc_corr_fetch(amc_handle* h, double* records, uint64_t* steps, int capacity, int* n_samples, int* observable)
{
    if (!h || !records || !steps || !n_samples || !observable) return fail(AMC_ERR_BAD_ARG, "amc_corr_fetch: NULL argument");
    const int n = h->corr.observable ? h->corr.n_samples : 0;
    if (capacity < n) return fail(AMC_ERR_BAD_ARG, "amc_corr_fetch: capacity = %d, the mark has %d samples", capacity, n);
    AMC_HIP(hipSetDevice(h->device));
    const size_t n_rows = (size_t)n * h->corr.groups * amc::CORR_COLS;
    if (h->blocks.n_blocks && n) {      // the merge over the blocks: integers, the records of a handle without a partition
        const int B = h->blocks.n_blocks;
        const size_t per_sample = (size_t)h->corr.groups * amc::CORR_COLS;
        std::vector<amc::xs_word> host(n_rows * B * amc::XS_ROW_R, 0ull);
        AMC_TRY(copy_to_host_sync(h, host.data(), h->blocks.d_corr_blk, host.size() * sizeof(amc::xs_word)));
        for (size_t s = 0; s < n_rows; ++s) {
            const size_t slot = s / per_sample, gc = s % per_sample;
            amc::xs::PartR p = amc::xs::part_r_empty();
            for (int b = 0; b < B; ++b) amc::xs::part_r_merge(p, amc::xs_load_r_row(host.data() + ((slot * B + b) * per_sample + gc) * amc::XS_ROW_R));
            amc::xs::rec_from_r(records + s * amc::xs::XS_WORDS, p);
        }
    } else {
        std::vector<amc::xs_word> host(n_rows * amc::XS_ROW_R + 1, 0ull);
        AMC_TRY(copy_to_host_sync(h, host.data(), n ? h->corr.d_corr : nullptr, n_rows * amc::XS_ROW_R * sizeof(amc::xs_word)));
        for (size_t s = 0; s < n_rows; ++s) amc::xs::rec_from_r(records + s * amc::xs::XS_WORDS, amc::xs_load_r_row(host.data() + s * amc::XS_ROW_R));
    }
    corr_report(h, n, steps, n_samples, observable);
    return AMC_OK;
}

int amc_corr_fetch_blocks(amc_handle* h, double* records, uint64_t* steps, int capacity, int* n_blocks, int* n_samples, int* observable)
{
    if (!h || !n_blocks || !n_samples || !observable) return fail(AMC_ERR_BAD_ARG, "amc_corr_fetch_blocks: NULL argument");
    const int B = h->blocks.n_blocks;
    if (!B) return fail(AMC_ERR_STATE, "amc_corr_fetch_blocks: no partition is set (amc_set_blocks)");
    const int n = h->corr.observable ? h->corr.n_samples : 0;
    if (!records || !steps) {           // the sizes alone, for a caller about to allocate: nothing waits, nothing is copied
        *n_blocks = B;
        corr_report(h, n, nullptr, n_samples, observable);
        return AMC_OK;
    }
    if (capacity < n) return fail(AMC_ERR_BAD_ARG, "amc_corr_fetch_blocks: capacity = %d, the mark has %d samples", capacity, n);
    AMC_HIP(hipSetDevice(h->device));
    const int G = pass_groups(h);
    const size_t per_sample = (size_t)G * amc::CORR_COLS;
    std::vector<amc::xs_word> host((size_t)n * B * per_sample * amc::XS_ROW_R + 1, 0ull);
    AMC_TRY(copy_to_host_sync(h, host.data(), n ? h->blocks.d_corr_blk : nullptr, (host.size() - 1) * sizeof(amc::xs_word)));
    const amc::blk::Part part = blocks_part(h);
    for (int b = 0; b < B; ++b) {
        const bool empty = amc::blk::ladders_in_block(part, b, h->M / G) == 0;      // a block without a local ladder: all-zero records
        for (int s = 0; s < n; ++s)
            for (size_t gc = 0; gc < per_sample; ++gc) {
                double* rec = records + (((size_t)b * n + s) * per_sample + gc) * amc::xs::XS_WORDS;
                if (empty) amc::xs::rec_clear(rec);
                else amc::xs::rec_from_r(rec, amc::xs_load_r_row(host.data() + (((size_t)s * B + b) * per_sample + gc) * amc::XS_ROW_R));
            }
    }
    *n_blocks = B;
    corr_report(h, n, steps, n_samples, observable);
    return AMC_OK;
}

int amc_corr_download_origin(amc_handle* h, double* origin)
{
    if (!h || !origin) return fail(AMC_ERR_BAD_ARG, "amc_corr_download_origin: NULL argument");
    if (!h->corr.observable) return fail(AMC_ERR_STATE, "amc_corr_download_origin: nothing is marked (amc_corr_mark)");
    AMC_HIP(hipSetDevice(h->device));
    return copy_to_host_sync(h, origin, h->corr.d_origin, (size_t)h->M * sizeof(double));
}

// What amc_set_corr and amc_set_corr_blocks refuse alike: the observable, the number of samples, the steps.
static int corr_set_check(const char* who, int observable, const uint64_t* steps, int n_samples)
{
    if (observable != AMC_CORR_E && observable != AMC_CORR_X)
        return fail(AMC_ERR_BAD_ARG, "%s: observable = %d must be AMC_CORR_E or AMC_CORR_X", who, observable);
    if (n_samples < 1 || n_samples > AMC_CORR_MAX_LAGS)
        return fail(AMC_ERR_BAD_ARG, "%s: n_samples = %d must lie in [1, %d]", who, n_samples, AMC_CORR_MAX_LAGS);
    for (int s = 0; s < n_samples; ++s) {
        if (steps[s] >> 48) return fail(AMC_ERR_BAD_ARG, "%s: steps[%d] must fit 48 bits", who, s);
        if (s && steps[s] < steps[s - 1]) return fail(AMC_ERR_BAD_ARG, "%s: steps[%d] = %llu lies before steps[%d]", who, s, (unsigned long long)steps[s], s - 1);
    }
    return AMC_OK;
}

// One record of a sample into its row: every (sample, group, column) had a summand, so each is a kind-R record, as amc_corr_fetch gave it.
static int corr_row_from_record(const char* who, const double* rec, int slot, int g, int c, amc::xs_word* row)
{
    char where[64];
    std::snprintf(where, sizeof where, "sample %d, group %d, column %d", slot, g, c);
    return r_row_from_record(who, where, rec, row);
}

int amc_set_corr(amc_handle* h, int observable, const double* origin, const double* records, const uint64_t* steps, int n_samples)
{
    if (!h || !origin || !records || !steps) return fail(AMC_ERR_BAD_ARG, "amc_set_corr: NULL argument");
    // (the accumulator in use is the blocked one, which merged records cannot fill: taking them would drop them silently)
    if (h->blocks.n_blocks)
        return fail(AMC_ERR_STATE, "amc_set_corr: a partition is set (amc_set_blocks): merged records cannot be split into its blocks, "
                                   "amc_set_corr_blocks restores them");
    AMC_TRY(corr_set_check("amc_set_corr", observable, steps, n_samples));
    const int G = pass_groups(h);
    const size_t n_rows = (size_t)n_samples * G * amc::CORR_COLS;
    std::vector<amc::xs_word> host(n_rows * amc::XS_ROW_R, 0ull);
    for (size_t s = 0; s < n_rows; ++s)
        AMC_TRY(corr_row_from_record("amc_set_corr", records + s * amc::xs::XS_WORDS, (int)(s / ((size_t)G * amc::CORR_COLS)), (int)(s / amc::CORR_COLS % G),
                                     (int)(s % amc::CORR_COLS), host.data() + s * amc::XS_ROW_R));
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(corr_room(h));
    AMC_HIP(hipMemcpyAsync(h->corr.d_origin, origin, (size_t)h->M * sizeof(double), hipMemcpyHostToDevice, h->stream));
    AMC_TRY(copy_to_device_sync(h, h->corr.d_corr, host.data(), host.size() * sizeof(amc::xs_word)));      // the caller's buffers are only valid during the call
    corr_adopt(h, observable, steps, n_samples);
    return AMC_OK;
}

int amc_set_corr_blocks(amc_handle* h, int observable, const double* origin, const double* records, const uint64_t* steps, int n_blocks, int n_samples)
{
    if (!h || !origin || !records || !steps) return fail(AMC_ERR_BAD_ARG, "amc_set_corr_blocks: NULL argument");
    const int B = h->blocks.n_blocks;
    if (!B) return fail(AMC_ERR_STATE, "amc_set_corr_blocks: no partition is set (amc_set_blocks)");
    if (n_blocks != B) return fail(AMC_ERR_BAD_ARG, "amc_set_corr_blocks: n_blocks = %d, the partition has %d blocks", n_blocks, B);
    AMC_TRY(corr_set_check("amc_set_corr_blocks", observable, steps, n_samples));
    // records[b][s][g][c] as amc_corr_fetch_blocks gave them, into the rows [s][b][g][c]; a block without a local ladder is all zero
    const int G = pass_groups(h);
    const size_t per_sample = (size_t)G * amc::CORR_COLS;
    std::vector<amc::xs_word> host((size_t)n_samples * B * per_sample * amc::XS_ROW_R, 0ull);
    const amc::blk::Part part = blocks_part(h);
    for (int b = 0; b < B; ++b) {
        const bool empty = amc::blk::ladders_in_block(part, b, h->M / G) == 0;
        for (int s = 0; s < n_samples; ++s)
            for (size_t gc = 0; gc < per_sample; ++gc) {
                const double* rec = records + (((size_t)b * n_samples + s) * per_sample + gc) * amc::xs::XS_WORDS;
                if (empty) {
                    for (int i = 0; i < amc::xs::XS_WORDS; ++i)
                        if (rec[i] != 0.0) return fail(AMC_ERR_BAD_ARG, "amc_set_corr_blocks: block %d has no local ladder, its records must be all zero", b);
                    continue;
                }
                AMC_TRY(corr_row_from_record("amc_set_corr_blocks", rec, s, (int)(gc / amc::CORR_COLS), (int)(gc % amc::CORR_COLS),
                                             host.data() + (((size_t)s * B + b) * per_sample + gc) * amc::XS_ROW_R));
            }
    }
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(corr_room(h));
    AMC_TRY(corr_blocks_room(h, n_samples - 1, false));      // (nothing the old rows hold is kept)
    AMC_HIP(hipMemcpyAsync(h->corr.d_origin, origin, (size_t)h->M * sizeof(double), hipMemcpyHostToDevice, h->stream));
    AMC_TRY(copy_to_device_sync(h, h->blocks.d_corr_blk, host.data(), host.size() * sizeof(amc::xs_word)));      // the caller's buffers are only valid during the call
    corr_adopt(h, observable, steps, n_samples);
    return AMC_OK;
}

int amc_corr_clear(amc_handle* h)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_corr_clear: NULL handle");
    corr_forget(h);
    return AMC_OK;
}

}  // extern "C"
