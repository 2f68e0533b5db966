// amc_emom.hip -- moments per energy bin (DESIGN.md section 3.17 "Moments per bin"): one pass per snapshot into a device-resident
// accumulator of 64-bit counts and signed 64-bit sums of x, x^2 and [x > 0] per (group, bin) (amc_energy_moments_accumulate), its fetch
// (amc_energy_moments_fetch) and the checkpoint entry (amc_set_energy_moments); the same kept per jackknife block ("Moments per block":
// amc_energy_moments_accumulate_blocks / _fetch_blocks, amc_set_energy_moments_blocks).  Independent of the energy histograms'
// accumulator (amc_ehist.hip): both may stand.  Allocated at its first use: a handle that never accumulates has none and launches what
// it always did.
#define AMC_KERNEL_LINKAGE static      // template instantiations only: the plain kernels of the accumulators over the energy bins are amc_ehist.hip's
#include "amc_internal.h"

static_assert(AMC_EMOM_X == amc::EMOM_X && AMC_EMOM_XX == amc::EMOM_XX && AMC_EMOM_POS == amc::EMOM_POS && AMC_EMOM_ALL == amc::EMOM_ALL,
              "the columns of include/amc.h and amc_emom.h");

// What every entry asks of a form: the bins as every histogram entry, a mask of known columns, a bound whose quanta exist.
// (2^-500 <= x_bound < 2^500 keeps 1.5 * 2^(E + 52) a normal number for both quanta)
static int emom_form_ok(const char* who, double lo, double hi, int n_bins, int mask, double x_bound)
{
    if (!hist_args_ok(who, lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    if (mask == 0 || (mask & ~AMC_EMOM_ALL)) return fail(AMC_ERR_BAD_ARG, "%s: mask = %d: need at least one of AMC_EMOM_X, AMC_EMOM_XX, AMC_EMOM_POS and no other bit", who, mask);
    if (!(std::isfinite(x_bound) && x_bound > 0.0)) return fail(AMC_ERR_BAD_ARG, "%s: x_bound = %g must be finite and positive", who, x_bound);
    if (!(x_bound >= 0x1p-500 && x_bound < 0x1p500)) return fail(AMC_ERR_BAD_ARG, "%s: x_bound = %g lies outside [2^-500, 2^500)", who, x_bound);
    return AMC_OK;
}

// The form of an accumulator begun now: a set is G rows of n_bins + 4 count cells, then G x C rows of n_bins sum cells; one set
// (plain) or one per jackknife block.
static EmomState emom_form(const amc_handle* h, double lo, double hi, int n_bins, int mask, double x_bound, int blocks = 0)
{
    EmomState f;
    f.n_bins = n_bins;
    f.groups = pass_groups(h);
    f.blocks = blocks;
    f.tail = 4;
    f.cols = __builtin_popcount((unsigned)mask);
    f.lo = lo;
    f.hi = hi;
    f.mask = mask;
    f.x_bound = x_bound;
    return f;
}

static int emom_cap_ok(const char* who, const EmomState& f)
{
    if (bins_words(f) > (size_t)AMC_EMOM_BLK_MAX_WORDS)
        return fail(AMC_ERR_BAD_ARG, "%s: %d blocks of %d rows of %d count cells and %d x %d rows of %d sum cells are more than AMC_EMOM_BLK_MAX_WORDS = %d words",
                    who, f.blocks, f.groups, f.n_bins + 4, f.groups, f.cols, f.n_bins, AMC_EMOM_BLK_MAX_WORDS);
    return AMC_OK;
}

// A cell holds fewer than 2^31 deposits: n_snapshots * (n_chains / G) stays below 2^31.
static inline bool emom_fits(const amc_handle* h, uint64_t n_snapshots)
{
    const uint64_t per_group = (uint64_t)(h->M / pass_groups(h));
    return n_snapshots < ((uint64_t)1 << 31) && n_snapshots * per_group < ((uint64_t)1 << 31);
}

// What both accumulate entries ask of a standing accumulator: the caller's form (plain or per block), the caller's bins, mask and bound.
static int emom_same(const amc_handle* h, const char* who, bool blocked, double lo, double hi, int n_bins, int mask, double x_bound)
{
    const EmomState& s = h->emom;
    if (!s.d_words) return AMC_OK;
    if ((s.blocks != 0) != blocked)
        return fail(AMC_ERR_STATE, "%s: the accumulator is %s (amc_energy_moments_fetch with reset frees it)", who,
                    blocked ? "a plain one, not kept per jackknife block" : "kept per jackknife block");
    if (n_bins != s.n_bins || lo != s.lo || hi != s.hi || mask != s.mask || x_bound != s.x_bound)
        return fail(AMC_ERR_STATE, "%s: the accumulator has another form: [%g, %g) in %d bins, mask %d, x_bound %g (amc_energy_moments_fetch with reset frees it)",
                    who, s.lo, s.hi, s.n_bins, s.mask, s.x_bound);
    return AMC_OK;
}

// The pass's arguments from the standing accumulator: counts and sums of its first set.
static amc::EmomArgs emom_args(const amc_handle* h)
{
    const EmomState& s = h->emom;
    amc::EmomArgs a = {};
    a.x = h->d_x;
    a.counts = s.d_words;
    a.sums = s.d_words + bins_count_cells(s);
    a.n_chains = h->M;
    a.lo = s.lo;
    a.hi = s.hi;
    a.inv_w = (double)s.n_bins / (s.hi - s.lo);
    a.x_bound = s.x_bound;
    a.n_groups = s.groups;
    a.n_bins = s.n_bins;
    a.mask = s.mask;
    a.n_cols = s.cols;
    a.e_x = amc::emom_e_x(s.x_bound);
    a.e_xx = amc::emom_e_xx(s.x_bound);
    return a;
}

// The cells of the sets of form f against what they must hold: every (set, group) count row sums to want[s], every sum cell is bounded
// by the count of its bin.  counts[(s G + g) (n_bins + 4) + cell], sums[((s G + g) C + c) n_bins + b].
static int emom_cells_ok(const char* who, const char* what, const uint64_t* counts, const int64_t* sums, const EmomState& f, const uint64_t* want)
{
    const int G = f.groups, n_bins = f.n_bins, cols = f.cols, pos_col = (f.mask & AMC_EMOM_POS) ? cols - 1 : -1;
    char where[32] = "";
    for (int s = 0; s < (f.blocks ? f.blocks : 1); ++s)
        for (int g = 0; g < G; ++g) {
            if (f.blocks) snprintf(where, sizeof where, " of block %d", s);
            const uint64_t* row = counts + ((size_t)s * G + g) * (n_bins + 4);
            AMC_TRY(bins_row_sum(who, what, row, (size_t)n_bins + 4, want[s], g, f.blocks ? s : -1));
            for (int c = 0; c < cols; ++c)
                for (int b = 0; b < n_bins; ++b) {
                    const int64_t v = sums[(((size_t)s * G + g) * cols + c) * n_bins + b];
                    const uint64_t n = row[b];                  // (< 2^31: n << 32 cannot wrap)
                    const uint64_t mag = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
                    if (c == pos_col ? (v < 0 || mag > n) : mag > (n << 32))
                        return fail(AMC_ERR_BAD_ARG, "%s: sum cell (group %d, column %d, bin %d)%s = %lld is more than the %llu chains of its bin can hold", who, g,
                                    c, b, where, (long long)v, (unsigned long long)n);
                }
        }
    return AMC_OK;
}

extern "C" {

int amc_energy_moments_accumulate(amc_handle* h, double lo, double hi, int n_bins, int mask, double x_bound)
{
    static const char* who = "amc_energy_moments_accumulate";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    AMC_TRY(emom_form_ok(who, lo, hi, n_bins, mask, x_bound));
    AMC_TRY(emom_same(h, who, false, lo, hi, n_bins, mask, x_bound));
    // before anything is allocated or launched: the pass that would let a cell reach 2^31 deposits
    if (!emom_fits(h, h->emom.n_snapshots + 1))
        return fail(AMC_ERR_STATE, "%s: %llu snapshots of %lld chains per group are all a cell holds (n_snapshots * n_chains / G < 2^31): fetch with reset", who,
                    (unsigned long long)h->emom.n_snapshots, (long long)(h->M / pass_groups(h)));
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of an energy-histogram snapshot: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    const bool first = !h->emom.d_words;
    if (first) AMC_TRY(bins_begin(h, h->emom, emom_form(h, lo, hi, n_bins, mask, x_bound), who, true));
    amc::EmomArgs a = emom_args(h);
    void* params[] = {&a};
    AMC_TRY(bins_pass(h, h->emom, first, "amc::energy_moments_kernel", (const void*)amc::energy_moments_kernel<amc::POT_DOUBLE_WELL>,
                      (const void*)amc::energy_moments_kernel<amc::POT_HARMONIC>, hist_grid(h), params));
    h->emom.n_snapshots += 1;
    return AMC_OK;
}

int amc_energy_moments_accumulate_blocks(amc_handle* h, double lo, double hi, int n_bins, int mask, double x_bound)
{
    static const char* who = "amc_energy_moments_accumulate_blocks";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    int B = 0, grid = 0;
    bool by_family = false;             // (never: the moments are kept per block of ladders alone)
    AMC_TRY(bins_partition(h, who, false, &B, &by_family));
    AMC_TRY(emom_form_ok(who, lo, hi, n_bins, mask, x_bound));
    const EmomState form = emom_form(h, lo, hi, n_bins, mask, x_bound, B);
    AMC_TRY(emom_cap_ok(who, form));
    AMC_TRY(emom_same(h, who, true, lo, hi, n_bins, mask, x_bound));
    // before anything is allocated or launched: the plain rule, conservative per block, and what keeps a later fold valid
    if (!emom_fits(h, h->emom.n_snapshots + 1))
        return fail(AMC_ERR_STATE, "%s: %llu snapshots of %lld chains per group are all a cell holds (n_snapshots * n_chains / G < 2^31): fetch with reset", who,
                    (unsigned long long)h->emom.n_snapshots, (long long)(h->M / form.groups));
    AMC_TRY(bins_u32_blocked_ok(h, who, B, &grid));
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));
    const bool first = !h->emom.d_words;
    if (first) AMC_TRY(bins_begin(h, h->emom, form, who, true));
    amc::EmomArgs a = emom_args(h);
    amc::blk::Part part = blocks_part(h);
    void* params[] = {&a, &part};
    AMC_TRY(bins_pass(h, h->emom, first, "amc::energy_moments_blocks_kernel", (const void*)amc::energy_moments_blocks_kernel<amc::POT_DOUBLE_WELL>,
                      (const void*)amc::energy_moments_blocks_kernel<amc::POT_HARMONIC>, grid, params));
    h->emom.n_snapshots += 1;
    return AMC_OK;
}

int amc_energy_moments_fetch(amc_handle* h, uint64_t* counts, int64_t* sums, int64_t capacity_counts, int64_t capacity_sums, int* n_groups, int* n_bins,
                             int* n_cols, double* lo, double* hi, int* mask, double* x_bound, uint64_t* n_snapshots, int reset)
{
    static const char* who = "amc_energy_moments_fetch";
    if (!h || !n_groups || !n_bins || !n_cols || !lo || !hi || !mask || !x_bound || !n_snapshots) return fail(AMC_ERR_BAD_ARG, "%s: NULL argument", who);
    const EmomState& s = h->emom;
    *n_groups = s.d_words ? s.groups : pass_groups(h);
    *n_bins = s.n_bins;
    *n_cols = s.cols;
    *lo = s.lo;
    *hi = s.hi;
    *mask = s.mask;
    *x_bound = s.x_bound;
    *n_snapshots = 0;
    if (!s.d_words) return AMC_OK;      // nothing accumulated: no cells (the arrays may be NULL), no form
    if (!counts && !sums) return AMC_OK;        // the sizes alone, for a caller about to allocate: nothing waits, nothing is copied, nothing is reset
    if (!counts || !sums) return fail(AMC_ERR_BAD_ARG, "%s: counts and sums are given together, or neither", who);
    const size_t n_counts = bins_count_cells(s), n_sums = bins_sum_cells(s);
    if (capacity_counts < (int64_t)n_counts || capacity_sums < (int64_t)n_sums)
        return fail(AMC_ERR_BAD_ARG, "%s: capacities %lld and %lld, the accumulator has %d rows of %d count cells and %d x %d rows of %d sum cells", who,
                    (long long)capacity_counts, (long long)capacity_sums, s.groups, s.n_bins + 4, s.groups, s.cols, s.n_bins);
    AMC_HIP(hipSetDevice(h->device));
    if (s.blocks) {
        std::vector<uint64_t> set(n_counts + n_sums);
        AMC_TRY(bins_merge_blocks(h, s, set.data()));
        memcpy(counts, set.data(), n_counts * sizeof(uint64_t));
        memcpy(sums, set.data() + n_counts, n_sums * sizeof(uint64_t));
    } else {
        AMC_HIP(hipMemcpyAsync(sums, s.d_words + n_counts, n_sums * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        AMC_TRY(copy_to_host_sync(h, counts, s.d_words, n_counts * sizeof(unsigned long long)));
    }
    *n_snapshots = bins_snapshots(h, s, counts, false);
    h->emom.n_snapshots = *n_snapshots;                     // (a respacing that was taken has zeroed the cells: the count follows them)
    if (reset) return emom_clear(h);
    return AMC_OK;
}

int amc_energy_moments_fetch_blocks(amc_handle* h, uint64_t* counts, int64_t* sums, int64_t capacity_counts, int64_t capacity_sums, int* n_blocks,
                                    int* n_groups, int* n_bins, int* n_cols, double* lo, double* hi, int* mask, double* x_bound, uint64_t* n_snapshots,
                                    int reset)
{
    static const char* who = "amc_energy_moments_fetch_blocks";
    if (!h || !n_blocks || !n_groups || !n_bins || !n_cols || !lo || !hi || !mask || !x_bound || !n_snapshots)
        return fail(AMC_ERR_BAD_ARG, "%s: NULL argument", who);
    const EmomState& s = h->emom;
    if (!s.d_words || !s.blocks) return fail(AMC_ERR_STATE, "%s: no accumulator kept per jackknife block stands (amc_energy_moments_accumulate_blocks)", who);
    const int B = s.blocks, G = s.groups;
    *n_blocks = B;
    *n_groups = G;
    *n_bins = s.n_bins;
    *n_cols = s.cols;
    *lo = s.lo;
    *hi = s.hi;
    *mask = s.mask;
    *x_bound = s.x_bound;
    *n_snapshots = 0;
    if (!counts && !sums) return AMC_OK;        // the sizes alone: nothing waits, nothing is copied, nothing is reset
    if (!counts || !sums) return fail(AMC_ERR_BAD_ARG, "%s: counts and sums are given together, or neither", who);
    const size_t n_counts = bins_count_cells(s), n_sums = bins_sum_cells(s), set_words = n_counts + n_sums;
    if (capacity_counts < (int64_t)(B * n_counts) || capacity_sums < (int64_t)(B * n_sums))
        return fail(AMC_ERR_BAD_ARG, "%s: capacities %lld and %lld, the accumulator has %d blocks of %d rows of %d count cells and %d x %d rows of %d sum cells",
                    who, (long long)capacity_counts, (long long)capacity_sums, B, G, s.n_bins + 4, G, s.cols, s.n_bins);
    AMC_HIP(hipSetDevice(h->device));
    std::vector<uint64_t> all(bins_words(s));
    AMC_TRY(copy_to_host_sync(h, all.data(), s.d_words, all.size() * sizeof(uint64_t)));
    for (int b = 0; b < B; ++b) {           // the sets de-interleaved: all counts, then all sums
        memcpy(counts + (size_t)b * n_counts, all.data() + (size_t)b * set_words, n_counts * sizeof(uint64_t));
        memcpy(sums + (size_t)b * n_sums, all.data() + (size_t)b * set_words + n_counts, n_sums * sizeof(uint64_t));
    }
    *n_snapshots = bins_snapshots(h, s, counts, true);
    h->emom.n_snapshots = *n_snapshots;                     // (a respacing that was taken has zeroed the cells: the count follows them)
    if (reset) return emom_clear(h);
    return AMC_OK;
}

// The checkpoint entries: the accumulator standing, of either form, is replaced; a copy that fails leaves none.
static int emom_restore(amc_handle* h, const char* who, const EmomState& form, const uint64_t* words, uint64_t n_snapshots)
{
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(emom_clear(h));
    AMC_TRY(bins_begin(h, h->emom, form, who, false));
    const int rc = copy_to_device_sync(h, h->emom.d_words, words, bins_words(form) * sizeof(uint64_t));      // (`words` is only valid during the call)
    if (rc != AMC_OK) {
        (void)emom_clear(h);
        return rc;
    }
    h->emom.n_snapshots = n_snapshots;
    return AMC_OK;
}

int amc_set_energy_moments(amc_handle* h, double lo, double hi, int n_bins, int mask, double x_bound, const uint64_t* counts_or_null,
                           const int64_t* sums_or_null, uint64_t n_snapshots)
{
    static const char* who = "amc_set_energy_moments";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    if (!counts_or_null || !sums_or_null || n_snapshots == 0) {
        AMC_HIP(hipSetDevice(h->device));
        return emom_clear(h);
    }
    AMC_TRY(emom_form_ok(who, lo, hi, n_bins, mask, x_bound));
    const EmomState form = emom_form(h, lo, hi, n_bins, mask, x_bound);
    const uint64_t per_group = (uint64_t)(h->M / form.groups);
    if (!emom_fits(h, n_snapshots))
        return fail(AMC_ERR_BAD_ARG, "%s: n_snapshots * n_chains / G = %llu * %llu is not below 2^31, all a cell holds", who, (unsigned long long)n_snapshots,
                    (unsigned long long)per_group);
    const uint64_t want = n_snapshots * per_group;
    AMC_TRY(emom_cells_ok(who, "n_snapshots * n_chains / G", counts_or_null, sums_or_null, form, &want));
    std::vector<uint64_t> set(bins_set_words(form));        // counts and sums side by side, as the accumulator holds them
    memcpy(set.data(), counts_or_null, bins_count_cells(form) * sizeof(uint64_t));
    memcpy(set.data() + bins_count_cells(form), sums_or_null, bins_sum_cells(form) * sizeof(uint64_t));
    return emom_restore(h, who, form, set.data(), n_snapshots);
}

int amc_set_energy_moments_blocks(amc_handle* h, double lo, double hi, int n_bins, int mask, double x_bound, const uint64_t* counts_or_null,
                                  const int64_t* sums_or_null, int n_blocks, uint64_t n_snapshots)
{
    static const char* who = "amc_set_energy_moments_blocks";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    int B = 0;
    bool by_family = false;             // (never, as above)
    AMC_TRY(bins_partition(h, who, false, &B, &by_family));
    if (!counts_or_null || !sums_or_null || n_snapshots == 0) {
        AMC_HIP(hipSetDevice(h->device));
        return emom_clear(h);
    }
    if (n_blocks != B) return fail(AMC_ERR_BAD_ARG, "%s: n_blocks = %d, the partition has %d blocks", who, n_blocks, B);
    AMC_TRY(emom_form_ok(who, lo, hi, n_bins, mask, x_bound));
    const EmomState form = emom_form(h, lo, hi, n_bins, mask, x_bound, B);
    AMC_TRY(emom_cap_ok(who, form));
    const int G = form.groups;
    if (!emom_fits(h, n_snapshots))
        return fail(AMC_ERR_BAD_ARG, "%s: n_snapshots * n_chains / G = %llu * %llu is not below 2^31, all a cell holds", who, (unsigned long long)n_snapshots,
                    (unsigned long long)(h->M / G));
    // every (block, group) row holds the block's ladders once per snapshot; a block without a local ladder holds nothing
    const amc::blk::Part part = blocks_part(h);
    uint64_t want[AMC_MAX_JK_BLOCKS];
    for (int b = 0; b < B; ++b) want[b] = n_snapshots * (uint64_t)amc::blk::ladders_in_block(part, b, h->M / G);      // (at most n_snapshots * n_chains / G < 2^31)
    AMC_TRY(emom_cells_ok(who, "n_snapshots * (local ladders of the block)", counts_or_null, sums_or_null, form, want));
    const size_t n_counts = bins_count_cells(form), n_sums = bins_sum_cells(form), set_words = n_counts + n_sums;
    std::vector<uint64_t> all((size_t)B * set_words);      // the sets interleaved: counts and sums of block b side by side
    for (int b = 0; b < B; ++b) {
        memcpy(all.data() + (size_t)b * set_words, counts_or_null + (size_t)b * n_counts, n_counts * sizeof(uint64_t));
        memcpy(all.data() + (size_t)b * set_words + n_counts, sums_or_null + (size_t)b * n_sums, n_sums * sizeof(uint64_t));
    }
    return emom_restore(h, who, form, all.data(), n_snapshots);
}

}  // extern "C"
