// amc_emom.hip -- moments per energy bin (DESIGN.md section 3.17 "Moments per bin"): one pass per snapshot into a device-resident
// accumulator of 64-bit counts and signed 64-bit sums of x, x^2 and [x > 0] per (group, bin) (amc_energy_moments_accumulate), its fetch
// (amc_energy_moments_fetch) and the checkpoint entry (amc_set_energy_moments); the same kept per jackknife block ("Moments per block":
// amc_energy_moments_accumulate_blocks / _fetch_blocks, amc_set_energy_moments_blocks).  Independent of the energy histograms'
// accumulator (amc_ehist.hip): both may stand.  Allocated at its first use: a handle that never accumulates has none and launches what
// it always did.
#define AMC_KERNEL_LINKAGE static      // template instantiations, and this object's own copies of the plain kernels it launches (emom_respaced_kernel, ehist_fold_kernel)
#include "amc_internal.h"

static_assert(AMC_EMOM_X == amc::EMOM_X && AMC_EMOM_XX == amc::EMOM_XX && AMC_EMOM_POS == amc::EMOM_POS && AMC_EMOM_ALL == amc::EMOM_ALL,
              "the columns of include/amc.h and amc_emom.h");
static_assert(AMC_EMOM_BLK_MAX_WORDS <= INT32_MAX, "the words of a blocked accumulator are counted in int");

// G rows of n_bins + 4 count cells; G x C rows of n_bins sum cells behind them: one set.  All the words the accumulator holds: one
// set, or one per jackknife block.
static inline size_t emom_count_cells(int G, int n_bins) { return (size_t)G * (size_t)(n_bins + 4); }
static inline size_t emom_sum_cells(int G, int cols, int n_bins) { return (size_t)G * (size_t)cols * (size_t)n_bins; }
static inline size_t emom_set_words(const amc_handle* h)
{
    return emom_count_cells(h->emom.groups, h->emom.n_bins) + emom_sum_cells(h->emom.groups, h->emom.cols, h->emom.n_bins);
}
static inline size_t emom_words(const amc_handle* h) { return emom_set_words(h) * (size_t)(h->emom.blocks ? h->emom.blocks : 1); }

// The accumulator gone, no form fixed.  hipFree waits for whatever still writes the memory.
int emom_clear(amc_handle* h)
{
    if (!h->emom.d_emom) return AMC_OK;
    (void)hipFree(h->emom.d_emom);
    h->emom = EmomState();
    return AMC_OK;
}

int emom_respaced(amc_handle* h)
{
    if (!h->emom.d_emom) return AMC_OK;
    const int words = (int)emom_words(h);       // (every block's set; a plain one: at most 64 rows of 8196 + 64 x 3 rows of 8192 cells)
    hipLaunchKernelGGL(amc::emom_respaced_kernel, dim3(grid_for(h, words)), dim3(AMC_BLOCK), 0, h->stream, h->emom.d_emom, words,
                       (const unsigned long long*)h->lad.d_respace);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

// A blocked accumulator becomes a plain one: the blocks' sets added into the first on the stream, word by word -- counts, and signed
// sums as unsigned words modulo 2^64: exact (the memory keeps its size; the sets behind the first are no longer read).
int emom_fold(amc_handle* h)
{
    if (!h->emom.d_emom || !h->emom.blocks) return AMC_OK;
    const int words = (int)emom_set_words(h);
    hipLaunchKernelGGL(amc::ehist_fold_kernel, dim3(grid_for(h, words)), dim3(AMC_BLOCK), 0, h->stream, h->emom.d_emom, words, h->emom.blocks);
    AMC_HIP(hipGetLastError());
    h->emom.blocks = 0;
    return AMC_OK;
}

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

// Room for n_sets (the blocks; 1: plain) x (G rows of counts and G x C rows of sums) under the form; the caller fills or zeroes it.
static int emom_begin(amc_handle* h, double lo, double hi, int n_bins, int mask, double x_bound, int blocks = 0)
{
    const int G = pass_groups(h), cols = __builtin_popcount((unsigned)mask);
    unsigned long long* d = nullptr;
    AMC_HIP(hipMalloc(&d, (size_t)(blocks ? blocks : 1) * (emom_count_cells(G, n_bins) + emom_sum_cells(G, cols, n_bins)) * sizeof(unsigned long long)));
    h->emom = EmomState();
    h->emom.d_emom = d;
    h->emom.groups = G;
    h->emom.blocks = blocks;
    h->emom.n_bins = n_bins;
    h->emom.mask = mask;
    h->emom.cols = cols;
    h->emom.lo = lo;
    h->emom.hi = hi;
    h->emom.x_bound = x_bound;
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
    if (!s.d_emom) return AMC_OK;
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
    a.counts = s.d_emom;
    a.sums = s.d_emom + emom_count_cells(s.groups, s.n_bins);
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

// The cells of n_sets sets against what they must hold: every (set, group) count row sums to want[s] (a sum that wraps cannot pass:
// every partial sum is held to `want`), every sum cell is bounded by the count of its bin.  counts[(s G + g) (n_bins + 4) + cell],
// sums[((s G + g) C + c) n_bins + b].
static int emom_cells_ok(const char* who, const char* what, const uint64_t* counts, const int64_t* sums, int n_sets, int G, int n_bins, int mask,
                         const uint64_t* want)
{
    const int cols = __builtin_popcount((unsigned)mask), pos_col = (mask & AMC_EMOM_POS) ? cols - 1 : -1;
    char where[32] = "";
    for (int s = 0; s < n_sets; ++s)
        for (int g = 0; g < G; ++g) {
            if (n_sets > 1) snprintf(where, sizeof where, " of block %d", s);
            const uint64_t* row = counts + ((size_t)s * G + g) * (n_bins + 4);
            uint64_t sum = 0;
            bool over = false;
            for (int i = 0; i < n_bins + 4 && !over; ++i) {
                over = row[i] > want[s] - sum;
                if (!over) sum += row[i];
            }
            if (over || sum != want[s]) return fail(AMC_ERR_BAD_ARG, "%s: row %d%s does not sum to %s = %llu", who, g, where, what, (unsigned long long)want[s]);
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
    const EmomState& s = h->emom;
    AMC_TRY(emom_same(h, who, false, lo, hi, n_bins, mask, x_bound));
    // before anything is allocated or launched: the pass that would let a cell reach 2^31 deposits
    if (!emom_fits(h, s.n_snapshots + 1))
        return fail(AMC_ERR_STATE, "%s: %llu snapshots of %lld chains per group are all a cell holds (n_snapshots * n_chains / G < 2^31): fetch with reset", who,
                    (unsigned long long)s.n_snapshots, (long long)(h->M / pass_groups(h)));
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of an energy-histogram snapshot: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    const bool first = !h->emom.d_emom;
    if (first) {
        AMC_TRY(emom_begin(h, lo, hi, n_bins, mask, x_bound));
        if (hipMemsetAsync(h->emom.d_emom, 0, emom_words(h) * sizeof(unsigned long long), h->stream) != hipSuccess) {
            (void)emom_clear(h);
            return fail(AMC_ERR_HIP, "%s: clearing the accumulator failed", who);
        }
    }
    amc::EmomArgs a = emom_args(h);
    void* params[] = {&a};
    const int rc = launch_by_potential(h, "amc::energy_moments_kernel", (const void*)amc::energy_moments_kernel<amc::POT_DOUBLE_WELL>,
                                       (const void*)amc::energy_moments_kernel<amc::POT_HARMONIC>, hist_grid(h), params);
    // a first call that is refused (a run-time build that fails, say) leaves no accumulator and no form behind
    if (rc != AMC_OK) {
        if (first) (void)emom_clear(h);
        return rc;
    }
    h->emom.n_snapshots += 1;
    return AMC_OK;
}

int amc_energy_moments_accumulate_blocks(amc_handle* h, double lo, double hi, int n_bins, int mask, double x_bound)
{
    static const char* who = "amc_energy_moments_accumulate_blocks";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    const int B = h->blocks.n_blocks, G = pass_groups(h);
    if (!B) return fail(AMC_ERR_STATE, "%s: no partition is set (amc_set_blocks)", who);
    AMC_TRY(emom_form_ok(who, lo, hi, n_bins, mask, x_bound));
    const int cols = __builtin_popcount((unsigned)mask);
    const size_t set_words = emom_count_cells(G, n_bins) + emom_sum_cells(G, cols, n_bins);
    if ((size_t)B * set_words > (size_t)AMC_EMOM_BLK_MAX_WORDS)
        return fail(AMC_ERR_BAD_ARG, "%s: %d blocks of %d rows of %d count cells and %d x %d rows of %d sum cells are more than AMC_EMOM_BLK_MAX_WORDS = %d words",
                    who, B, G, n_bins + 4, G, cols, n_bins, AMC_EMOM_BLK_MAX_WORDS);
    AMC_TRY(emom_same(h, who, true, lo, hi, n_bins, mask, x_bound));
    // before anything is allocated or launched: the plain rule, conservative per block, and what keeps a later fold valid
    if (!emom_fits(h, h->emom.n_snapshots + 1))
        return fail(AMC_ERR_STATE, "%s: %llu snapshots of %lld chains per group are all a cell holds (n_snapshots * n_chains / G < 2^31): fetch with reset", who,
                    (unsigned long long)h->emom.n_snapshots, (long long)(h->M / G));
    // the blocked form of the u32 check: a HIP block's count cell holds at most lane_bound x AMC_BLOCK chains of one pass
    const int grid = amc::blk::grid_round(hist_grid(h), B);
    const int64_t lanes = amc::blk::lane_bound(h->M / G, B, h->blocks.chunk, G, grid, AMC_BLOCK);
    if (lanes >= ((int64_t)1 << 32) / AMC_BLOCK)
        return fail(AMC_ERR_STATE, "%s: %lld chains over a grid of %d blocks overflow a block's 32-bit cells", who, (long long)h->M, grid);
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));
    const bool first = !h->emom.d_emom;
    if (first) {
        AMC_HIP(hipStreamSynchronize(h->stream));      // (as the other blocked accumulators wait where they allocate)
        AMC_TRY(emom_begin(h, lo, hi, n_bins, mask, x_bound, B));
        if (hipMemsetAsync(h->emom.d_emom, 0, emom_words(h) * sizeof(unsigned long long), h->stream) != hipSuccess) {
            (void)emom_clear(h);
            return fail(AMC_ERR_HIP, "%s: clearing the accumulator failed", who);
        }
    }
    amc::EmomArgs a = emom_args(h);
    amc::blk::Part part = blocks_part(h);
    void* params[] = {&a, &part};
    const int rc = launch_by_potential(h, "amc::energy_moments_blocks_kernel", (const void*)amc::energy_moments_blocks_kernel<amc::POT_DOUBLE_WELL>,
                                       (const void*)amc::energy_moments_blocks_kernel<amc::POT_HARMONIC>, grid, params);
    if (rc != AMC_OK) {
        if (first) (void)emom_clear(h);
        return rc;
    }
    h->emom.n_snapshots += 1;
    return AMC_OK;
}

int amc_energy_moments_fetch(amc_handle* h, uint64_t* counts, int64_t* sums, int64_t capacity_counts, int64_t capacity_sums, int* n_groups, int* n_bins,
                             int* n_cols, double* lo, double* hi, int* mask, double* x_bound, uint64_t* n_snapshots, int reset)
{
    static const char* who = "amc_energy_moments_fetch";
    if (!h || !n_groups || !n_bins || !n_cols || !lo || !hi || !mask || !x_bound || !n_snapshots) return fail(AMC_ERR_BAD_ARG, "%s: NULL argument", who);
    const EmomState& s = h->emom;
    *n_groups = s.d_emom ? s.groups : pass_groups(h);
    *n_bins = s.n_bins;
    *n_cols = s.cols;
    *lo = s.lo;
    *hi = s.hi;
    *mask = s.mask;
    *x_bound = s.x_bound;
    *n_snapshots = 0;
    if (!s.d_emom) return AMC_OK;       // nothing accumulated: no cells (the arrays may be NULL), no form
    if (!counts && !sums) return AMC_OK;        // the sizes alone, for a caller about to allocate: nothing waits, nothing is copied, nothing is reset
    if (!counts || !sums) return fail(AMC_ERR_BAD_ARG, "%s: counts and sums are given together, or neither", who);
    const size_t n_counts = emom_count_cells(s.groups, s.n_bins), n_sums = emom_sum_cells(s.groups, s.cols, s.n_bins);
    if (capacity_counts < (int64_t)n_counts || capacity_sums < (int64_t)n_sums)
        return fail(AMC_ERR_BAD_ARG, "%s: capacities %lld and %lld, the accumulator has %d rows of %d count cells and %d x %d rows of %d sum cells", who,
                    (long long)capacity_counts, (long long)capacity_sums, s.groups, s.n_bins + 4, s.groups, s.cols, s.n_bins);
    AMC_HIP(hipSetDevice(h->device));
    if (s.blocks) {                     // a blocked accumulator: the sum over its blocks, formed here behind the copy (modulo 2^64: exact)
        const size_t set_words = n_counts + n_sums;
        std::vector<uint64_t> all(emom_words(h));
        AMC_TRY(copy_to_host_sync(h, all.data(), s.d_emom, all.size() * sizeof(uint64_t)));
        for (size_t i = 0; i < set_words; ++i) {
            uint64_t t = 0;
            for (int b = 0; b < s.blocks; ++b) t += all[(size_t)b * set_words + i];
            if (i < n_counts) counts[i] = t;
            else sums[i - n_counts] = (int64_t)t;
        }
    } else {
        AMC_HIP(hipMemcpyAsync(sums, s.d_emom + n_counts, n_sums * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        AMC_TRY(copy_to_host_sync(h, counts, s.d_emom, n_counts * sizeof(unsigned long long)));
    }
    uint64_t row0 = 0;
    for (int i = 0; i < s.n_bins + 4; ++i) row0 += counts[i];
    *n_snapshots = row0 / (uint64_t)(h->M / s.groups);      // every chain of a group lands in exactly one cell of its row
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
    if (!s.d_emom || !s.blocks) return fail(AMC_ERR_STATE, "%s: no accumulator kept per jackknife block stands (amc_energy_moments_accumulate_blocks)", who);
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
    const size_t n_counts = emom_count_cells(G, s.n_bins), n_sums = emom_sum_cells(G, s.cols, s.n_bins), set_words = n_counts + n_sums;
    if (capacity_counts < (int64_t)(B * n_counts) || capacity_sums < (int64_t)(B * n_sums))
        return fail(AMC_ERR_BAD_ARG, "%s: capacities %lld and %lld, the accumulator has %d blocks of %d rows of %d count cells and %d x %d rows of %d sum cells",
                    who, (long long)capacity_counts, (long long)capacity_sums, B, G, s.n_bins + 4, G, s.cols, s.n_bins);
    AMC_HIP(hipSetDevice(h->device));
    std::vector<uint64_t> all(emom_words(h));
    AMC_TRY(copy_to_host_sync(h, all.data(), s.d_emom, all.size() * sizeof(uint64_t)));
    for (int b = 0; b < B; ++b) {           // the sets de-interleaved: all counts, then all sums
        memcpy(counts + (size_t)b * n_counts, all.data() + (size_t)b * set_words, n_counts * sizeof(uint64_t));
        memcpy(sums + (size_t)b * n_sums, all.data() + (size_t)b * set_words + n_counts, n_sums * sizeof(uint64_t));
    }
    // a block without a local ladder holds nothing; the snapshots from the first block that has one
    const amc::blk::Part part = blocks_part(h);
    const size_t row = (size_t)s.n_bins + 4;
    for (int b = 0; b < B; ++b) {
        const uint64_t ladders = (uint64_t)amc::blk::ladders_in_block(part, b, h->M / G);
        if (!ladders) continue;
        uint64_t row0 = 0;
        for (size_t i = 0; i < row; ++i) row0 += counts[(size_t)b * n_counts + i];
        *n_snapshots = row0 / ladders;
        break;
    }
    h->emom.n_snapshots = *n_snapshots;                     // (a respacing that was taken has zeroed the cells: the count follows them)
    if (reset) return emom_clear(h);
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
    const int G = pass_groups(h), cols = __builtin_popcount((unsigned)mask);
    const uint64_t per_group = (uint64_t)(h->M / G);
    if (!emom_fits(h, n_snapshots))
        return fail(AMC_ERR_BAD_ARG, "%s: n_snapshots * n_chains / G = %llu * %llu is not below 2^31, all a cell holds", who, (unsigned long long)n_snapshots,
                    (unsigned long long)per_group);
    const uint64_t want = n_snapshots * per_group;
    AMC_TRY(emom_cells_ok(who, "n_snapshots * n_chains / G", counts_or_null, sums_or_null, 1, G, n_bins, mask, &want));
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(emom_clear(h));             // (an accumulator of either form is replaced by a plain one)
    AMC_TRY(emom_begin(h, lo, hi, n_bins, mask, x_bound));
    const size_t n_counts = emom_count_cells(G, n_bins), n_sums = emom_sum_cells(G, cols, n_bins);
    // (the caller's buffers are only valid during the call)
    int rc = copy_to_device_sync(h, h->emom.d_emom, counts_or_null, n_counts * sizeof(unsigned long long));
    if (rc == AMC_OK) rc = copy_to_device_sync(h, h->emom.d_emom + n_counts, sums_or_null, n_sums * sizeof(unsigned long long));
    if (rc != AMC_OK) {
        (void)emom_clear(h);
        return rc;
    }
    h->emom.n_snapshots = n_snapshots;
    return AMC_OK;
}

int amc_set_energy_moments_blocks(amc_handle* h, double lo, double hi, int n_bins, int mask, double x_bound, const uint64_t* counts_or_null,
                                  const int64_t* sums_or_null, int n_blocks, uint64_t n_snapshots)
{
    static const char* who = "amc_set_energy_moments_blocks";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    const int B = h->blocks.n_blocks, G = pass_groups(h);
    if (!B) return fail(AMC_ERR_STATE, "%s: no partition is set (amc_set_blocks)", who);
    if (!counts_or_null || !sums_or_null || n_snapshots == 0) {
        AMC_HIP(hipSetDevice(h->device));
        return emom_clear(h);
    }
    if (n_blocks != B) return fail(AMC_ERR_BAD_ARG, "%s: n_blocks = %d, the partition has %d blocks", who, n_blocks, B);
    AMC_TRY(emom_form_ok(who, lo, hi, n_bins, mask, x_bound));
    const int cols = __builtin_popcount((unsigned)mask);
    const size_t n_counts = emom_count_cells(G, n_bins), n_sums = emom_sum_cells(G, cols, n_bins), set_words = n_counts + n_sums;
    if ((size_t)B * set_words > (size_t)AMC_EMOM_BLK_MAX_WORDS)
        return fail(AMC_ERR_BAD_ARG, "%s: %d blocks of %d rows of %d count cells and %d x %d rows of %d sum cells are more than AMC_EMOM_BLK_MAX_WORDS = %d words",
                    who, B, G, n_bins + 4, G, cols, n_bins, AMC_EMOM_BLK_MAX_WORDS);
    if (!emom_fits(h, n_snapshots))
        return fail(AMC_ERR_BAD_ARG, "%s: n_snapshots * n_chains / G = %llu * %llu is not below 2^31, all a cell holds", who, (unsigned long long)n_snapshots,
                    (unsigned long long)(h->M / G));
    // every (block, group) row holds the block's ladders once per snapshot; a block without a local ladder holds nothing
    const amc::blk::Part part = blocks_part(h);
    uint64_t want[AMC_MAX_JK_BLOCKS];
    for (int b = 0; b < B; ++b) want[b] = n_snapshots * (uint64_t)amc::blk::ladders_in_block(part, b, h->M / G);      // (at most n_snapshots * n_chains / G < 2^31)
    AMC_TRY(emom_cells_ok(who, "n_snapshots * (local ladders of the block)", counts_or_null, sums_or_null, B, G, n_bins, mask, want));
    std::vector<uint64_t> all((size_t)B * set_words);      // the sets interleaved: counts and sums of block b side by side
    for (int b = 0; b < B; ++b) {
        memcpy(all.data() + (size_t)b * set_words, counts_or_null + (size_t)b * n_counts, n_counts * sizeof(uint64_t));
        memcpy(all.data() + (size_t)b * set_words + n_counts, sums_or_null + (size_t)b * n_sums, n_sums * sizeof(uint64_t));
    }
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(emom_clear(h));
    AMC_TRY(emom_begin(h, lo, hi, n_bins, mask, x_bound, B));
    const int rc = copy_to_device_sync(h, h->emom.d_emom, all.data(), all.size() * sizeof(uint64_t));      // `all` is only valid during the call
    if (rc != AMC_OK) {
        (void)emom_clear(h);
        return rc;
    }
    h->emom.n_snapshots = n_snapshots;
    return AMC_OK;
}

}  // extern "C"
