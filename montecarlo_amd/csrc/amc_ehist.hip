// amc_ehist.hip -- energy histograms per group: one pass per snapshot into a device-resident accumulator of
// 64-bit counts (amc_energy_histogram_accumulate), its fetch (amc_energy_histogram_fetch) and the checkpoint entry
// (amc_set_energy_histogram); the same kept per jackknife block (amc_energy_histogram_accumulate_blocks / _fetch_blocks,
// amc_set_energy_histogram_blocks).  The groups are those of the time correlation: the rungs of the ladder, ONE group without a ladder.
// The accumulator is allocated at its first use: a handle that never accumulates has none and launches what it always did.
// In front of the entries: what the life cycle of every accumulator over the energy bins shares beyond amc_internal.h's bins_clear /
// bins_begin / bins_pass -- the two plain kernels' launches, the checks and the fetches' host arithmetic -- for the moments per bin
// (amc_emom.hip) too.
#define AMC_KERNEL_LINKAGE static      // template instantiations, and the plain kernels of both accumulators over the energy bins (ehist_respaced_kernel, ehist_fold_kernel)
#include "amc_internal.h"

static_assert(AMC_EHIST_BLK_MAX_CELLS <= INT32_MAX && AMC_EMOM_BLK_MAX_WORDS <= INT32_MAX, "the words of a blocked accumulator are counted in int");

int bins_respaced(amc_handle* h, const BinsState& s)
{
    if (!s.d_words) return AMC_OK;
    const int words = (int)bins_words(s);       // (every block's set; a plain one: at most 64 rows of 8196 + 64 x 3 rows of 8192 cells)
    hipLaunchKernelGGL(amc::ehist_respaced_kernel, dim3(grid_for(h, words)), dim3(AMC_BLOCK), 0, h->stream, s.d_words, words,
                       (const unsigned long long*)h->lad.d_respace);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

// A blocked accumulator becomes a plain one: the blocks' sets added into the first on the stream, word by word -- counts, and signed
// sums as unsigned words modulo 2^64: exact (the memory keeps its size; the sets behind the first are no longer read).
int bins_fold(amc_handle* h, BinsState& s)
{
    if (!s.d_words || !s.blocks) return AMC_OK;
    const int words = (int)bins_set_words(s);
    hipLaunchKernelGGL(amc::ehist_fold_kernel, dim3(grid_for(h, words)), dim3(AMC_BLOCK), 0, h->stream, s.d_words, words, s.blocks);
    AMC_HIP(hipGetLastError());
    s.blocks = 0;
    s.by_family = false;
    return AMC_OK;
}

// The partition a blocked entry works under: the ladders' (amc_set_blocks), or -- the two exclude each other, and only where the entry
// keeps `families` -- the one over an annealed population's families (amc_set_anneal_blocks), whose blocks are a property of the
// chain, not of the slot.
int bins_partition(const amc_handle* h, const char* who, bool families, int* n_blocks, bool* by_family)
{
    *by_family = families && !h->blocks.n_blocks && h->ann.blk_B;
    *n_blocks = *by_family ? h->ann.blk_B : h->blocks.n_blocks;
    if (!*n_blocks) return fail(AMC_ERR_STATE, "%s: no partition is set (amc_set_blocks)", who);
    if (*by_family && pass_groups(h) != 1)
        return fail(AMC_ERR_STATE, "%s: blocks of families belong to one population at one shared beta, the handle has a ladder", who);
    return AMC_OK;
}

// A HIP block's u32 LDS cell holds its share of ONE pass: at most ceil(M / grid) chains, for the grid actually launched ...
int bins_u32_ok(const amc_handle* h, const char* who, int grid)
{
    if ((h->M + grid - 1) / grid >= (int64_t)1 << 32)
        return fail(AMC_ERR_STATE, "%s: %lld chains over a grid of %d blocks overflow a block's 32-bit cells", who, (long long)h->M, grid);
    return AMC_OK;
}
// ... and in a pass per jackknife block, whose grid (*grid: hist_grid's, rounded to the blocks) it is, at most lane_bound x AMC_BLOCK.
int bins_u32_blocked_ok(const amc_handle* h, const char* who, int n_blocks, int* grid)
{
    const int G = pass_groups(h);
    *grid = amc::blk::grid_round(hist_grid(h), n_blocks);
    const int64_t lanes = amc::blk::lane_bound(h->M / G, n_blocks, h->blocks.chunk, G, *grid, AMC_BLOCK);
    if (lanes >= ((int64_t)1 << 32) / AMC_BLOCK)
        return fail(AMC_ERR_STATE, "%s: %lld chains over a grid of %d blocks overflow a block's 32-bit cells", who, (long long)h->M, *grid);
    return AMC_OK;
}

// One count row of n cells against the chains it must hold: row g, of block s where s >= 0 -- or, g < 0, all the cells of an accumulator
// per block of families as ONE row.  (a sum that wraps cannot pass: every partial sum is held to `want`)
int bins_row_sum(const char* who, const char* what, const uint64_t* row, size_t n, uint64_t want, int g, int s)
{
    uint64_t sum = 0;
    bool over = false;
    for (size_t i = 0; i < n && !over; ++i) {
        over = row[i] > want - sum;
        if (!over) sum += row[i];
    }
    if (!over && sum == want) return AMC_OK;
    char which[48];
    if (g < 0) snprintf(which, sizeof which, "the cells do");
    else if (s >= 0) snprintf(which, sizeof which, "row %d of block %d does", g, s);
    else snprintf(which, sizeof which, "row %d does", g);
    return fail(AMC_ERR_BAD_ARG, "%s: %s not sum to %s = %llu", who, which, what, (unsigned long long)want);
}

// A blocked accumulator fetched as a plain one: the sum over its blocks' sets, formed here behind the copy (modulo 2^64: exact).
int bins_merge_blocks(amc_handle* h, const BinsState& s, uint64_t* set)
{
    const size_t words = bins_set_words(s);
    std::vector<uint64_t> all(bins_words(s));
    AMC_TRY(copy_to_host_sync(h, all.data(), s.d_words, all.size() * sizeof(uint64_t)));
    for (size_t i = 0; i < words; ++i) {
        uint64_t t = 0;
        for (int b = 0; b < s.blocks; ++b) t += all[(size_t)b * words + i];
        set[i] = t;
    }
    return AMC_OK;
}

// The snapshots that fetched count rows hold, every chain landing in exactly one cell of its row.  A plain set: row 0 over the chains of
// a group.  `blocked`, counts[B][G][n_bins + tail]: a block without a local ladder holds nothing, so the first block that has one --
// or, per block of families, whose sizes change at every resampling, all the cells over all the chains.
uint64_t bins_snapshots(const amc_handle* h, const BinsState& s, const uint64_t* counts, bool blocked)
{
    const size_t row = (size_t)(s.n_bins + s.tail);
    auto sum = [&](const uint64_t* c, size_t n) {
        uint64_t t = 0;
        for (size_t i = 0; i < n; ++i) t += c[i];
        return t;
    };
    if (!blocked) return sum(counts, row) / (uint64_t)(h->M / s.groups);
    if (s.by_family) return sum(counts, (size_t)s.blocks * row) / (uint64_t)h->M;
    const amc::blk::Part part = blocks_part(h);
    for (int b = 0; b < s.blocks; ++b) {
        const uint64_t ladders = (uint64_t)amc::blk::ladders_in_block(part, b, h->M / s.groups);
        if (ladders) return sum(counts + (size_t)b * s.groups * row, row) / ladders;
    }
    return 0;
}

// The form of an accumulator begun now: G rows of n_bins + 3 cells, in one set (plain) or one per block.
static EhistState ehist_form(const amc_handle* h, double lo, double hi, int n_bins, int blocks = 0, bool by_family = false)
{
    EhistState f;
    f.n_bins = n_bins;
    f.groups = pass_groups(h);
    f.blocks = blocks;
    f.by_family = by_family;
    f.tail = 3;
    f.lo = lo;
    f.hi = hi;
    return f;
}

static int ehist_cap_ok(const char* who, const EhistState& f)
{
    if (bins_words(f) > (size_t)AMC_EHIST_BLK_MAX_CELLS)
        return fail(AMC_ERR_BAD_ARG, "%s: %d blocks of %d rows of %d cells are more than AMC_EHIST_BLK_MAX_CELLS = %d cells", who, f.blocks, f.groups,
                    f.n_bins + 3, AMC_EHIST_BLK_MAX_CELLS);
    return AMC_OK;
}

// What both accumulate entries ask of a standing accumulator: the caller's form, the caller's bins.
static int ehist_same(const amc_handle* h, const char* who, bool blocked, double lo, double hi, int n_bins)
{
    if (!h->ehist.d_words) return AMC_OK;
    if ((h->ehist.blocks != 0) != blocked)
        return fail(AMC_ERR_STATE, "%s: the accumulator is %s (amc_energy_histogram_fetch with reset frees it)", who,
                    blocked ? "a plain one, not kept per jackknife block" : "kept per jackknife block");
    if (n_bins != h->ehist.n_bins || lo != h->ehist.lo || hi != h->ehist.hi)
        return fail(AMC_ERR_STATE, "%s: the accumulator has other bins: [%g, %g) in %d (amc_energy_histogram_fetch with reset frees them)", who,
                    h->ehist.lo, h->ehist.hi, h->ehist.n_bins);
    return AMC_OK;
}

static amc::EhistArgs ehist_args(const amc_handle* h)
{
    amc::EhistArgs a = {};
    a.x = h->d_x;
    a.counts = h->ehist.d_words;
    a.n_chains = h->M;
    a.lo = h->ehist.lo;
    a.hi = h->ehist.hi;
    a.inv_w = (double)h->ehist.n_bins / (h->ehist.hi - h->ehist.lo);
    a.n_groups = h->ehist.groups;
    a.n_bins = h->ehist.n_bins;
    return a;
}

extern "C" {

int amc_energy_histogram_accumulate(amc_handle* h, double lo, double hi, int n_bins)
{
    static const char* who = "amc_energy_histogram_accumulate";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    if (!hist_args_ok(who, lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    AMC_TRY(ehist_same(h, who, false, lo, hi, n_bins));
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of a bridge snapshot: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    const int grid = hist_grid(h);
    AMC_TRY(bins_u32_ok(h, who, grid));
    const bool first = !h->ehist.d_words;
    if (first) AMC_TRY(bins_begin(h, h->ehist, ehist_form(h, lo, hi, n_bins), who, true));
    amc::EhistArgs a = ehist_args(h);
    void* params[] = {&a};
    return bins_pass(h, h->ehist, first, "amc::energy_histogram_kernel", (const void*)amc::energy_histogram_kernel<amc::POT_DOUBLE_WELL>,
                     (const void*)amc::energy_histogram_kernel<amc::POT_HARMONIC>, grid, params);
}

// Under amc_set_blocks one pass of energy_histogram_blocks_kernel into counts[B][G][n_bins + 3]; under amc_set_anneal_blocks one of
// energy_histogram_families_kernel into counts[B][n_bins + 3].
int amc_energy_histogram_accumulate_blocks(amc_handle* h, double lo, double hi, int n_bins)
{
    static const char* who = "amc_energy_histogram_accumulate_blocks";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    if (!hist_args_ok(who, lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    int B = 0, grid = hist_grid(h);
    bool by_family = false;
    AMC_TRY(bins_partition(h, who, true, &B, &by_family));
    const EhistState form = ehist_form(h, lo, hi, n_bins, B, by_family);
    AMC_TRY(ehist_cap_ok(who, form));
    AMC_TRY(ehist_same(h, who, true, lo, hi, n_bins));
    if (by_family) AMC_TRY(bins_u32_ok(h, who, grid));      // (the block is the chain's: the plain pass's grid and share)
    else AMC_TRY(bins_u32_blocked_ok(h, who, B, &grid));
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));
    const bool first = !h->ehist.d_words;
    if (first) AMC_TRY(bins_begin(h, h->ehist, form, who, true));
    amc::EhistArgs a = ehist_args(h);
    if (by_family) {
        const uint32_t* fam = h->ann.d_fam;
        uint32_t chunk = (uint32_t)std::min<int64_t>(h->ann.blk_chunk, 0xFFFFFFFFll);
        void* params[] = {&a, &fam, &chunk, &B};
        return bins_pass(h, h->ehist, first, "amc::energy_histogram_families_kernel", (const void*)amc::energy_histogram_families_kernel<amc::POT_DOUBLE_WELL>,
                         (const void*)amc::energy_histogram_families_kernel<amc::POT_HARMONIC>, grid, params);
    }
    amc::blk::Part part = blocks_part(h);
    void* params[] = {&a, &part};
    return bins_pass(h, h->ehist, first, "amc::energy_histogram_blocks_kernel", (const void*)amc::energy_histogram_blocks_kernel<amc::POT_DOUBLE_WELL>,
                     (const void*)amc::energy_histogram_blocks_kernel<amc::POT_HARMONIC>, grid, params);
}

int amc_energy_histogram_fetch(amc_handle* h, uint64_t* counts, int64_t capacity_cells, int* n_groups, int* n_bins, double* lo, double* hi,
                               uint64_t* n_snapshots, int reset)
{
    if (!h || !n_groups || !n_bins || !lo || !hi || !n_snapshots) return fail(AMC_ERR_BAD_ARG, "amc_energy_histogram_fetch: NULL argument");
    const EhistState& s = h->ehist;     // nothing accumulated: no counts (the array may be NULL), no bins
    *n_groups = s.d_words ? s.groups : pass_groups(h);
    *n_bins = s.n_bins;
    *lo = s.lo;
    *hi = s.hi;
    *n_snapshots = 0;
    if (!s.d_words || !counts) return AMC_OK;       // (the sizes alone, for a caller about to allocate: nothing waits, nothing is copied, nothing is reset)
    const size_t cells = bins_set_words(s);
    if (capacity_cells < (int64_t)cells)
        return fail(AMC_ERR_BAD_ARG, "amc_energy_histogram_fetch: capacity_cells = %lld, the accumulator has %d rows of %d cells", (long long)capacity_cells,
                    s.groups, s.n_bins + 3);
    AMC_HIP(hipSetDevice(h->device));
    if (s.blocks) AMC_TRY(bins_merge_blocks(h, s, counts));
    else AMC_TRY(copy_to_host_sync(h, counts, s.d_words, cells * sizeof(unsigned long long)));
    *n_snapshots = bins_snapshots(h, s, counts, false);
    if (reset) return ehist_clear(h);
    return AMC_OK;
}

int amc_energy_histogram_fetch_blocks(amc_handle* h, uint64_t* counts, int64_t capacity_cells, int* n_blocks, int* n_groups, int* n_bins, double* lo,
                                      double* hi, uint64_t* n_snapshots, int reset)
{
    static const char* who = "amc_energy_histogram_fetch_blocks";
    if (!h || !n_blocks || !n_groups || !n_bins || !lo || !hi || !n_snapshots) return fail(AMC_ERR_BAD_ARG, "%s: NULL argument", who);
    const EhistState& s = h->ehist;
    if (!s.d_words || !s.blocks)
        return fail(AMC_ERR_STATE, "%s: no accumulator kept per jackknife block stands (amc_energy_histogram_accumulate_blocks)", who);
    *n_blocks = s.blocks;
    *n_groups = s.groups;
    *n_bins = s.n_bins;
    *lo = s.lo;
    *hi = s.hi;
    *n_snapshots = 0;
    if (!counts) return AMC_OK;         // the sizes alone: nothing waits, nothing is copied, nothing is reset
    const size_t cells = bins_words(s);
    if (capacity_cells < (int64_t)cells)
        return fail(AMC_ERR_BAD_ARG, "%s: capacity_cells = %lld, the accumulator has %d blocks of %d rows of %d cells", who, (long long)capacity_cells,
                    s.blocks, s.groups, s.n_bins + 3);
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(copy_to_host_sync(h, counts, s.d_words, cells * sizeof(unsigned long long)));
    *n_snapshots = bins_snapshots(h, s, counts, true);
    if (reset) return ehist_clear(h);
    return AMC_OK;
}

int amc_set_energy_histogram(amc_handle* h, double lo, double hi, int n_bins, const uint64_t* counts_or_null, uint64_t n_snapshots)
{
    static const char* who = "amc_set_energy_histogram";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    if (!counts_or_null || n_snapshots == 0) {
        AMC_HIP(hipSetDevice(h->device));
        return ehist_clear(h);
    }
    if (!hist_args_ok(who, lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    const int G = pass_groups(h);
    const uint64_t per_group = (uint64_t)(h->M / G);
    if (n_snapshots > UINT64_MAX / per_group) return fail(AMC_ERR_BAD_ARG, "%s: n_snapshots * n_chains / G does not fit 64 bits", who);
    const uint64_t want = n_snapshots * per_group;
    for (int g = 0; g < G; ++g) AMC_TRY(bins_row_sum(who, "n_snapshots * n_chains / G", counts_or_null + (size_t)g * (n_bins + 3), (size_t)n_bins + 3, want, g, -1));
    AMC_HIP(hipSetDevice(h->device));
    if (h->ehist.d_words && (h->ehist.blocks || h->ehist.groups != G || h->ehist.n_bins != n_bins)) AMC_TRY(ehist_clear(h));
    if (!h->ehist.d_words) AMC_TRY(bins_begin(h, h->ehist, ehist_form(h, lo, hi, n_bins), who, false));
    h->ehist.lo = lo;
    h->ehist.hi = hi;
    return copy_to_device_sync(h, h->ehist.d_words, counts_or_null, bins_words(h->ehist) * sizeof(unsigned long long));      // the caller's buffer is only valid during the call
}

int amc_set_energy_histogram_blocks(amc_handle* h, double lo, double hi, int n_bins, const uint64_t* counts_or_null, int n_blocks, uint64_t n_snapshots)
{
    static const char* who = "amc_set_energy_histogram_blocks";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    int B = 0;
    bool by_family = false;
    AMC_TRY(bins_partition(h, who, true, &B, &by_family));
    if (!counts_or_null || n_snapshots == 0) {
        AMC_HIP(hipSetDevice(h->device));
        return ehist_clear(h);
    }
    if (n_blocks != B) return fail(AMC_ERR_BAD_ARG, "%s: n_blocks = %d, the partition has %d blocks", who, n_blocks, B);
    if (!hist_args_ok(who, lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    const EhistState form = ehist_form(h, lo, hi, n_bins, B, by_family);
    AMC_TRY(ehist_cap_ok(who, form));
    const size_t row = (size_t)n_bins + 3;
    if (by_family) {                    // a block's share changes with every resampling: all the cells hold every chain once per snapshot
        if (n_snapshots > UINT64_MAX / (uint64_t)h->M) return fail(AMC_ERR_BAD_ARG, "%s: n_snapshots * n_chains does not fit 64 bits", who);
        const uint64_t want = n_snapshots * (uint64_t)h->M;
        AMC_TRY(bins_row_sum(who, "n_snapshots * n_chains", counts_or_null, (size_t)B * row, want, -1, -1));
    } else {                            // every (block, group) row holds the block's ladders once per snapshot; a block without a local ladder holds nothing
        const amc::blk::Part part = blocks_part(h);
        uint64_t want[AMC_MAX_JK_BLOCKS];
        for (int b = 0; b < B; ++b) {
            const uint64_t ladders = (uint64_t)amc::blk::ladders_in_block(part, b, h->M / form.groups);
            if (ladders && n_snapshots > UINT64_MAX / ladders) return fail(AMC_ERR_BAD_ARG, "%s: n_snapshots * (ladders of block %d) does not fit 64 bits", who, b);
            want[b] = n_snapshots * ladders;
        }
        for (int b = 0; b < B; ++b)
            for (int g = 0; g < form.groups; ++g)
                AMC_TRY(bins_row_sum(who, "n_snapshots * (local ladders of the block)", counts_or_null + ((size_t)b * form.groups + g) * row, row, want[b], g, b));
    }
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(ehist_clear(h));
    AMC_TRY(bins_begin(h, h->ehist, form, who, false));
    return copy_to_device_sync(h, h->ehist.d_words, counts_or_null, bins_words(h->ehist) * sizeof(unsigned long long));      // the caller's buffer is only valid during the call
}

}  // extern "C"
