// amc_ehist.hip -- energy histograms per group: one pass per snapshot into a device-resident accumulator of
// 64-bit counts (amc_energy_histogram_accumulate), its fetch (amc_energy_histogram_fetch) and the checkpoint entry
// (amc_set_energy_histogram); the same kept per jackknife block (amc_energy_histogram_accumulate_blocks / _fetch_blocks,
// amc_set_energy_histogram_blocks).  The groups are those of the time correlation: the rungs of the ladder, ONE group without a ladder.
// The accumulator is allocated at its first use: a handle that never accumulates has none and launches what it always did.
#define AMC_KERNEL_LINKAGE static      // template instantiations, and this object's own copies of the plain kernels it launches (ehist_respaced_kernel, ehist_fold_kernel)
#include "amc_internal.h"

static_assert(AMC_EHIST_BLK_MAX_CELLS <= INT32_MAX, "the cells of a blocked accumulator are counted in int");

// One set of rows: G rows of n_bins + 3 cells; all the cells the accumulator holds: one set, or one per jackknife block.
static inline size_t ehist_set_cells(const amc_handle* h) { return (size_t)h->ehist.groups * (size_t)(h->ehist.n_bins + 3); }
static inline size_t ehist_cells(const amc_handle* h) { return ehist_set_cells(h) * (size_t)(h->ehist.blocks ? h->ehist.blocks : 1); }

// The accumulator gone, no bins fixed, no form.  hipFree waits for whatever still writes the memory.
int ehist_clear(amc_handle* h)
{
    if (!h->ehist.d_ehist) return AMC_OK;
    (void)hipFree(h->ehist.d_ehist);
    h->ehist = EhistState();
    return AMC_OK;
}

int ehist_respaced(amc_handle* h)
{
    if (!h->ehist.d_ehist) return AMC_OK;
    const int cells = (int)ehist_cells(h);      // (every block's rows)
    hipLaunchKernelGGL(amc::ehist_respaced_kernel, dim3(grid_for(h, cells)), dim3(AMC_BLOCK), 0, h->stream, h->ehist.d_ehist, cells,
                       (const unsigned long long*)h->lad.d_respace);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

// A blocked accumulator becomes a plain one: the blocks' rows added into the first set on the stream, exact integer sums (the memory
// keeps its size; the sets behind the first are no longer read).
int ehist_fold(amc_handle* h)
{
    if (!h->ehist.d_ehist || !h->ehist.blocks) return AMC_OK;
    const int cells = (int)ehist_set_cells(h);
    hipLaunchKernelGGL(amc::ehist_fold_kernel, dim3(grid_for(h, cells)), dim3(AMC_BLOCK), 0, h->stream, h->ehist.d_ehist, cells, h->ehist.blocks);
    AMC_HIP(hipGetLastError());
    h->ehist.blocks = 0;
    h->ehist.by_family = false;
    return AMC_OK;
}

// The partition a blocked entry works under: the ladders' (amc_set_blocks), or -- the two exclude each other -- the one over an annealed
// population's families (amc_set_anneal_blocks), whose blocks are a property of the chain, not of the slot.
static inline bool ehist_by_family(const amc_handle* h) { return !h->blocks.n_blocks && h->ann.blk_B; }
static inline int ehist_partition_blocks(const amc_handle* h) { return h->blocks.n_blocks ? h->blocks.n_blocks : h->ann.blk_B; }


// Room for n_sets (the blocks; 1: plain) x G rows of n_bins + 3 cells under the bins (lo, hi, n_bins); the caller fills or zeroes it.
static int ehist_begin(amc_handle* h, double lo, double hi, int n_bins, int blocks = 0)
{
    const int G = pass_groups(h);
    unsigned long long* d = nullptr;
    AMC_HIP(hipMalloc(&d, (size_t)(blocks ? blocks : 1) * (size_t)G * (size_t)(n_bins + 3) * sizeof(unsigned long long)));
    h->ehist.d_ehist = d;
    h->ehist.groups = G;
    h->ehist.n_bins = n_bins;
    h->ehist.blocks = blocks;
    h->ehist.lo = lo;
    h->ehist.hi = hi;
    return AMC_OK;
}

// What both accumulate entries ask of a standing accumulator: the caller's form, the caller's bins.
static int ehist_same(const amc_handle* h, const char* who, bool blocked, double lo, double hi, int n_bins)
{
    if (!h->ehist.d_ehist) return AMC_OK;
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
    a.counts = h->ehist.d_ehist;
    a.n_chains = h->M;
    a.lo = h->ehist.lo;
    a.hi = h->ehist.hi;
    a.inv_w = (double)h->ehist.n_bins / (h->ehist.hi - h->ehist.lo);
    a.n_groups = h->ehist.groups;
    a.n_bins = h->ehist.n_bins;
    return a;
}

// Every (set, group) row against the chains it must hold: counts[(s * G + g) * (n_bins + 3) + cell], row sums want[s] each.
// (a sum that wraps cannot pass: every partial sum is held to `want`)
static int ehist_rows_sum(const char* who, const char* what, const uint64_t* counts, int n_sets, int G, int n_bins, const uint64_t* want)
{
    for (int s = 0; s < n_sets; ++s)
        for (int g = 0; g < G; ++g) {
            uint64_t sum = 0;
            bool over = false;
            for (int i = 0; i < n_bins + 3; ++i) {
                const uint64_t c = counts[((size_t)s * G + g) * (n_bins + 3) + i];
                over = over || c > want[s] - sum;
                if (over) break;
                sum += c;
            }
            if (over || sum != want[s]) {
                if (n_sets > 1) return fail(AMC_ERR_BAD_ARG, "%s: row %d of block %d does not sum to %s = %llu", who, g, s, what, (unsigned long long)want[s]);
                return fail(AMC_ERR_BAD_ARG, "%s: row %d does not sum to %s = %llu", who, g, what, (unsigned long long)want[s]);
            }
        }
    return AMC_OK;
}

// amc_energy_histogram_accumulate_blocks under amc_set_anneal_blocks: one pass of energy_histogram_families_kernel into counts[B][n_bins + 3].
static int ehist_accumulate_families(amc_handle* h, const char* who, double lo, double hi, int n_bins)
{
    // a HIP block's u32 LDS cell holds its share of ONE pass: at most ceil(M / grid) chains (as the plain pass)
    const int grid = hist_grid(h);
    if ((h->M + grid - 1) / grid >= (int64_t)1 << 32)
        return fail(AMC_ERR_STATE, "%s: %lld chains over a grid of %d blocks overflow a block's 32-bit cells", who, (long long)h->M, grid);
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));
    const bool first = !h->ehist.d_ehist;
    if (first) {
        AMC_HIP(hipStreamSynchronize(h->stream));      // (as the other blocked accumulators wait where they allocate)
        AMC_TRY(ehist_begin(h, lo, hi, n_bins, h->ann.blk_B));
        h->ehist.by_family = true;
        if (hipMemsetAsync(h->ehist.d_ehist, 0, ehist_cells(h) * sizeof(unsigned long long), h->stream) != hipSuccess) {
            (void)ehist_clear(h);
            return fail(AMC_ERR_HIP, "%s: clearing the accumulator failed", who);
        }
    }
    amc::EhistArgs a = ehist_args(h);
    const uint32_t* fam = h->ann.d_fam;
    uint32_t chunk = (uint32_t)std::min<int64_t>(h->ann.blk_chunk, 0xFFFFFFFFll);
    int B = h->ann.blk_B;
    void* params[] = {&a, &fam, &chunk, &B};
    const int rc = launch_by_potential(h, "amc::energy_histogram_families_kernel", (const void*)amc::energy_histogram_families_kernel<amc::POT_DOUBLE_WELL>,
                                       (const void*)amc::energy_histogram_families_kernel<amc::POT_HARMONIC>, grid, params);
    if (rc != AMC_OK && first) (void)ehist_clear(h);
    return rc;
}

extern "C" {

int amc_energy_histogram_accumulate(amc_handle* h, double lo, double hi, int n_bins)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_energy_histogram_accumulate: NULL handle");
    if (!hist_args_ok("amc_energy_histogram_accumulate", lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    AMC_TRY(ehist_same(h, "amc_energy_histogram_accumulate", false, lo, hi, n_bins));
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of a bridge snapshot: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    const bool first = !h->ehist.d_ehist;
    if (first) {
        AMC_TRY(ehist_begin(h, lo, hi, n_bins));
        if (hipMemsetAsync(h->ehist.d_ehist, 0, ehist_cells(h) * sizeof(unsigned long long), h->stream) != hipSuccess) {
            (void)ehist_clear(h);
            return fail(AMC_ERR_HIP, "amc_energy_histogram_accumulate: clearing the accumulator failed");
        }
    }
    // a block's u32 LDS cell holds its share of ONE pass: at most ceil(M / grid) chains, for the grid actually launched
    const int grid = hist_grid(h);
    if ((h->M + grid - 1) / grid >= (int64_t)1 << 32) {
        if (first) (void)ehist_clear(h);
        return fail(AMC_ERR_STATE, "amc_energy_histogram_accumulate: %lld chains over a grid of %d blocks overflow a block's 32-bit cells", (long long)h->M, grid);
    }
    amc::EhistArgs a = ehist_args(h);
    void* params[] = {&a};
    const int rc = launch_by_potential(h, "amc::energy_histogram_kernel", (const void*)amc::energy_histogram_kernel<amc::POT_DOUBLE_WELL>,
                                       (const void*)amc::energy_histogram_kernel<amc::POT_HARMONIC>, grid, params);
    // a first call that is refused (a run-time build that fails, say) leaves no accumulator and no bins behind
    if (rc != AMC_OK && first) (void)ehist_clear(h);
    return rc;
}

int amc_energy_histogram_accumulate_blocks(amc_handle* h, double lo, double hi, int n_bins)
{
    static const char* who = "amc_energy_histogram_accumulate_blocks";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    if (!hist_args_ok(who, lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    const int B = ehist_partition_blocks(h), G = pass_groups(h);
    const bool by_family = ehist_by_family(h);
    if (!B) return fail(AMC_ERR_STATE, "%s: no partition is set (amc_set_blocks)", who);
    if (by_family && G != 1) return fail(AMC_ERR_STATE, "%s: blocks of families belong to one population at one shared beta, the handle has a ladder", who);
    if ((int64_t)B * G * (n_bins + 3) > AMC_EHIST_BLK_MAX_CELLS)
        return fail(AMC_ERR_BAD_ARG, "%s: %d blocks of %d rows of %d cells are more than AMC_EHIST_BLK_MAX_CELLS = %d cells", who, B, G, n_bins + 3,
                    AMC_EHIST_BLK_MAX_CELLS);
    AMC_TRY(ehist_same(h, who, true, lo, hi, n_bins));
    if (by_family) return ehist_accumulate_families(h, who, lo, hi, n_bins);
    // the blocked form of the u32 check: a HIP block's cell holds at most lane_bound x AMC_BLOCK chains of one pass
    const int grid = amc::blk::grid_round(hist_grid(h), B);
    const int64_t lanes = amc::blk::lane_bound(h->M / G, B, h->blocks.chunk, G, grid, AMC_BLOCK);
    if (lanes >= ((int64_t)1 << 32) / AMC_BLOCK)
        return fail(AMC_ERR_STATE, "%s: %lld chains over a grid of %d blocks overflow a block's 32-bit cells", who, (long long)h->M, grid);
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));
    const bool first = !h->ehist.d_ehist;
    if (first) {
        AMC_HIP(hipStreamSynchronize(h->stream));      // (as the other blocked accumulators wait where they allocate: blocks_words)
        AMC_TRY(ehist_begin(h, lo, hi, n_bins, B));
        if (hipMemsetAsync(h->ehist.d_ehist, 0, ehist_cells(h) * sizeof(unsigned long long), h->stream) != hipSuccess) {
            (void)ehist_clear(h);
            return fail(AMC_ERR_HIP, "%s: clearing the accumulator failed", who);
        }
    }
    amc::EhistArgs a = ehist_args(h);
    amc::blk::Part part = blocks_part(h);
    void* params[] = {&a, &part};
    const int rc = launch_by_potential(h, "amc::energy_histogram_blocks_kernel", (const void*)amc::energy_histogram_blocks_kernel<amc::POT_DOUBLE_WELL>,
                                       (const void*)amc::energy_histogram_blocks_kernel<amc::POT_HARMONIC>, grid, params);
    if (rc != AMC_OK && first) (void)ehist_clear(h);
    return rc;
}

int amc_energy_histogram_fetch(amc_handle* h, uint64_t* counts, int64_t capacity_cells, int* n_groups, int* n_bins, double* lo, double* hi,
                               uint64_t* n_snapshots, int reset)
{
    if (!h || !n_groups || !n_bins || !lo || !hi || !n_snapshots) return fail(AMC_ERR_BAD_ARG, "amc_energy_histogram_fetch: NULL argument");
    if (!h->ehist.d_ehist) {            // nothing accumulated: no counts (the array may be NULL), no bins
        *n_groups = pass_groups(h);
        *n_bins = 0;
        *lo = *hi = 0.0;
        *n_snapshots = 0;
        return AMC_OK;
    }
    const size_t cells = ehist_set_cells(h);
    if (!counts) {                      // the sizes alone, for a caller about to allocate: nothing waits, nothing is copied, nothing is reset
        *n_groups = h->ehist.groups;
        *n_bins = h->ehist.n_bins;
        *lo = h->ehist.lo;
        *hi = h->ehist.hi;
        *n_snapshots = 0;
        return AMC_OK;
    }
    if (capacity_cells < (int64_t)cells)
        return fail(AMC_ERR_BAD_ARG, "amc_energy_histogram_fetch: capacity_cells = %lld, the accumulator has %d rows of %d cells", (long long)capacity_cells,
                    h->ehist.groups, h->ehist.n_bins + 3);
    AMC_HIP(hipSetDevice(h->device));
    if (h->ehist.blocks) {              // a blocked accumulator: the sum over its blocks, formed here behind the copy
        std::vector<uint64_t> all(ehist_cells(h));
        AMC_TRY(copy_to_host_sync(h, all.data(), h->ehist.d_ehist, all.size() * sizeof(uint64_t)));
        for (size_t i = 0; i < cells; ++i) {
            uint64_t s = 0;
            for (int b = 0; b < h->ehist.blocks; ++b) s += all[(size_t)b * cells + i];
            counts[i] = s;
        }
    } else {
        AMC_TRY(copy_to_host_sync(h, counts, h->ehist.d_ehist, cells * sizeof(unsigned long long)));
    }
    uint64_t row0 = 0;
    for (int i = 0; i < h->ehist.n_bins + 3; ++i) row0 += counts[i];
    *n_groups = h->ehist.groups;
    *n_bins = h->ehist.n_bins;
    *lo = h->ehist.lo;
    *hi = h->ehist.hi;
    *n_snapshots = row0 / (uint64_t)(h->M / h->ehist.groups);      // every chain of a group lands in exactly one cell of its row
    if (reset) return ehist_clear(h);
    return AMC_OK;
}

int amc_energy_histogram_fetch_blocks(amc_handle* h, uint64_t* counts, int64_t capacity_cells, int* n_blocks, int* n_groups, int* n_bins, double* lo,
                                      double* hi, uint64_t* n_snapshots, int reset)
{
    static const char* who = "amc_energy_histogram_fetch_blocks";
    if (!h || !n_blocks || !n_groups || !n_bins || !lo || !hi || !n_snapshots) return fail(AMC_ERR_BAD_ARG, "%s: NULL argument", who);
    if (!h->ehist.d_ehist || !h->ehist.blocks)
        return fail(AMC_ERR_STATE, "%s: no accumulator kept per jackknife block stands (amc_energy_histogram_accumulate_blocks)", who);
    const int B = h->ehist.blocks, G = h->ehist.groups;
    *n_blocks = B;
    *n_groups = G;
    *n_bins = h->ehist.n_bins;
    *lo = h->ehist.lo;
    *hi = h->ehist.hi;
    *n_snapshots = 0;
    if (!counts) return AMC_OK;         // the sizes alone: nothing waits, nothing is copied, nothing is reset
    const size_t cells = ehist_cells(h), row = (size_t)h->ehist.n_bins + 3;
    if (capacity_cells < (int64_t)cells)
        return fail(AMC_ERR_BAD_ARG, "%s: capacity_cells = %lld, the accumulator has %d blocks of %d rows of %d cells", who, (long long)capacity_cells, B, G,
                    h->ehist.n_bins + 3);
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(copy_to_host_sync(h, counts, h->ehist.d_ehist, cells * sizeof(unsigned long long)));
    if (h->ehist.by_family) {           // blocks of families change their size at every resampling: every chain lands in exactly one cell
        uint64_t all = 0;
        for (size_t i = 0; i < cells; ++i) all += counts[i];
        *n_snapshots = all / (uint64_t)h->M;
        if (reset) return ehist_clear(h);
        return AMC_OK;
    }
    // a block without a local ladder holds nothing; the snapshots from the first block that has one
    const amc::blk::Part part = blocks_part(h);
    for (int b = 0; b < B; ++b) {
        const uint64_t ladders = (uint64_t)amc::blk::ladders_in_block(part, b, h->M / G);
        if (!ladders) continue;
        uint64_t row0 = 0;
        for (size_t i = 0; i < row; ++i) row0 += counts[(size_t)b * G * row + i];
        *n_snapshots = row0 / ladders;
        break;
    }
    if (reset) return ehist_clear(h);
    return AMC_OK;
}

int amc_set_energy_histogram(amc_handle* h, double lo, double hi, int n_bins, const uint64_t* counts_or_null, uint64_t n_snapshots)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_energy_histogram: NULL handle");
    if (!counts_or_null || n_snapshots == 0) {
        AMC_HIP(hipSetDevice(h->device));
        return ehist_clear(h);
    }
    if (!hist_args_ok("amc_set_energy_histogram", lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    const int G = pass_groups(h);
    const uint64_t per_group = (uint64_t)(h->M / G);
    if (n_snapshots > UINT64_MAX / per_group) return fail(AMC_ERR_BAD_ARG, "amc_set_energy_histogram: n_snapshots * n_chains / G does not fit 64 bits");
    const uint64_t want = n_snapshots * per_group;
    AMC_TRY(ehist_rows_sum("amc_set_energy_histogram", "n_snapshots * n_chains / G", counts_or_null, 1, G, n_bins, &want));
    AMC_HIP(hipSetDevice(h->device));
    if (h->ehist.d_ehist && (h->ehist.blocks || h->ehist.groups != G || h->ehist.n_bins != n_bins)) AMC_TRY(ehist_clear(h));
    if (!h->ehist.d_ehist) AMC_TRY(ehist_begin(h, lo, hi, n_bins));
    h->ehist.lo = lo;
    h->ehist.hi = hi;
    return copy_to_device_sync(h, h->ehist.d_ehist, counts_or_null, ehist_cells(h) * sizeof(unsigned long long));      // the caller's buffer is only valid during the call
}

int amc_set_energy_histogram_blocks(amc_handle* h, double lo, double hi, int n_bins, const uint64_t* counts_or_null, int n_blocks, uint64_t n_snapshots)
{
    static const char* who = "amc_set_energy_histogram_blocks";
    if (!h) return fail(AMC_ERR_BAD_ARG, "%s: NULL handle", who);
    const int B = ehist_partition_blocks(h), G = pass_groups(h);
    const bool by_family = ehist_by_family(h);
    if (!B) return fail(AMC_ERR_STATE, "%s: no partition is set (amc_set_blocks)", who);
    if (by_family && G != 1) return fail(AMC_ERR_STATE, "%s: blocks of families belong to one population at one shared beta, the handle has a ladder", who);
    if (!counts_or_null || n_snapshots == 0) {
        AMC_HIP(hipSetDevice(h->device));
        return ehist_clear(h);
    }
    if (n_blocks != B) return fail(AMC_ERR_BAD_ARG, "%s: n_blocks = %d, the partition has %d blocks", who, n_blocks, B);
    if (!hist_args_ok(who, lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    if ((int64_t)B * G * (n_bins + 3) > AMC_EHIST_BLK_MAX_CELLS)
        return fail(AMC_ERR_BAD_ARG, "%s: %d blocks of %d rows of %d cells are more than AMC_EHIST_BLK_MAX_CELLS = %d cells", who, B, G, n_bins + 3,
                    AMC_EHIST_BLK_MAX_CELLS);
    if (by_family) {                    // a block's share changes with every resampling: all the cells hold every chain once per snapshot
        if (n_snapshots > UINT64_MAX / (uint64_t)h->M) return fail(AMC_ERR_BAD_ARG, "%s: n_snapshots * n_chains does not fit 64 bits", who);
        const uint64_t want = n_snapshots * (uint64_t)h->M;
        uint64_t sum = 0;
        bool over = false;
        for (size_t i = 0; i < (size_t)B * (size_t)(n_bins + 3) && !over; ++i) {
            over = counts_or_null[i] > want - sum;
            if (!over) sum += counts_or_null[i];
        }
        if (over || sum != want) return fail(AMC_ERR_BAD_ARG, "%s: the cells do not sum to n_snapshots * n_chains = %llu", who, (unsigned long long)want);
        AMC_HIP(hipSetDevice(h->device));
        AMC_TRY(ehist_clear(h));
        AMC_TRY(ehist_begin(h, lo, hi, n_bins, B));
        h->ehist.by_family = true;
        return copy_to_device_sync(h, h->ehist.d_ehist, counts_or_null, ehist_cells(h) * sizeof(unsigned long long));
    }
    // every (block, group) row holds the block's ladders once per snapshot; a block without a local ladder holds nothing
    const amc::blk::Part part = blocks_part(h);
    uint64_t want[AMC_MAX_JK_BLOCKS];
    for (int b = 0; b < B; ++b) {
        const uint64_t ladders = (uint64_t)amc::blk::ladders_in_block(part, b, h->M / G);
        if (ladders && n_snapshots > UINT64_MAX / ladders) return fail(AMC_ERR_BAD_ARG, "%s: n_snapshots * (ladders of block %d) does not fit 64 bits", who, b);
        want[b] = n_snapshots * ladders;
    }
    AMC_TRY(ehist_rows_sum(who, "n_snapshots * (local ladders of the block)", counts_or_null, B, G, n_bins, want));
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(ehist_clear(h));
    AMC_TRY(ehist_begin(h, lo, hi, n_bins, B));
    return copy_to_device_sync(h, h->ehist.d_ehist, counts_or_null, ehist_cells(h) * sizeof(unsigned long long));      // the caller's buffer is only valid during the call
}

}  // extern "C"
