// amc_ehist.hip -- energy histograms per group: one pass per snapshot into a device-resident accumulator of
// 64-bit counts (amc_energy_histogram_accumulate), its fetch (amc_energy_histogram_fetch) and the checkpoint entry
// (amc_set_energy_histogram).  The groups are those of the time correlation: the rungs of the ladder, ONE group without a ladder.
// The accumulator is allocated at its first use: a handle that never accumulates has none and launches what it always did.
#define AMC_KERNEL_LINKAGE static      // template instantiations, and this object's own copy of the plain kernel it launches (ehist_respaced_kernel)
#include "amc_internal.h"

static inline size_t ehist_cells(const amc_handle* h) { return (size_t)h->ehist.groups * (size_t)(h->ehist.n_bins + 3); }

// The accumulator gone, no bins fixed.  hipFree waits for whatever still writes the memory.
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
    const int cells = (int)ehist_cells(h);
    hipLaunchKernelGGL(amc::ehist_respaced_kernel, dim3(grid_for(h, cells)), dim3(AMC_BLOCK), 0, h->stream, h->ehist.d_ehist, cells,
                       (const unsigned long long*)h->lad.d_respace);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

// Room for G rows of n_bins + 3 cells under the bins (lo, hi, n_bins); the caller fills or zeroes it.
static int ehist_begin(amc_handle* h, double lo, double hi, int n_bins)
{
    const int G = pass_groups(h);
    unsigned long long* d = nullptr;
    AMC_HIP(hipMalloc(&d, (size_t)G * (size_t)(n_bins + 3) * sizeof(unsigned long long)));
    h->ehist.d_ehist = d;
    h->ehist.groups = G;
    h->ehist.n_bins = n_bins;
    h->ehist.lo = lo;
    h->ehist.hi = hi;
    return AMC_OK;
}

extern "C" {

int amc_energy_histogram_accumulate(amc_handle* h, double lo, double hi, int n_bins)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_energy_histogram_accumulate: NULL handle");
    if (!hist_args_ok("amc_energy_histogram_accumulate", lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    if (h->ehist.d_ehist && (n_bins != h->ehist.n_bins || lo != h->ehist.lo || hi != h->ehist.hi))
        return fail(AMC_ERR_STATE, "amc_energy_histogram_accumulate: the accumulator has other bins: [%g, %g) in %d (amc_energy_histogram_fetch with reset frees them)",
                    h->ehist.lo, h->ehist.hi, h->ehist.n_bins);
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
    amc::EhistArgs a = {};
    a.x = h->d_x;
    a.counts = h->ehist.d_ehist;
    a.n_chains = h->M;
    a.lo = lo;
    a.hi = hi;
    a.inv_w = (double)n_bins / (hi - lo);
    a.n_groups = h->ehist.groups;
    a.n_bins = n_bins;
    void* params[] = {&a};
    const int rc = launch_by_potential(h, "amc::energy_histogram_kernel", (const void*)amc::energy_histogram_kernel<amc::POT_DOUBLE_WELL>,
                                       (const void*)amc::energy_histogram_kernel<amc::POT_HARMONIC>, grid, params);
    // a first call that is refused (a run-time build that fails, say) leaves no accumulator and no bins behind
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
    const size_t cells = ehist_cells(h);
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
    AMC_TRY(copy_to_host_sync(h, counts, h->ehist.d_ehist, cells * sizeof(unsigned long long)));
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
    for (int g = 0; g < G; ++g) {
        // (a sum that wraps cannot pass: every partial sum is held to `want`)
        uint64_t sum = 0;
        bool over = false;
        for (int i = 0; i < n_bins + 3; ++i) {
            const uint64_t c = counts_or_null[(size_t)g * (n_bins + 3) + i];
            over = over || c > want - sum;
            if (over) break;
            sum += c;
        }
        if (over || sum != want)
            return fail(AMC_ERR_BAD_ARG, "amc_set_energy_histogram: row %d does not sum to n_snapshots * n_chains / G = %llu", g, (unsigned long long)want);
    }
    AMC_HIP(hipSetDevice(h->device));
    if (h->ehist.d_ehist && (h->ehist.groups != G || h->ehist.n_bins != n_bins)) AMC_TRY(ehist_clear(h));
    if (!h->ehist.d_ehist) AMC_TRY(ehist_begin(h, lo, hi, n_bins));
    h->ehist.lo = lo;
    h->ehist.hi = hi;
    return copy_to_device_sync(h, h->ehist.d_ehist, counts_or_null, ehist_cells(h) * sizeof(unsigned long long));      // the caller's buffer is only valid during the call
}

}  // extern "C"
