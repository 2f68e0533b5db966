// amc_chainstats.hip -- convergence per group: one pass per sample into running sums per chain
// (amc_chain_stats_accumulate), their reproducible sums by group (amc_chain_stats_fetch), the checkpoint pair
// (amc_chain_stats_download, amc_set_chain_stats) and amc_chain_stats_clear.  The sums by group are rung passes (RungPass,
// amc_internal.h) with G = 1 where the handle has no ladder, never blocked; their block rows share lad.d_rung_rows with the rung sums,
// the bridge sums and the time correlation.  Everything here is allocated at its first use: a handle that never accumulates has none
// of it and launches what it always did.
#define AMC_KERNEL_LINKAGE static      // template instantiations, and this object's own copies of the plain kernels it launches (chain_stats_sums_kernel, chain_stats_finish_kernel)
#include "amc_internal.h"

static_assert(AMC_CHAIN_STATS_PARTS == amc::CS_PARTS && AMC_CHAIN_STATS_COLS == amc::CS_COLS, "the chain statistics of include/amc.h and amc_chainstats.h");

static const size_t STAT_ROWS_BYTES = (size_t)AMC_MAX_RUNGS * amc::CS_COLS * amc::XS_ROW_R * sizeof(amc::xs_word);      // d_stat_rows

static inline size_t chain_stats_bytes(const amc_handle* h) { return (size_t)amc::CS_PARTS * 2 * (size_t)h->M * sizeof(double); }

static inline bool observable_ok(int observable) { return observable == AMC_CORR_E || observable == AMC_CORR_X; }

extern "C" {

int amc_chain_stats_accumulate(amc_handle* h, int observable, int part)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_chain_stats_accumulate: NULL handle");
    if (!observable_ok(observable))
        return fail(AMC_ERR_BAD_ARG, "amc_chain_stats_accumulate: observable = %d must be AMC_CORR_E or AMC_CORR_X", observable);
    if (part < 0 || part >= AMC_CHAIN_STATS_PARTS) return fail(AMC_ERR_BAD_ARG, "amc_chain_stats_accumulate: part = %d must be 0 or 1", part);
    if (h->cstat.observable && h->cstat.observable != observable)
        return fail(AMC_ERR_STATE, "amc_chain_stats_accumulate: the accumulators hold observable %d (amc_chain_stats_clear frees them for another)",
                    h->cstat.observable);
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of a sample of the time correlation: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    const bool first = !h->cstat.observable;
    if (first) {
        if (!h->cstat.d_sums) AMC_HIP(hipMalloc(&h->cstat.d_sums, chain_stats_bytes(h)));
        AMC_HIP(hipMemsetAsync(h->cstat.d_sums, 0, chain_stats_bytes(h), h->stream));
    }
    amc::ChainStatsArgs a = {};
    a.x = h->d_x;
    a.s = h->cstat.d_sums + (size_t)part * 2 * (size_t)h->M;
    a.q = a.s + h->M;
    a.n_chains = h->M;
    a.observable = observable;
    void* params[] = {&a};
    // (a first call that is refused -- a run-time build that fails, say -- fixes no observable: the handle is as it was)
    AMC_TRY(launch_by_potential(h, "amc::chain_stats_add_kernel", (const void*)amc::chain_stats_add_kernel<amc::POT_DOUBLE_WELL>,
                                (const void*)amc::chain_stats_add_kernel<amc::POT_HARMONIC>, rung_pass_grid(h), params));
    h->cstat.observable = observable;
    h->cstat.n[part] += 1;
    return AMC_OK;
}

int amc_chain_stats_fetch(amc_handle* h, double* records, int capacity_words, uint64_t* n, int* groups, int* observable)
{
    if (!h || !n || !groups || !observable) return fail(AMC_ERR_BAD_ARG, "amc_chain_stats_fetch: NULL argument");
    const int G = pass_groups(h);
    if (!h->cstat.observable || !records) {      // nothing accumulated, or the sizes alone: nothing waits, nothing is copied
        *groups = G;
        *observable = h->cstat.observable;
        n[0] = h->cstat.n[0];
        n[1] = h->cstat.n[1];
        return AMC_OK;
    }
    const size_t n_rows = (size_t)G * amc::CS_COLS;
    if (capacity_words < 0 || (size_t)capacity_words < n_rows * amc::xs::XS_WORDS)
        return fail(AMC_ERR_BAD_ARG, "amc_chain_stats_fetch: capacity_words = %d, %d groups of %d records take %d", capacity_words, G, amc::CS_COLS,
                    (int)(n_rows * amc::xs::XS_WORDS));
    AMC_HIP(hipSetDevice(h->device));
    RungPass p;
    AMC_TRY(rung_pass_plan(h, amc::CS_COLS, false, &p));      // (unpartitioned under a partition too)
    if (!h->cstat.d_stat_rows) AMC_HIP(hipMalloc(&h->cstat.d_stat_rows, STAT_ROWS_BYTES));
    amc::ChainStatsSumsArgs a = {};
    a.sums = h->cstat.d_sums;
    a.n_chains = h->M;
    a.cols = (1 << amc::CS_COLS) - 1;
    AMC_TRY(rung_pass_each(h, p, a, [&](amc::ChainStatsSumsArgs& one) {
        hipLaunchKernelGGL(amc::chain_stats_sums_kernel, dim3(p.grid), dim3(AMC_BLOCK), 0, h->stream, one);
        AMC_HIP(hipGetLastError());
        return (int)AMC_OK;
    }));
    hipLaunchKernelGGL(amc::chain_stats_finish_kernel, dim3((unsigned)n_rows), dim3(64), 0, h->stream, (const amc::xs_word*)h->lad.d_rung_rows, p.n_blocks(),
                       p.groups, h->cstat.d_stat_rows);
    AMC_HIP(hipGetLastError());
    std::vector<amc::xs_word> host(n_rows * amc::XS_ROW_R, 0ull);
    AMC_TRY(copy_to_host_sync(h, host.data(), h->cstat.d_stat_rows, host.size() * sizeof(amc::xs_word)));
    for (size_t s = 0; s < n_rows; ++s) amc::xs::rec_from_r(records + s * amc::xs::XS_WORDS, amc::xs_load_r_row(host.data() + s * amc::XS_ROW_R));
    *groups = G;
    *observable = h->cstat.observable;
    n[0] = h->cstat.n[0];
    n[1] = h->cstat.n[1];
    return AMC_OK;
}

int amc_chain_stats_download(amc_handle* h, double* sums)
{
    if (!h || !sums) return fail(AMC_ERR_BAD_ARG, "amc_chain_stats_download: NULL argument");
    if (!h->cstat.observable) return fail(AMC_ERR_STATE, "amc_chain_stats_download: nothing is accumulated (amc_chain_stats_accumulate)");
    AMC_HIP(hipSetDevice(h->device));
    return copy_to_host_sync(h, sums, h->cstat.d_sums, chain_stats_bytes(h));
}

int amc_set_chain_stats(amc_handle* h, int observable, const uint64_t* n, const double* sums)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_chain_stats: NULL handle");
    if (!sums || !n || (n[0] == 0 && n[1] == 0)) {
        chain_stats_forget(h);
        return AMC_OK;
    }
    if (!observable_ok(observable)) return fail(AMC_ERR_BAD_ARG, "amc_set_chain_stats: observable = %d must be AMC_CORR_E or AMC_CORR_X", observable);
    AMC_HIP(hipSetDevice(h->device));
    if (!h->cstat.d_sums) AMC_HIP(hipMalloc(&h->cstat.d_sums, chain_stats_bytes(h)));
    AMC_TRY(copy_to_device_sync(h, h->cstat.d_sums, sums, chain_stats_bytes(h)));      // the caller's buffer is only valid during the call
    h->cstat.observable = observable;
    h->cstat.n[0] = n[0];
    h->cstat.n[1] = n[1];
    return AMC_OK;
}

int amc_chain_stats_clear(amc_handle* h)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_chain_stats_clear: NULL handle");
    chain_stats_forget(h);
    return AMC_OK;
}

}  // extern "C"
