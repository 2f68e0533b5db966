// amc_anneal.hip -- population annealing: the annealing step (amc_anneal), its record log (amc_anneal_fetch,
// amc_set_anneal_records), the annealing step index, the shared beta (amc_get_beta, amc_set_beta), the choice of the next beta
// (amc_anneal_next_beta) and the families (amc_set_anneal_families .. amc_upload_families) with the partition into blocks of families and its log of block records
// (amc_set_anneal_blocks .. amc_anneal_block_counts).  Everything here is allocated at its first use: a handle that never anneals has none of it.
#define AMC_KERNEL_LINKAGE static      // the template instantiations, and this object's own copies of the plain kernels it launches
#include "amc_internal.h"

static_assert(AMC_ANNEAL_RECORD_WORDS == amc::ANNEAL_R_WORDS, "the record of include/amc.h and amc_anneal.h");
static_assert(AMC_ANNEAL_SEARCH_MAX_ROUNDS == amc::SEARCH_MAX_ROUNDS && AMC_ANNEAL_SEARCH_OK == amc::SEARCH_OK && AMC_ANNEAL_SEARCH_LIMIT == amc::SEARCH_LIMIT &&
                  AMC_ANNEAL_SEARCH_BELOW_RESOLUTION == amc::SEARCH_BELOW_RESOLUTION && AMC_ANNEAL_SEARCH_STALLED == amc::SEARCH_STALLED &&
                  AMC_ANNEAL_SEARCH_ALL_NAN == amc::SEARCH_ALL_NAN && AMC_ANNEAL_SEARCH_INF == amc::SEARCH_INF &&
                  AMC_ANNEAL_SEARCH_NO_WEIGHT == amc::SEARCH_NO_WEIGHT,
              "the search of include/amc.h and amc_anneal_search.h");

static const size_t ANNEAL_LOG_BYTES = (size_t)AMC_ANNEAL_MAX_RECORDS * amc::ANNEAL_R_WORDS * sizeof(unsigned long long);

static_assert(AMC_MAX_JK_BLOCKS == amc::ANNEAL_MAX_BLOCKS, "the blocks of include/amc.h and amc_anneal.h");
static size_t blk_log_bytes(int B) { return (size_t)AMC_ANNEAL_MAX_RECORDS * 2 * (size_t)B * sizeof(unsigned long long); }

static int64_t anneal_tiles(const amc_handle* h) { return (h->M + amc::ANNEAL_TILE - 1) / amc::ANNEAL_TILE; }

// The buffers of the step itself: the second position buffer (padded and zeroed like the first), the word per chain that holds a, W
// and N in turn, the tile sums, the scratch words.
static int anneal_room(amc_handle* h)
{
    if (!h->ann.d_x_alt) {
        AMC_HIP(hipMalloc(&h->ann.d_x_alt, (size_t)h->M_pad * sizeof(double)));
        AMC_HIP(hipMemsetAsync(h->ann.d_x_alt, 0, (size_t)h->M_pad * sizeof(double), h->stream));
    }
    if (!h->ann.d_anneal_n) AMC_HIP(hipMalloc(&h->ann.d_anneal_n, (size_t)h->M * sizeof(unsigned long long)));
    if (!h->ann.d_anneal_tiles) AMC_HIP(hipMalloc(&h->ann.d_anneal_tiles, (size_t)anneal_tiles(h) * sizeof(unsigned long long)));
    if (!h->ann.d_anneal_s) AMC_HIP(hipMalloc(&h->ann.d_anneal_s, amc::ANNEAL_S_WORDS * sizeof(unsigned long long)));
    return zeroed_words(h, &h->ann.d_anneal_log, ANNEAL_LOG_BYTES);
}

// The partition over the families gone, its log with it.  hipFree waits for whatever still writes the memory.
static void anneal_blocks_off(amc_handle* h)
{
    if (h->ehist.by_family) (void)ehist_fold(h);      // energy histograms kept under the partition that goes: folded into a plain one, nothing is lost
    if (h->ann.d_blk_log) (void)hipFree(h->ann.d_blk_log);
    h->ann.d_blk_log = nullptr;
    h->ann.blk_B = h->ann.blk_n = 0;
    h->ann.blk_chunk = 0;
}

// n_b (and T_b, with w) of the chains as they stand into rec[2 B], zeroed in front on the stream.
static int anneal_block_sums(amc_handle* h, const unsigned long long* w, unsigned long long* rec)
{
    const int B = h->ann.blk_B;
    const uint32_t chunk = (uint32_t)std::min<int64_t>(h->ann.blk_chunk, 0xFFFFFFFFll);      // (an id is below 2^32 - 1: the quotient is 0 either way)
    AMC_HIP(hipMemsetAsync(rec, 0, 2 * (size_t)B * sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(amc::anneal_block_sums_kernel, dim3(grid_for(h, (h->M + amc::ANNEAL_ITEMS - 1) / amc::ANNEAL_ITEMS)), dim3(AMC_BLOCK), 0, h->stream, w,
                       (const uint32_t*)h->ann.d_fam, h->M, (const unsigned long long*)h->ann.d_anneal_s, chunk, B, rec);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

static int families_off(amc_handle* h)
{
    if (!h->ann.d_fam) return AMC_OK;
    AMC_HIP(hipStreamSynchronize(h->stream));      // launches queued on the stream may still use them
    anneal_blocks_off(h);                          // the partition is a function of the family ids
    (void)hipFree(h->ann.d_fam);
    (void)hipFree(h->ann.d_fam_alt);
    (void)hipFree(h->ann.d_fam_cnt);
    h->ann.d_fam = h->ann.d_fam_alt = nullptr;
    h->ann.d_fam_cnt = nullptr;
    return AMC_OK;
}

extern "C" {

int amc_anneal(amc_handle* h, double beta_new)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_anneal: NULL handle");
    if (h->beta_arr) return fail(AMC_ERR_STATE, "amc_anneal: the handle has a per-chain beta array; population annealing cools one shared beta");
    if (h->lad.n_rungs) return fail(AMC_ERR_STATE, "amc_anneal: the handle has a ladder (amc_set_ladder)");
    if (h->blocks.n_blocks)
        return fail(AMC_ERR_STATE, "amc_anneal: a partition is set (amc_set_blocks); resampling makes copies of one parent share blocks, which are then not independent");
    if (h->offset != 0 || h->M != h->M_global)
        return fail(AMC_ERR_STATE, "amc_anneal: the handle holds chains [%lld, %lld) of %lld; resampling needs the whole ensemble on one handle",
                    (long long)h->offset, (long long)(h->offset + h->M), (long long)h->M_global);
    if (!std::isfinite(beta_new)) return fail(AMC_ERR_BAD_ARG, "amc_anneal: beta_new = %g is not finite", beta_new);
    if (h->M >> 33) return fail(AMC_ERR_BAD_ARG, "amc_anneal: n_chains = %lld, the total weight needs n_chains < 2^33", (long long)h->M);
    if (h->ann.anneal_n >= AMC_ANNEAL_MAX_RECORDS)
        return fail(AMC_ERR_STATE, "amc_anneal: the record log is full (%d records; amc_anneal_fetch with reset empties it)", AMC_ANNEAL_MAX_RECORDS);
    if (h->ann.t_a >> 48) return fail(AMC_ERR_STATE, "amc_anneal: the annealing step index has reached 2^48");
    if (h->ann.blk_B && h->ann.blk_n >= AMC_ANNEAL_MAX_RECORDS)
        return fail(AMC_ERR_STATE, "amc_anneal: the log of block records is full (%d records; amc_anneal_fetch_blocks with reset empties it)", AMC_ANNEAL_MAX_RECORDS);
    AMC_HIP(hipSetDevice(h->device));
    // (what an exchange step does before it launches: a learning step left pending by a fused time step is taken now; reductions in
    // flight were queued on the same stream and have read x before the buffers change places)
    AMC_TRY(pg_resolve(h));
    AMC_TRY(anneal_room(h));
    if (h->ann.blk_B) AMC_TRY(zeroed_words(h, &h->ann.d_blk_log, blk_log_bytes(h->ann.blk_B)));
    const int64_t n_tiles = anneal_tiles(h);
    const int grid_chains = grid_for(h, h->M), grid_tiles = grid_for(h, n_tiles * AMC_BLOCK);
    unsigned long long* rec = h->ann.d_anneal_log + (size_t)h->ann.anneal_n * amc::ANNEAL_R_WORDS;
    AMC_HIP(hipMemsetAsync(h->ann.d_anneal_s, 0, amc::ANNEAL_S_WORDS * sizeof(unsigned long long), h->stream));
    {
        amc::AnnealLogwArgs a;
        a.x = h->d_x;
        a.a = h->ann.d_anneal_n;
        a.scratch = h->ann.d_anneal_s;
        a.n_chains = h->M;
        a.delta = h->f32 ? (double)((float)beta_new - (float)h->beta) : beta_new - h->beta;
        void* params[] = {&a};
        AMC_TRY(launch_by_potential(h, "amc::anneal_logw_kernel", (const void*)amc::anneal_logw_kernel<amc::POT_DOUBLE_WELL>,
                                    (const void*)amc::anneal_logw_kernel<amc::POT_HARMONIC>, grid_chains, params));
    }
    hipLaunchKernelGGL(amc::anneal_weights_kernel, dim3(grid_tiles), dim3(AMC_BLOCK), 0, h->stream, h->ann.d_anneal_n, h->M, n_tiles,
                       (const unsigned long long*)h->ann.d_anneal_s, h->ann.d_anneal_tiles);
    AMC_HIP(hipGetLastError());
    // blocks of families: the step's block record, from W -- behind the weights, in front of the prefix pass that overwrites them
    if (h->ann.blk_B) AMC_TRY(anneal_block_sums(h, h->ann.d_anneal_n, h->ann.d_blk_log + (size_t)h->ann.blk_n * 2 * h->ann.blk_B));
    {
        amc::AnnealTotalArgs a;
        a.tile_sums = h->ann.d_anneal_tiles;
        a.scratch = h->ann.d_anneal_s;
        a.rec = rec;
        a.n_tiles = n_tiles;
        a.t_a = h->ann.t_a;
        std::memcpy(&a.beta_from, &h->beta, sizeof(double));
        std::memcpy(&a.beta_to, &beta_new, sizeof(double));
        a.key0 = (uint32_t)h->seed;
        a.key1 = (uint32_t)(h->seed >> 32);
        hipLaunchKernelGGL(amc::anneal_total_kernel, dim3(1), dim3(AMC_BLOCK), 0, h->stream, a);
        AMC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(amc::anneal_prefix_kernel, dim3(grid_tiles), dim3(AMC_BLOCK), 0, h->stream, h->ann.d_anneal_n, h->M, n_tiles,
                       (const unsigned long long*)h->ann.d_anneal_s, (const unsigned long long*)h->ann.d_anneal_tiles, rec);
    AMC_HIP(hipGetLastError());
    hipLaunchKernelGGL(amc::anneal_gather_kernel, dim3(grid_chains), dim3(AMC_BLOCK), 0, h->stream, (const void*)h->d_x, (void*)h->ann.d_x_alt, h->f32 ? 1 : 0,
                       (const uint32_t*)h->ann.d_fam, h->ann.d_fam_alt, (const unsigned long long*)h->ann.d_anneal_n, h->M, (const unsigned long long*)h->ann.d_anneal_s);
    AMC_HIP(hipGetLastError());
    std::swap(h->d_x, h->ann.d_x_alt);
    if (h->ann.d_fam) std::swap(h->ann.d_fam, h->ann.d_fam_alt);
    h->beta = beta_new;          // the host field: in force for every launch queued from now on (nothing on the device is derived from it)
    h->ann.t_a += 1;
    h->ann.anneal_n += 1;
    if (h->ann.blk_B) h->ann.blk_n += 1;
    corr_forget(h);              // the copies have changed slots: the mark of the time correlation goes (include/amc.h "Time correlation")
    return AMC_OK;
}

// Choosing the next beta (DESIGN.md section 3.14 "Choosing the next beta"; the kernels are amc_anneal_search.h's).
int amc_anneal_next_beta(amc_handle* h, double beta_limit, double target, int rounds, double* beta_new, uint64_t* diag, uint64_t* trace)
{
    if (!h || !beta_new) return fail(AMC_ERR_BAD_ARG, "amc_anneal_next_beta: NULL argument");
    if (h->beta_arr)
        return fail(AMC_ERR_STATE, "amc_anneal_next_beta: the handle has a per-chain beta array; population annealing cools one shared beta");
    if (h->lad.n_rungs) return fail(AMC_ERR_STATE, "amc_anneal_next_beta: the handle has a ladder (amc_set_ladder)");
    if (h->offset != 0 || h->M != h->M_global)
        return fail(AMC_ERR_STATE, "amc_anneal_next_beta: the handle holds chains [%lld, %lld) of %lld; the weights need the whole ensemble on one handle",
                    (long long)h->offset, (long long)(h->offset + h->M), (long long)h->M_global);
    if (!std::isfinite(beta_limit)) return fail(AMC_ERR_BAD_ARG, "amc_anneal_next_beta: beta_limit = %g is not finite", beta_limit);
    if (!(target > 0.0 && target < 1.0)) return fail(AMC_ERR_BAD_ARG, "amc_anneal_next_beta: target = %g must lie strictly between 0 and 1", target);
    if (rounds < 1 || rounds > AMC_ANNEAL_SEARCH_MAX_ROUNDS)
        return fail(AMC_ERR_BAD_ARG, "amc_anneal_next_beta: rounds = %d must lie in [1, %d]", rounds, AMC_ANNEAL_SEARCH_MAX_ROUNDS);
    if (h->M >> 33) return fail(AMC_ERR_BAD_ARG, "amc_anneal_next_beta: n_chains = %lld, the sums need n_chains < 2^33", (long long)h->M);
    const double span = h->f32 ? (double)((float)beta_limit - (float)h->beta) : beta_limit - h->beta;
    if (!std::isfinite(span)) return fail(AMC_ERR_BAD_ARG, "amc_anneal_next_beta: the span from beta = %g to beta_limit = %g is not finite", h->beta, beta_limit);
    const size_t n_trace = (size_t)rounds * amc::SEARCH_SUMS;
    if (span == 0.0) {                                         // nothing to search and nothing launched
        *beta_new = beta_limit;
        if (diag) {
            std::memset(diag, 0, AMC_ANNEAL_SEARCH_WORDS * sizeof(uint64_t));
            diag[0] = AMC_ANNEAL_SEARCH_LIMIT;
        }
        if (trace) std::memset(trace, 0, n_trace * sizeof(uint64_t));
        return AMC_OK;
    }
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));                                    // (as amc_anneal: a learning step left pending is taken now)
    if (!h->ann.d_anneal_n) AMC_HIP(hipMalloc(&h->ann.d_anneal_n, (size_t)h->M * sizeof(unsigned long long)));
    if (!h->ann.d_anneal_search) AMC_HIP(hipMalloc(&h->ann.d_anneal_search, amc::SEARCH_S_WORDS * sizeof(unsigned long long)));
    unsigned long long* s = h->ann.d_anneal_search;
    AMC_HIP(hipMemsetAsync(s, 0, amc::SEARCH_S_WORDS * sizeof(unsigned long long), h->stream));      // the keys, the bracket, every round's sums
    const int grid = grid_for(h, h->M);
    {
        amc::AnnealEnergyArgs a;
        a.x = h->d_x;
        a.ne = h->ann.d_anneal_n;
        a.scratch = s;
        a.n_chains = h->M;
        a.span = span;
        void* params[] = {&a};
        AMC_TRY(launch_by_potential(h, "amc::anneal_energy_kernel", (const void*)amc::anneal_energy_kernel<amc::POT_DOUBLE_WELL>,
                                    (const void*)amc::anneal_energy_kernel<amc::POT_HARMONIC>, grid, params));
    }
    amc::AnnealDecideArgs d;
    d.scratch = s;
    d.n_chains = h->M;
    d.rounds = rounds;
    d.f32 = h->f32 ? 1 : 0;
    d.span = span;
    d.beta = h->beta;
    d.beta_limit = beta_limit;
    d.target = target;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(amc::anneal_search_sums_kernel, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, (const unsigned long long*)h->ann.d_anneal_n, h->M,
                           d.f32, r, s);
        AMC_HIP(hipGetLastError());
        d.round = r;
        hipLaunchKernelGGL(amc::anneal_search_decide_kernel, dim3(1), dim3(64), 0, h->stream, d);
        AMC_HIP(hipGetLastError());
    }
    // the one synchronisation: beta is a host field (it goes into the sweeps' launch arguments), so the host must know the answer
    unsigned long long host[amc::SEARCH_S_WORDS];
    AMC_TRY(copy_to_host_sync(h, host, s, (amc::SEARCH_S_HEAD + n_trace) * sizeof(unsigned long long)));
    std::memcpy(beta_new, &host[amc::SEARCH_S_BETA], sizeof(double));
    if (diag) {
        static const int words[AMC_ANNEAL_SEARCH_WORDS] = {amc::SEARCH_S_STATUS, amc::SEARCH_S_ROUNDS, amc::SEARCH_S_STEP,  amc::SEARCH_S_RHO_LO,
                                                            amc::SEARCH_S_HI,     amc::SEARCH_S_RHO_HI, amc::SEARCH_S_NE_HI, amc::SEARCH_S_NE_LO};
        for (int i = 0; i < AMC_ANNEAL_SEARCH_WORDS; ++i) diag[i] = (uint64_t)host[words[i]];
    }
    if (trace)
        for (size_t i = 0; i < n_trace; ++i) trace[i] = (uint64_t)host[amc::SEARCH_S_HEAD + i];
    return AMC_OK;
}

int amc_anneal_fetch(amc_handle* h, uint64_t* records, int capacity, int* n, int reset)
{
    if (!h || !n) return fail(AMC_ERR_BAD_ARG, "amc_anneal_fetch: NULL argument");
    *n = h->ann.anneal_n;
    if (!records) {              // the count alone
        if (reset) h->ann.anneal_n = 0;
        return AMC_OK;
    }
    if (capacity < h->ann.anneal_n)
        return fail(AMC_ERR_BAD_ARG, "amc_anneal_fetch: capacity = %d, the log holds %d records", capacity, h->ann.anneal_n);
    AMC_HIP(hipSetDevice(h->device));
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "records are copied as they are");
    // (an empty log copies nothing and still waits)
    AMC_TRY(copy_to_host_sync(h, records, h->ann.anneal_n ? h->ann.d_anneal_log : nullptr, (size_t)h->ann.anneal_n * amc::ANNEAL_R_WORDS * sizeof(uint64_t)));
    if (reset) h->ann.anneal_n = 0;
    return AMC_OK;
}

int amc_set_anneal_records(amc_handle* h, const uint64_t* records, int n)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_records: NULL handle");
    if (n < 0 || n > AMC_ANNEAL_MAX_RECORDS) return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_records: n = %d must lie in [0, %d]", n, AMC_ANNEAL_MAX_RECORDS);
    if (!records || n == 0) {
        h->ann.anneal_n = 0;
        return AMC_OK;
    }
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(zeroed_words(h, &h->ann.d_anneal_log, ANNEAL_LOG_BYTES));
    AMC_TRY(copy_to_device_sync(h, h->ann.d_anneal_log, records, (size_t)n * amc::ANNEAL_R_WORDS * sizeof(uint64_t)));      // `records` is only valid during the call
    h->ann.anneal_n = n;
    return AMC_OK;
}

int amc_get_anneal_step(amc_handle* h, uint64_t* t)
{
    if (!h || !t) return fail(AMC_ERR_BAD_ARG, "amc_get_anneal_step: NULL argument");
    *t = h->ann.t_a;
    return AMC_OK;
}

int amc_set_anneal_step(amc_handle* h, uint64_t t)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_step: NULL handle");
    if (t >> 48) return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_step: step index must fit 48 bits");
    h->ann.t_a = t;
    return AMC_OK;
}

int amc_get_beta(amc_handle* h, double* beta)
{
    if (!h || !beta) return fail(AMC_ERR_BAD_ARG, "amc_get_beta: NULL argument");
    *beta = h->beta;
    return AMC_OK;
}

int amc_set_beta(amc_handle* h, double beta)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_beta: NULL handle");
    if (!std::isfinite(beta)) return fail(AMC_ERR_BAD_ARG, "amc_set_beta: beta = %g is not finite", beta);
    h->beta = beta;              // (as amc_anneal leaves it: the launches queued from now on read the host field)
    return AMC_OK;
}

// ---- families (DESIGN.md section 3.14 "Families") ------------------------------------------------------------------------------------
int amc_set_anneal_families(amc_handle* h, int on)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_families: NULL handle");
    AMC_HIP(hipSetDevice(h->device));
    if (!on) return families_off(h);
    if (h->M > 0xFFFFFFFFll) return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_families: n_chains = %lld, a family id holds 32 bits", (long long)h->M);
    anneal_blocks_off(h);          // families afresh: block records of the ones that go say nothing about them
    if (!h->ann.d_fam) {
        AMC_HIP(hipMalloc(&h->ann.d_fam, (size_t)h->M * sizeof(uint32_t)));
        const hipError_t e = hipMalloc(&h->ann.d_fam_alt, (size_t)h->M * sizeof(uint32_t));
        if (e != hipSuccess) {
            (void)hipFree(h->ann.d_fam);
            h->ann.d_fam = h->ann.d_fam_alt = nullptr;
            return fail(e == hipErrorOutOfMemory ? AMC_ERR_OOM : AMC_ERR_HIP, "amc_set_anneal_families: %s", hipGetErrorString(e));
        }
    }
    hipLaunchKernelGGL(amc::family_iota_kernel, dim3(grid_for(h, h->M)), dim3(AMC_BLOCK), 0, h->stream, h->ann.d_fam, h->M);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

int amc_anneal_family_stats(amc_handle* h, uint64_t* n_families, uint64_t* sum_sq, uint64_t* largest)
{
    if (!h || !n_families || !sum_sq || !largest) return fail(AMC_ERR_BAD_ARG, "amc_anneal_family_stats: NULL argument");
    AMC_TRY(need_families(h, "amc_anneal_family_stats"));
    AMC_HIP(hipSetDevice(h->device));
    // the scratch: a count per family id, then the three results (allocated at the first call, zeroed per call)
    const size_t cnt_bytes = (size_t)h->M * sizeof(unsigned int), bytes = cnt_bytes + (8 - cnt_bytes % 8) % 8 + 3 * sizeof(unsigned long long);
    if (!h->ann.d_fam_cnt) AMC_HIP(hipMalloc(&h->ann.d_fam_cnt, bytes));
    unsigned long long* d_out = (unsigned long long*)((char*)h->ann.d_fam_cnt + (bytes - 3 * sizeof(unsigned long long)));
    AMC_HIP(hipMemsetAsync(h->ann.d_fam_cnt, 0, bytes, h->stream));
    const int grid = grid_for(h, h->M);
    hipLaunchKernelGGL(amc::family_count_kernel, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, (const uint32_t*)h->ann.d_fam, h->M, h->ann.d_fam_cnt);
    AMC_HIP(hipGetLastError());
    hipLaunchKernelGGL(amc::family_stats_kernel, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, (const unsigned int*)h->ann.d_fam_cnt, h->M, d_out);
    AMC_HIP(hipGetLastError());
    unsigned long long host[3];
    AMC_TRY(copy_to_host_sync(h, host, d_out, sizeof host));
    *n_families = (uint64_t)host[0];
    *sum_sq = (uint64_t)host[1];
    *largest = (uint64_t)host[2];
    return AMC_OK;
}

// ---- blocks of families (DESIGN.md section 3.14 "Error bars") --------------------------------------------------------------------------
int amc_set_anneal_blocks(amc_handle* h, int n_blocks, int64_t chunk)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_blocks: NULL handle");
    if (n_blocks != 0 && (n_blocks < 2 || n_blocks > AMC_MAX_JK_BLOCKS))
        return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_blocks: n_blocks = %d must be 0 (no partition) or lie in [2, %d]", n_blocks, AMC_MAX_JK_BLOCKS);
    if (chunk < 0 || chunk > AMC_MAX_JK_CHUNK)
        return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_blocks: chunk = %lld must lie in [1, 2^40], or be 0 for the default", (long long)chunk);
    if (n_blocks) {
        AMC_TRY(need_families(h, "amc_set_anneal_blocks"));
        if (h->blocks.n_blocks)
            return fail(AMC_ERR_STATE, "amc_set_anneal_blocks: a partition over the ladders is set (amc_set_blocks); the two exclude each other");
    }
    AMC_HIP(hipSetDevice(h->device));
    anneal_blocks_off(h);          // records kept under another partition (or under none) are not sums of these blocks
    if (n_blocks) {
        h->ann.blk_B = n_blocks;
        h->ann.blk_chunk = chunk ? chunk : (h->M + n_blocks - 1) / n_blocks;      // every block one contiguous range of ancestors
    }
    return AMC_OK;
}

int amc_anneal_fetch_blocks(amc_handle* h, uint64_t* records, int capacity, int* n, int* n_blocks, int reset)
{
    if (!h || !n || !n_blocks) return fail(AMC_ERR_BAD_ARG, "amc_anneal_fetch_blocks: NULL argument");
    if (!h->ann.blk_B) return fail(AMC_ERR_STATE, "amc_anneal_fetch_blocks: no partition over the families is set (amc_set_anneal_blocks)");
    *n = h->ann.blk_n;
    *n_blocks = h->ann.blk_B;
    if (!records) return AMC_OK;         // the sizes alone: nothing waits, nothing is copied, nothing is reset
    if (capacity < h->ann.blk_n)
        return fail(AMC_ERR_BAD_ARG, "amc_anneal_fetch_blocks: capacity = %d, the log holds %d block records", capacity, h->ann.blk_n);
    AMC_HIP(hipSetDevice(h->device));
    // (an empty log copies nothing and still waits)
    AMC_TRY(copy_to_host_sync(h, records, h->ann.blk_n ? h->ann.d_blk_log : nullptr, (size_t)h->ann.blk_n * 2 * h->ann.blk_B * sizeof(uint64_t)));
    if (reset) h->ann.blk_n = 0;
    return AMC_OK;
}

int amc_set_anneal_block_records(amc_handle* h, const uint64_t* records, int n, int n_blocks)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_block_records: NULL handle");
    if (!h->ann.blk_B) return fail(AMC_ERR_STATE, "amc_set_anneal_block_records: no partition over the families is set (amc_set_anneal_blocks)");
    if (n < 0 || n > AMC_ANNEAL_MAX_RECORDS)
        return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_block_records: n = %d must lie in [0, %d]", n, AMC_ANNEAL_MAX_RECORDS);
    if (!records || n == 0) {
        h->ann.blk_n = 0;
        return AMC_OK;
    }
    if (n_blocks != h->ann.blk_B)
        return fail(AMC_ERR_BAD_ARG, "amc_set_anneal_block_records: n_blocks = %d, the partition has %d blocks", n_blocks, h->ann.blk_B);
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(zeroed_words(h, &h->ann.d_blk_log, blk_log_bytes(h->ann.blk_B)));
    AMC_TRY(copy_to_device_sync(h, h->ann.d_blk_log, records, (size_t)n * 2 * h->ann.blk_B * sizeof(uint64_t)));      // `records` is only valid during the call
    h->ann.blk_n = n;
    return AMC_OK;
}

int amc_anneal_block_counts(amc_handle* h, uint64_t* counts)
{
    if (!h || !counts) return fail(AMC_ERR_BAD_ARG, "amc_anneal_block_counts: NULL argument");
    if (!h->ann.blk_B) return fail(AMC_ERR_STATE, "amc_anneal_block_counts: no partition over the families is set (amc_set_anneal_blocks)");
    AMC_HIP(hipSetDevice(h->device));
    if (!h->ann.d_blk_now) AMC_HIP(hipMalloc(&h->ann.d_blk_now, 2 * AMC_MAX_JK_BLOCKS * sizeof(unsigned long long)));
    AMC_TRY(anneal_block_sums(h, nullptr, h->ann.d_blk_now));
    return copy_to_host_sync(h, counts, h->ann.d_blk_now, (size_t)h->ann.blk_B * sizeof(uint64_t));
}

int amc_download_families(amc_handle* h, uint32_t* families)
{
    if (!h || !families) return fail(AMC_ERR_BAD_ARG, "amc_download_families: NULL argument");
    AMC_TRY(need_families(h, "amc_download_families"));
    AMC_HIP(hipSetDevice(h->device));
    return copy_to_host_sync(h, families, h->ann.d_fam, (size_t)h->M * sizeof(uint32_t));
}

int amc_upload_families(amc_handle* h, const uint32_t* families)
{
    if (!h || !families) return fail(AMC_ERR_BAD_ARG, "amc_upload_families: NULL argument");
    AMC_TRY(need_families(h, "amc_upload_families"));
    for (int64_t c = 0; c < h->M; ++c)
        if ((int64_t)families[c] >= h->M)
            return fail(AMC_ERR_BAD_ARG, "amc_upload_families: chain %lld: family id %u >= n_chains = %lld", (long long)c, families[c], (long long)h->M);
    AMC_HIP(hipSetDevice(h->device));
    return copy_to_device_sync(h, h->ann.d_fam, families, (size_t)h->M * sizeof(uint32_t));      // `families` is only valid during the call
}

}  // extern "C"
