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

static inline int corr_groups(const amc_handle* h) { return h->lad.n_rungs ? h->lad.n_rungs : 1; }
// words of one sample's rows
static inline size_t corr_sample_words(int groups) { return (size_t)groups * amc::CORR_COLS * amc::XS_ROW_R; }

static int corr_room(amc_handle* h)
{
    if (!h->corr.d_origin) {
        AMC_HIP(hipMalloc(&h->corr.d_origin, (size_t)h->M_pad * sizeof(double)));
        AMC_HIP(hipMemsetAsync(h->corr.d_origin, 0, (size_t)h->M_pad * sizeof(double), h->stream));
    }
    return zeroed_words(h, &h->corr.d_corr, CORR_BYTES);
}

// One pass into slot `slot`: the sums of the sample, and with `mark` the origin values too.
static int corr_pass(amc_handle* h, int observable, int slot, bool mark)
{
    AMC_HIP(hipSetDevice(h->device));
    // (as in front of a bridge snapshot: a learning step left pending belongs in front of this point of the stream)
    AMC_TRY(pg_resolve(h));
    RungPass p;
    AMC_TRY(rung_pass_plan(h, amc::CORR_COLS, &p));
    AMC_TRY(corr_room(h));
    amc::CorrArgs a = {};
    a.origin = h->corr.d_origin;
    a.mark = mark ? 1 : 0;
    AMC_TRY(rung_pass_launch(h, p, a, observable, "amc::corr_sums_kernel", (const void*)amc::corr_sums_kernel<amc::POT_DOUBLE_WELL>,
                             (const void*)amc::corr_sums_kernel<amc::POT_HARMONIC>));
    hipLaunchKernelGGL(amc::corr_finish_kernel, dim3(p.groups * amc::CORR_COLS), dim3(64), 0, h->stream, (const amc::xs_word*)h->lad.d_rung_rows, p.n_blocks(),
                       p.groups, h->corr.d_corr + (size_t)slot * corr_sample_words(p.groups));
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

extern "C" {

int amc_corr_mark(amc_handle* h, int observable)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_corr_mark: NULL handle");
    if (observable != AMC_CORR_E && observable != AMC_CORR_X)
        return fail(AMC_ERR_BAD_ARG, "amc_corr_mark: observable = %d must be AMC_CORR_E or AMC_CORR_X", observable);
    AMC_TRY(corr_pass(h, observable, 0, true));
    h->corr.observable = observable;
    h->corr.groups = corr_groups(h);
    h->corr.n_samples = 1;
    h->corr.steps[0] = h->t;
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
    std::vector<amc::xs_word> host(n_rows * amc::XS_ROW_R + 1, 0ull);
    AMC_TRY(copy_to_host_sync(h, host.data(), n ? h->corr.d_corr : nullptr, n_rows * amc::XS_ROW_R * sizeof(amc::xs_word)));
    for (size_t s = 0; s < n_rows; ++s) amc::xs::rec_from_r(records + s * amc::xs::XS_WORDS, amc::xs_load_r_row(host.data() + s * amc::XS_ROW_R));
    for (int s = 0; s < n; ++s) steps[s] = h->corr.steps[s];
    *n_samples = n;
    *observable = h->corr.observable;
    return AMC_OK;
}

int amc_corr_download_origin(amc_handle* h, double* origin)
{
    if (!h || !origin) return fail(AMC_ERR_BAD_ARG, "amc_corr_download_origin: NULL argument");
    if (!h->corr.observable) return fail(AMC_ERR_STATE, "amc_corr_download_origin: nothing is marked (amc_corr_mark)");
    AMC_HIP(hipSetDevice(h->device));
    return copy_to_host_sync(h, origin, h->corr.d_origin, (size_t)h->M * sizeof(double));
}

int amc_set_corr(amc_handle* h, int observable, const double* origin, const double* records, const uint64_t* steps, int n_samples)
{
    if (!h || !origin || !records || !steps) return fail(AMC_ERR_BAD_ARG, "amc_set_corr: NULL argument");
    if (observable != AMC_CORR_E && observable != AMC_CORR_X)
        return fail(AMC_ERR_BAD_ARG, "amc_set_corr: observable = %d must be AMC_CORR_E or AMC_CORR_X", observable);
    if (n_samples < 1 || n_samples > AMC_CORR_MAX_LAGS)
        return fail(AMC_ERR_BAD_ARG, "amc_set_corr: n_samples = %d must lie in [1, %d]", n_samples, AMC_CORR_MAX_LAGS);
    for (int s = 0; s < n_samples; ++s) {
        if (steps[s] >> 48) return fail(AMC_ERR_BAD_ARG, "amc_set_corr: steps[%d] must fit 48 bits", s);
        if (s && steps[s] < steps[s - 1]) return fail(AMC_ERR_BAD_ARG, "amc_set_corr: steps[%d] = %llu lies before steps[%d]", s, (unsigned long long)steps[s], s - 1);
    }
    // every (sample, group, column) had a summand: each record is a kind-R record, as amc_corr_fetch gave it
    const int G = corr_groups(h);
    const size_t n_rows = (size_t)n_samples * G * amc::CORR_COLS;
    std::vector<amc::xs_word> host(n_rows * amc::XS_ROW_R, 0ull);
    for (size_t s = 0; s < n_rows; ++s) {
        const double* rec = records + s * amc::xs::XS_WORDS;
        const int slot = (int)(s / ((size_t)G * amc::CORR_COLS)), g = (int)(s / amc::CORR_COLS % G), c = (int)(s % amc::CORR_COLS);
        if (rec[0] != (double)amc::xs::XS_R || !(rec[1] >= amc::xs::XS_LMIN && rec[1] <= amc::xs::XS_LMAX) || rec[1] != std::floor(rec[1]) ||
            !(rec[2] >= 0.0 && rec[2] <= 7.0) || rec[2] != std::floor(rec[2]))
            return fail(AMC_ERR_BAD_ARG, "amc_set_corr: record of sample %d, group %d, column %d is no kind-R record", slot, g, c);
        for (int i = 3; i < amc::xs::XS_WORDS; ++i)
            if (!(std::fabs(rec[i]) < 9007199254740992.0) || rec[i] != std::floor(rec[i]))
                return fail(AMC_ERR_BAD_ARG, "amc_set_corr: record of sample %d, group %d, column %d: word %d is no integer below 2^53", slot, g, c, i);
        const amc::xs::PartR p = amc::xs::rec_to_r(rec);
        amc::xs_word* row = host.data() + s * amc::XS_ROW_R;
        row[0] = (amc::xs_word)(uint32_t)p.top | ((amc::xs_word)p.flags << 32);
        row[1] = (amc::xs_word)p.k1.lo; row[2] = (amc::xs_word)p.k1.hi;
        row[3] = (amc::xs_word)p.k2.lo; row[4] = (amc::xs_word)p.k2.hi;
    }
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(corr_room(h));
    AMC_HIP(hipMemcpyAsync(h->corr.d_origin, origin, (size_t)h->M * sizeof(double), hipMemcpyHostToDevice, h->stream));
    AMC_TRY(copy_to_device_sync(h, h->corr.d_corr, host.data(), host.size() * sizeof(amc::xs_word)));      // the caller's buffers are only valid during the call
    h->corr.observable = observable;
    h->corr.groups = G;
    h->corr.n_samples = n_samples;
    for (int s = 0; s < n_samples; ++s) h->corr.steps[s] = steps[s];
    return AMC_OK;
}

int amc_corr_clear(amc_handle* h)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_corr_clear: NULL handle");
    corr_forget(h);
    return AMC_OK;
}

}  // extern "C"
