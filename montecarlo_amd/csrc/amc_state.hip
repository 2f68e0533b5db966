// amc_state.hip -- the ensemble's state: upload / download (Float32 state through a Float64 staging copy), the initial ensemble,
// histograms (pooled, running, by rung of a temperature ladder), strided downloads, the step indices, the stream and the timing events.
#define AMC_KERNEL_LINKAGE static      // this object's own copies of the plain kernels it launches (initial ensemble, histograms, gathers)
#include "amc_internal.h"

// Wait for everything queued on the stream (or for one event).  The runtime's blocking wait parks the thread on an interrupt after a
// short spin and wakes it tens of microseconds after the device is done -- as long as a whole sweep; a host that steps
// the engine (callbacks, short timed regions) sees that latency on every hand-over.  So: poll for up to 5 ms (a query is a read of
// the queue's completion signal), then fall back to the blocking wait.
template <class Query, class Block>
static hipError_t spin_then_block(Query query, Block block)
{
    timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int spins = 0;; ++spins) {
        const hipError_t e = query();
        if (e != hipErrorNotReady) return e;
        if ((spins & 63) == 63) {
            timespec t1;
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec) > 5000000ll) break;
        }
    }
    return block();
}

hipError_t wait_stream(hipStream_t stream)
{
    return spin_then_block([&] { return hipStreamQuery(stream); }, [&] { return hipStreamSynchronize(stream); });
}

hipError_t wait_event(hipEvent_t ev)
{
    return spin_then_block([&] { return hipEventQuery(ev); }, [&] { return hipEventSynchronize(ev); });
}

int copy_to_host_sync(amc_handle* h, void* dst, const void* d_src, size_t bytes)
{
    if (d_src) AMC_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));
    return AMC_OK;
}

int copy_to_device_sync(amc_handle* h, void* d_dst, const void* src, size_t bytes)
{
    AMC_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));
    return AMC_OK;
}

int zeroed_words(amc_handle* h, unsigned long long** p, size_t bytes)
{
    if (*p) return AMC_OK;
    AMC_HIP(hipMalloc(p, bytes));
    AMC_HIP(hipMemsetAsync(*p, 0, bytes, h->stream));
    return AMC_OK;
}

// Float32 state: d_x64 (doubles) -> dst (floats, rounded to nearest) and back, on the stream.
static int narrow_from_x64(amc_handle* h, double* dst_as_float)
{
    const double* in = h->d_x64;
    int64_t n = h->M;
    void* params[] = {&in, &n, &dst_as_float};
    return rtc_launch(h, "amc::narrow_state_kernel", grid_for(h, h->M), params);
}

static int widen_to_x64(amc_handle* h)
{
    const double* in = h->d_x;
    int64_t n = h->M;
    double* out = h->d_x64;
    void* params[] = {&in, &n, &out};
    return rtc_launch(h, "amc::widen_state_kernel", grid_for(h, h->M), params);
}

// The positions as doubles on the device: d_x itself, or (Float32 state) the widened copy.
static int positions_f64(amc_handle* h, const double** out)
{
    *out = h->d_x;
    if (!h->f32) return AMC_OK;
    *out = h->d_x64;
    return widen_to_x64(h);
}

// What every histogram entry asks of its bins; the message is left for amc_last_error().
bool hist_args_ok(const char* who, double lo, double hi, int n_bins)
{
    if (n_bins >= 1 && n_bins <= 8192 && hi > lo && std::isfinite(lo) && std::isfinite(hi)) return true;
    fail(AMC_ERR_BAD_ARG, "%s: need 1 <= n_bins <= 8192 and finite lo < hi", who);
    return false;
}

// Every block ends with one 64-bit atomic per non-empty bin on the SAME few hundred addresses, and those serialise (~13 ns
// each per address): a full grid of 2048 blocks spends 27 us there.  Two blocks per CU keep enough loads in flight and the
// flush short (1e7 chains, 200 bins: 53.1 us with 2048 blocks, 32.2 with 1024, 23.4 with 512, 27.0 with 256, 43.5 with 128).
int hist_grid(const amc_handle* h)
{
    const int g = 2 * h->n_cu;
    return g < h->red_blocks ? g : h->red_blocks;
}

// A histogram launch into a scratch buffer of `cells` cleared counters, copied to the caller's `counts`: launch(d_pos, d_counts) queues
// the kernel on the stream.  The buffer is freed on every path.
template <class Launch>
static int hist_to_host(amc_handle* h, const char* who, int cells, uint64_t* counts, Launch launch)
{
    unsigned long long* d_counts = nullptr;
    const size_t bytes = (size_t)cells * sizeof(unsigned long long);
    AMC_HIP(hipMalloc(&d_counts, bytes));
    hipError_t e = hipMemsetAsync(d_counts, 0, bytes, h->stream);
    const double* d_pos = nullptr;
    const int rc = e == hipSuccess ? positions_f64(h, &d_pos) : AMC_OK;
    if (e == hipSuccess && rc == AMC_OK) {
        launch(d_pos, d_counts);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(counts, d_counts, bytes, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    (void)hipFree(d_counts);
    if (rc != AMC_OK) return rc;
    if (e != hipSuccess) return fail(AMC_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return AMC_OK;
}

extern "C" {

int amc_upload_state(amc_handle* h, const double* x, const double* beta_or_null)
{
    if (!h || !x) return fail(AMC_ERR_BAD_ARG, "amc_upload_state: NULL argument");
    AMC_HIP(hipSetDevice(h->device));
    corr_forget(h);              // other positions in the slots: the mark of the time correlation goes
    chain_stats_forget(h);       // ... and the running sums per chain
    if (h->f32) {
        AMC_HIP(hipMemcpyAsync(h->d_x64, x, (size_t)h->M * sizeof(double), hipMemcpyHostToDevice, h->stream));
        AMC_TRY(narrow_from_x64(h, h->d_x));
    } else {
        AMC_HIP(hipMemcpyAsync(h->d_x, x, (size_t)h->M * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (beta_or_null) {
        if (!h->d_beta) {
            AMC_HIP(hipMalloc(&h->d_beta, (size_t)h->M_pad * sizeof(double)));
            AMC_HIP(hipMemsetAsync(h->d_beta, 0, (size_t)h->M_pad * sizeof(double), h->stream));
        }
        if (h->f32) {
            AMC_HIP(hipMemcpyAsync(h->d_x64, beta_or_null, (size_t)h->M * sizeof(double), hipMemcpyHostToDevice, h->stream));
            AMC_TRY(narrow_from_x64(h, h->d_beta));
        } else {
            AMC_HIP(hipMemcpyAsync(h->d_beta, beta_or_null, (size_t)h->M * sizeof(double), hipMemcpyHostToDevice, h->stream));
        }
        h->beta_arr = true;
    }
    AMC_HIP(hipStreamSynchronize(h->stream));   // caller's buffers are only valid during the call
    return AMC_OK;
}

int amc_init_uniform(amc_handle* h, double lo, double hi)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_init_uniform: NULL handle");
    AMC_HIP(hipSetDevice(h->device));
    corr_forget(h);
    chain_stats_forget(h);
    const int grid = grid_for(h, (h->M + 1) / 2);
    // Float32 state: System(Float32(lo + (hi - lo) u), beta) -- the Float64 ensemble, rounded
    hipLaunchKernelGGL(amc::init_uniform_kernel, dim3(grid), dim3(AMC_BLOCK), 0, h->stream, h->f32 ? h->d_x64 : h->d_x, h->M,
                       (uint64_t)h->offset >> 1, (uint32_t)h->seed, (uint32_t)(h->seed >> 32), lo, hi);
    AMC_HIP(hipGetLastError());
    if (h->f32) return narrow_from_x64(h, h->d_x);
    return AMC_OK;
}

int amc_download_state(amc_handle* h, double* x, double* e)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_download_state: NULL handle");
    if (!x && !e) return AMC_OK;
    AMC_HIP(hipSetDevice(h->device));
    double* dst = x;
    std::vector<double> tmp;
    if (!dst) { tmp.resize((size_t)h->M); dst = tmp.data(); }
    const double* d_pos = nullptr;
    AMC_TRY(positions_f64(h, &d_pos));
    AMC_HIP(hipMemcpyAsync(dst, d_pos, (size_t)h->M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));
    if (e && h->use_rtc) {
        // the host cannot evaluate the user's expression (or must not: Float32 arithmetic): e = potential(x) by the
        // run-time compiled kernel
        double* d_e = nullptr;
        AMC_HIP(hipMalloc(&d_e, (size_t)h->M * sizeof(double)));
        const double* d_x = h->d_x;
        int64_t m = h->M;
        void* params[] = {&d_x, &m, &d_e};
        int rc = rtc_launch(h, "amc::energy_kernel<" + std::to_string(h->potential) + ">", h->red_blocks, params);
        hipError_t he = hipSuccess;
        if (rc == AMC_OK) he = hipMemcpyAsync(e, d_e, (size_t)h->M * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (rc == AMC_OK && he == hipSuccess) he = hipStreamSynchronize(h->stream);
        (void)hipFree(d_e);
        if (rc != AMC_OK) return rc;
        if (he != hipSuccess) return fail(AMC_ERR_HIP, "amc_download_state: %s", hipGetErrorString(he));
        return AMC_OK;
    }
    if (e) {
        // e == potential(x) exactly (particle_1d.jl:33): the same two IEEE multiplies on the host
        for (int64_t c = 0; c < h->M; ++c) {
            const double xc = dst[c];
            if (h->potential == AMC_POTENTIAL_DOUBLE_WELL) {
                volatile double q = xc * xc;   // volatile: no host-side fma contraction of x*x - 1
                const double r = q - 1.0;
                e[c] = r * r;
            } else {
                e[c] = xc * xc;
            }
        }
    }
    return AMC_OK;
}

int amc_histogram(amc_handle* h, double lo, double hi, int n_bins, uint64_t* counts)
{
    if (!h || !counts) return fail(AMC_ERR_BAD_ARG, "amc_histogram: NULL argument");
    if (!hist_args_ok("amc_histogram", lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    AMC_HIP(hipSetDevice(h->device));
    const double inv_w = (double)n_bins / (hi - lo);
    return hist_to_host(h, "amc_histogram", n_bins + 3, counts, [&](const double* d_pos, unsigned long long* d_counts) {
        hipLaunchKernelGGL(amc::histogram_kernel, dim3(hist_grid(h)), dim3(AMC_BLOCK), (size_t)(n_bins + 3) * sizeof(unsigned int),
                           h->stream, d_pos, h->M, lo, hi, inv_w, n_bins, d_counts);
    });
}

int amc_histogram_rungs(amc_handle* h, double lo, double hi, int n_bins, uint64_t* counts)
{
    if (!h || !counts) return fail(AMC_ERR_BAD_ARG, "amc_histogram_rungs: NULL argument");
    AMC_TRY(need_ladder(h, "amc_histogram_rungs"));
    if (!hist_args_ok("amc_histogram_rungs", lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    AMC_HIP(hipSetDevice(h->device));
    const int cells = (n_bins + 3) * h->lad.n_rungs;
    const double inv_w = (double)n_bins / (hi - lo);
    const int lds_rows = cells <= 12288 ? 1 : 0;      // 48 KiB of u32 counters; beyond that one global atomic per position
    return hist_to_host(h, "amc_histogram_rungs", cells, counts, [&](const double* d_pos, unsigned long long* d_counts) {
        hipLaunchKernelGGL(amc::rung_histogram_kernel, dim3(hist_grid(h)), dim3(AMC_BLOCK), lds_rows ? (size_t)cells * sizeof(unsigned int) : 0,
                           h->stream, d_pos, h->M, h->lad.n_rungs, lo, hi, inv_w, n_bins, lds_rows, d_counts);
    });
}

int amc_histogram_accumulate(amc_handle* h, double lo, double hi, int n_bins)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_histogram_accumulate: NULL handle");
    if (!hist_args_ok("amc_histogram_accumulate", lo, hi, n_bins)) return AMC_ERR_BAD_ARG;
    AMC_HIP(hipSetDevice(h->device));
    if (h->d_hist && (n_bins != h->hist_bins || lo != h->hist_lo || hi != h->hist_hi))
        return fail(AMC_ERR_STATE, "amc_histogram_accumulate: the running histogram has other bins (fetch it with reset first)");
    if (!h->d_hist) {
        const size_t bytes = (size_t)(n_bins + 3) * sizeof(unsigned long long);
        AMC_HIP(hipMalloc(&h->d_hist, bytes));
        AMC_HIP(hipMemsetAsync(h->d_hist, 0, bytes, h->stream));
        h->hist_bins = n_bins; h->hist_lo = lo; h->hist_hi = hi;
    }
    const double inv_w = (double)n_bins / (hi - lo);
    const double* d_pos = nullptr;
    AMC_TRY(positions_f64(h, &d_pos));
    hipLaunchKernelGGL(amc::histogram_kernel, dim3(hist_grid(h)), dim3(AMC_BLOCK), (size_t)(n_bins + 3) * sizeof(unsigned int),
                       h->stream, d_pos, h->M, lo, hi, inv_w, n_bins, h->d_hist);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

int amc_histogram_fetch(amc_handle* h, uint64_t* counts, int n_bins, int reset)
{
    if (!h || !counts) return fail(AMC_ERR_BAD_ARG, "amc_histogram_fetch: NULL argument");
    if (!h->d_hist) return fail(AMC_ERR_STATE, "amc_histogram_fetch: nothing has been accumulated");
    if (n_bins != h->hist_bins) return fail(AMC_ERR_BAD_ARG, "amc_histogram_fetch: the running histogram has %d bins", h->hist_bins);
    AMC_HIP(hipSetDevice(h->device));
    const size_t bytes = (size_t)(n_bins + 3) * sizeof(unsigned long long);
    AMC_HIP(hipMemcpyAsync(counts, h->d_hist, bytes, hipMemcpyDeviceToHost, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));
    if (reset) {
        (void)hipFree(h->d_hist);
        h->d_hist = nullptr;
        h->hist_bins = 0;
    }
    return AMC_OK;
}

int amc_download_strided(amc_handle* h, int64_t first, int64_t stride, int64_t count, double* x)
{
    if (!h || !x) return fail(AMC_ERR_BAD_ARG, "amc_download_strided: NULL argument");
    // (no product that could overflow: count - 1 <= (M - 1 - first) / stride)
    if (first < 0 || stride < 1 || count < 0 || (count > 0 && (first >= h->M || count - 1 > (h->M - 1 - first) / stride)))
        return fail(AMC_ERR_BAD_ARG, "amc_download_strided: range [first + i*stride] leaves the local shard");
    if (count == 0) return AMC_OK;
    AMC_HIP(hipSetDevice(h->device));
    double* d_out = nullptr;
    AMC_HIP(hipMalloc(&d_out, (size_t)count * sizeof(double)));
    const double* d_pos = nullptr;
    { const int rc = positions_f64(h, &d_pos); if (rc != AMC_OK) { (void)hipFree(d_out); return rc; } }
    hipLaunchKernelGGL(amc::gather_strided_kernel, dim3(grid_for(h, count)), dim3(AMC_BLOCK), 0, h->stream, d_pos, first,
                       stride, count, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(x, d_out, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(AMC_ERR_HIP, "amc_download_strided: %s", hipGetErrorString(e));
    return AMC_OK;
}

int amc_get_estimator_step(amc_handle* h, uint64_t* t)
{
    if (!h || !t) return fail(AMC_ERR_BAD_ARG, "amc_get_estimator_step: NULL argument");
    *t = h->t_est;
    return AMC_OK;
}

int amc_set_estimator_step(amc_handle* h, uint64_t t)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_estimator_step: NULL handle");
    if (t >> 48) return fail(AMC_ERR_BAD_ARG, "amc_set_estimator_step: call index must fit 48 bits");
    h->t_est = t;
    return AMC_OK;
}

int amc_get_step(amc_handle* h, uint64_t* t)
{
    if (!h || !t) return fail(AMC_ERR_BAD_ARG, "amc_get_step: NULL argument");
    *t = h->t;
    return AMC_OK;
}

int amc_set_step(amc_handle* h, uint64_t t)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_set_step: NULL handle");
    if (t >> 48) return fail(AMC_ERR_BAD_ARG, "amc_set_step: step index must fit 48 bits");
    h->t = t;
    return AMC_OK;
}

int amc_sync(amc_handle* h)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_sync: NULL handle");
    AMC_HIP(hipSetDevice(h->device));
    AMC_HIP(wait_stream(h->stream));
    return AMC_OK;
}

int amc_get_stream(amc_handle* h, void** stream)
{
    if (!h || !stream) return fail(AMC_ERR_BAD_ARG, "amc_get_stream: NULL argument");
    *stream = (void*)h->stream;
    return AMC_OK;
}

int amc_timing_begin(amc_handle* h)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_timing_begin: NULL handle");
    AMC_HIP(hipSetDevice(h->device));
    AMC_HIP(hipEventRecord(h->ev0, h->stream));
    return AMC_OK;
}

int amc_timing_mark(amc_handle* h)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_timing_mark: NULL handle");
    AMC_HIP(hipSetDevice(h->device));
    AMC_HIP(hipEventRecord(h->ev1, h->stream));
    h->ev1_marked = true;
    return AMC_OK;
}

int amc_timing_end(amc_handle* h, double* elapsed_ms)
{
    if (!h || !elapsed_ms) return fail(AMC_ERR_BAD_ARG, "amc_timing_end: NULL argument");
    AMC_HIP(hipSetDevice(h->device));
    if (!h->ev1_marked) AMC_HIP(hipEventRecord(h->ev1, h->stream));
    h->ev1_marked = false;
    AMC_HIP(wait_stream(h->stream));           // the end event has completed once the stream has drained up to it
    AMC_HIP(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    AMC_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *elapsed_ms = (double)ms;
    return AMC_OK;
}

}  // extern "C"
