// amc_parameters.hip -- the parameter table of the moves: sigma and weights at creation (push_params), a policy's parameters set
// and read (amc_set / get_parameters), and the read queued in stream order (amc_parameters_begin / _end / _end_all).
#define AMC_KERNEL_LINKAGE static      // this object's own copies of the plain kernels it launches (parameter tables)
#include "amc_internal.h"

// Float32 policy parameters: a parameter is checked, not rounded -- no caller gets a sigma they did not write -- and the range is
// the one in which the Float32 arithmetic on sigma stays normal and finite (include/amc.h, amc_config.param_dtype).
int check_sigma_f32(const char* who, int k, double s)
{
    if (!((double)(float)s == s))
        return fail(AMC_ERR_BAD_ARG, "%s: sigma[%d] = %.17g is not a Float32 value (param_dtype = AMC_DTYPE_F32 takes (double)(float)sigma)", who, k, s);
    if (!(s >= AMC_SIGMA_F32_MIN) || !(s <= AMC_SIGMA_F32_MAX))
        return fail(AMC_ERR_BAD_ARG, "%s: sigma[%d] must lie in [2^-63, 2^60] with param_dtype = AMC_DTYPE_F32 (got %.9g)", who, k, s);
    return AMC_OK;
}

// what derives from sigma, in the arithmetic of the handle's parameter type
static int launch_prepare_params(amc_handle* h)
{
    if (h->param_f32) hipLaunchKernelGGL(amc::prepare_params_f32_kernel, dim3(1), dim3(64), 0, h->stream, h->d_ptab, h->K);
    else hipLaunchKernelGGL(amc::prepare_params_kernel, dim3(1), dim3(64), 0, h->stream, h->d_ptab, h->K);
    AMC_HIP(hipGetLastError());
    return AMC_OK;
}

int push_params(amc_handle* h, const double* sigma, const double* weight)
{
    AMC_TRY(pg_resolve(h));
    std::vector<double> tab((size_t)amc::PT_ROWS * AMC_MAX_MOVES, 0.0);
    AMC_HIP(hipMemcpyAsync(tab.data(), h->d_ptab, tab.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < h->K; ++k) {
        if (sigma) tab[amc::PT_SIGMA * AMC_MAX_MOVES + k] = sigma[k];
        if (weight) tab[amc::PT_WEIGHT * AMC_MAX_MOVES + k] = weight[k];
    }
    AMC_HIP(hipMemcpyAsync(h->d_ptab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));   // tab is a stack-scoped host buffer
    AMC_TRY(launch_prepare_params(h));
    if (weight && h->K > 1) {      // the cumulative weights changed: rebuild the 12-bit move-pick table from them
        hipLaunchKernelGGL(amc::prepare_pick_kernel, dim3(AMC_PICK_CELLS / AMC_BLOCK), dim3(AMC_BLOCK), 0, h->stream, h->d_ptab, h->K,
                           h->d_pick);
        AMC_HIP(hipGetLastError());
    }
    return AMC_OK;
}

// row of the parameter table that holds parameter p of every move
static int theta_row(int p) { return p == 0 ? (int)amc::PT_SIGMA : (int)amc::PT_THETA1 + p - 1; }

static int parameters_end_impl(amc_handle* h, const char* who, double* out, int per_move)
{
    if (!h || !out) return fail(AMC_ERR_BAD_ARG, "%s: NULL argument", who);
    if (!h->params_pending) return fail(AMC_ERR_STATE, "%s: no read in flight (call amc_parameters_begin)", who);
    AMC_HIP(hipSetDevice(h->device));
    AMC_HIP(wait_event(h->ev_params));           // waits for that copy only, not for work queued after it
    h->params_pending = false;
    for (int k = 0; k < h->K; ++k)
        for (int p = 0; p < per_move; ++p) out[(size_t)k * per_move + p] = h->h_params[(size_t)p * AMC_MAX_MOVES + k];
    return AMC_OK;
}

extern "C" {

int amc_set_parameters(amc_handle* h, int k, const double* p, int n)
{
    if (!h || !p) return fail(AMC_ERR_BAD_ARG, "amc_set_parameters: NULL argument");
    if (k < 0 || k >= h->K) return fail(AMC_ERR_BAD_ARG, "amc_set_parameters: move index %d out of range", k);
    if (n != h->n_params)
        return fail(AMC_ERR_BAD_ARG, h->n_params == 1 ? "amc_set_parameters: StandardGaussian has exactly 1 parameter (sigma)"
                                                     : "amc_set_parameters: this handle's policy has %d parameters", h->n_params);
    if (h->n_params == 1) {
        if (h->param_f32) {
            AMC_TRY(check_sigma_f32("amc_set_parameters", k, p[0]));
        } else if (!(p[0] >= 1e-100) || !(p[0] <= 1e100))
            return fail(AMC_ERR_BAD_ARG, "amc_set_parameters: sigma must lie in [1e-100, 1e100] (got %.17g)", p[0]);
    } else {
        for (int i = 0; i < n; ++i)
            if (!(p[i] - p[i] == 0.0)) return fail(AMC_ERR_BAD_ARG, "amc_set_parameters: parameter %d is not finite", i);
    }
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));
    for (int i = 0; i < n; ++i)
        AMC_HIP(hipMemcpyAsync(h->d_ptab + theta_row(i) * AMC_MAX_MOVES + k, p + i, sizeof(double), hipMemcpyHostToDevice, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));
    if (h->n_params == 1) {            // what derives from sigma (the script kernels of a policy with several parameters read none of it)
        AMC_TRY(launch_prepare_params(h));
    }
    return AMC_OK;
}

int amc_get_parameters(amc_handle* h, int k, double* p, int n)
{
    if (!h || !p) return fail(AMC_ERR_BAD_ARG, "amc_get_parameters: NULL argument");
    if (k < 0 || k >= h->K) return fail(AMC_ERR_BAD_ARG, "amc_get_parameters: move index %d out of range", k);
    if (n != h->n_params)
        return fail(AMC_ERR_BAD_ARG, h->n_params == 1 ? "amc_get_parameters: StandardGaussian has exactly 1 parameter (sigma)"
                                                     : "amc_get_parameters: this handle's policy has %d parameters", h->n_params);
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));
    for (int i = 0; i < n; ++i)
        AMC_HIP(hipMemcpyAsync(p + i, h->d_ptab + theta_row(i) * AMC_MAX_MOVES + k, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    AMC_HIP(hipStreamSynchronize(h->stream));
    return AMC_OK;
}

int amc_n_params(amc_handle* h, int* n_params, int* gd_stride)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_n_params: NULL handle");
    if (n_params) *n_params = h->n_params;
    if (gd_stride) *gd_stride = amc::pg_gd_stride(h->n_params);
    return AMC_OK;
}

int amc_parameters_begin(amc_handle* h)
{
    if (!h) return fail(AMC_ERR_BAD_ARG, "amc_parameters_begin: NULL handle");
    if (h->params_pending) return fail(AMC_ERR_STATE, "amc_parameters_begin: a read is already in flight (call amc_parameters_end)");
    AMC_HIP(hipSetDevice(h->device));
    AMC_TRY(pg_resolve(h));
    AMC_HIP(hipMemcpyAsync(h->h_params, h->d_ptab + amc::PT_SIGMA * AMC_MAX_MOVES, (size_t)h->K * sizeof(double), hipMemcpyDeviceToHost,
                           h->stream));
    if (h->n_params > 1)         // parameters 1 .. P - 1: consecutive rows of the table
        AMC_HIP(hipMemcpyAsync(h->h_params + AMC_MAX_MOVES, h->d_ptab + amc::PT_THETA1 * AMC_MAX_MOVES,
                               (size_t)(h->n_params - 1) * AMC_MAX_MOVES * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    AMC_HIP(hipEventRecord(h->ev_params, h->stream));
    h->params_pending = true;
    return AMC_OK;
}

int amc_parameters_end(amc_handle* h, double* sigma) { return parameters_end_impl(h, "amc_parameters_end", sigma, 1); }

int amc_parameters_end_all(amc_handle* h, double* parameters, int n)
{
    if (h && n != h->K * h->n_params)
        return fail(AMC_ERR_BAD_ARG, "amc_parameters_end_all: this handle has %d moves of %d parameters", h->K, h->n_params);
    return parameters_end_impl(h, "amc_parameters_end_all", parameters, h ? h->n_params : 1);
}

}  // extern "C"
