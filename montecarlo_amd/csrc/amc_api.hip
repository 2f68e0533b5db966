// amc_api.hip -- C ABI (include/amc.h) over the HIP kernels of amc_kernels.h: errors, handle creation and destruction.
//
// Host side of the engine: owns device memory, the stream and the step counter;
// validates arguments the way the reference's constructors assert them
// (src/metropolis.jl:248-251, Distributions.Categorical's probability-vector check).
// No CPU fallback: every entry point either runs on the GPU or returns an error.
// This object holds the headers' plain kernels; the other units keep static copies of those they launch.
#include "amc_internal.h"

static thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...)
{
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int grid_for(const amc_handle* h, int64_t n_items, int blocks_per_cu)
{
    // memory-streaming shape: <= 8 blocks of 256 per CU, grid-stride the rest
    int64_t blocks = (n_items + AMC_BLOCK - 1) / AMC_BLOCK;
    const int64_t cap = (int64_t)h->n_cu * (blocks_per_cu > 0 ? blocks_per_cu : h->blocks_per_cu);
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

const char* amc_env(const char* name) { return std::getenv(name); }

// The handle knobs of amc_internal.h's table, as the environment has them now.
AmcKnobs amc_knobs()
{
    auto in = [](const char* name, int lo, int hi) { const char* e = amc_env(name); const int v = e ? std::atoi(e) : 0; return v >= lo && v <= hi ? v : 0; };
    auto flag = [](const char* name) { const char* e = amc_env(name); return e && std::atoi(e) != 0; };
    auto set = [](const char* name) { return amc_env(name) != nullptr; };
    auto text = [](const char* name) { const char* e = amc_env(name); return std::string(e ? e : ""); };
    AmcKnobs k;
    k.blocks_per_cu = in("AMC_BLOCKS_PER_CU", 1, 64);
    k.blocks_per_cu_single = in("AMC_BLOCKS_PER_CU_SINGLE", 1, 64);
    k.blocks_per_cu_reduce = in("AMC_BLOCKS_PER_CU_REDUCE", 1, 64);
    k.log_depth = in("AMC_LOG_DEPTH", 1, 255);
    k.exact_accept = flag("AMC_EXACT_ACCEPT");
    { const char* e = amc_env("AMC_WIDE_COUNTERS"); k.wide_counters = e && *e && *e != '0'; }
    k.wide_red_rows = flag("AMC_WIDE_RED_ROWS");
    k.shard_route_one_rank = flag("AMC_SHARD_ROUTE_ON_ONE_RANK");
    k.no_deferred_update = flag("AMC_NO_DEFERRED_UPDATE");
    k.class_per_move = flag("AMC_CLASS_PER_MOVE");
    k.no_column_skip = flag("AMC_NO_COLUMN_SKIP");
    k.np_small_launches = flag("AMC_NP_SMALL_LAUNCHES");
    k.no_sweep_estimator_fusion = set("AMC_NO_SWEEP_ESTIMATOR_FUSION");
    k.sweep_slices = in("AMC_SWEEP_SLICES", 1, amc::AMC_MAX_SLICES);
    k.sweep_slice_blocks_per_cu = in("AMC_SWEEP_SLICE_BLOCKS_PER_CU", 1, 64);
    { const char* e = amc_env("AMC_SWEEP_SLICE_MIN_CHAINS"); const long long v = e && *e ? std::atoll(e) : -1; k.sweep_slice_min_chains = v >= 0 ? v : -1; }
    k.debug_plan = set("AMC_DEBUG_PLAN");
    k.rtc_licm = text("AMC_RTC_LICM");
    k.rtc_waves_set = set("AMC_RTC_WAVES");
    k.rtc_waves = text("AMC_RTC_WAVES");
    k.no_gauss_class_rows = set("AMC_NO_GAUSS_CLASS_ROWS");
    k.no_sigma_memo = set("AMC_NO_SIGMA_MEMO");
    k.model_check_f32 = text("AMC_MODEL_CHECK_F32")[0] == '1';
    k.model_check_inst = text("AMC_MODEL_CHECK_INST");
    return k;
}

extern "C" {

const char* amc_last_error(void) { return g_last_error.c_str(); }

int amc_version(void) { return AMC_VERSION_MAJOR * 1000 + AMC_VERSION_MINOR; }

int amc_device_count(int* count)
{
    if (!count) return fail(AMC_ERR_BAD_ARG, "amc_device_count: count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(AMC_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return AMC_OK;
}

// The expressions of a model's classes, checked as text (validate_potential_expr: one line of ordinary expression text that
// mentions what it must).  The derivative of a class with one parameter must mention it where the class is the model's first --
// sigma, or theta0, its other name --; the partials of several parameters need not mention anything.
static int validate_classes(const ModelSpec& spec)
{
    int rc = AMC_OK;
    for (size_t c = 0; rc == AMC_OK && c < spec.classes.size(); ++c) {
        const PolicyClass& pc = spec.classes[c];
        rc = validate_potential_expr(pc.sample.c_str(), "sample_action expression", "z");
        if (rc == AMC_OK) rc = validate_potential_expr(pc.logq.c_str(), "log_proposal_density expression", "delta");
        if (rc == AMC_OK && !pc.dlogq.empty()) {
            const char* d0 = pc.dlogq[0].c_str();
            const bool named = c == 0 && spec.n_params == 1;
            rc = validate_potential_expr(d0, "d log_proposal_density / d sigma expression", named ? "sigma" : "");
            if (rc != AMC_OK && named && validate_potential_expr(d0, "d log_proposal_density / d sigma expression", "theta0") == AMC_OK) rc = AMC_OK;
        }
        for (size_t p = 1; rc == AMC_OK && p < pc.dlogq.size(); ++p)
            rc = validate_potential_expr(pc.dlogq[p].c_str(), "d log_proposal_density / d theta expression", "");
        if (rc == AMC_OK && pc.perform.empty() != pc.invert.empty())      // (the entries that take arrays have checked it, class by class)
            rc = fail(AMC_ERR_BAD_ARG, "amc_create_action_model: perform_expr and invert_expr come together (No invert_action! is defined)");
        if (rc == AMC_OK && !pc.perform.empty()) rc = validate_potential_expr(pc.perform.c_str(), "perform_action expression", "delta");
        if (rc == AMC_OK && !pc.invert.empty()) rc = validate_potential_expr(pc.invert.c_str(), "invert_action expression", "delta");
    }
    return rc;
}

// An expression of the C ABI as a ModelSpec field.  NULL: not given.  An empty one stays given -- a NUL character, which
// validate_potential_expr reads as the empty expression it refuses.
static std::string given(const char* expr) { return !expr ? std::string() : *expr ? std::string(expr) : std::string(1, '\0'); }

// The C arguments of a script-defined model as a ModelSpec.  The arrays hold one entry per class -- dlogq_exprs the partials of the
// one class where n_params > 1 --; a NULL array or entry: not given.  who != nullptr: with the checks of the entries that take
// arrays (every class has sample and logq, perform and invert come together), `note` behind the first one's message.
static int model_spec(const char* who, const char* note, const char* potential_expr, const char* reward_expr, const char* scale_expr, int n_params,
                      int n_classes, const char* const* sample_exprs, const char* const* logq_exprs, const char* const* dlogq_exprs,
                      const char* const* perform_exprs, const char* const* invert_exprs, ModelSpec* spec)
{
    for (int c = 0; who && c < n_classes; ++c) {
        if (!sample_exprs[c] || !logq_exprs[c]) return fail(AMC_ERR_BAD_ARG, "%s: class %d has no sample / logq expression%s", who, c, note);
        const bool p = perform_exprs && perform_exprs[c], i = invert_exprs && invert_exprs[c];
        if (p != i) return fail(AMC_ERR_BAD_ARG, "%s: class %d: perform_expr and invert_expr come together (No invert_action! is defined)", who, c);
    }
    spec->potential = given(potential_expr);
    spec->reward = given(reward_expr);
    spec->scale = given(scale_expr);
    spec->n_params = n_params;
    for (int c = 0; c < n_classes; ++c) {
        PolicyClass pc;
        pc.sample = given(sample_exprs[c]);
        pc.logq = given(logq_exprs[c]);
        for (int q = 0; dlogq_exprs && dlogq_exprs[c] && q < n_params; ++q) pc.dlogq.push_back(given(dlogq_exprs[c + q]));
        pc.perform = given(perform_exprs ? perform_exprs[c] : nullptr);
        pc.invert = given(invert_exprs ? invert_exprs[c] : nullptr);
        spec->classes.push_back(pc);
    }
    return AMC_OK;
}

// spec: the script-defined part of the model (an empty one: amc_create's); its dtype switches are set here, from the config
static int create_impl(const amc_config* cfg, const ModelSpec& spec, amc_handle** out)
{
    if (!cfg || !out) return fail(AMC_ERR_BAD_ARG, "amc_create: NULL argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(amc_config) && cfg->struct_size != AMC_CONFIG_SIZE_V0_1)
        return fail(AMC_ERR_BAD_ARG, "amc_create: struct_size %u != %zu (ABI mismatch)", cfg->struct_size, sizeof(amc_config));
    const int state_dtype = cfg->struct_size == sizeof(amc_config) ? cfg->state_dtype : (int)AMC_DTYPE_F64;
    if (state_dtype != AMC_DTYPE_F64 && state_dtype != AMC_DTYPE_F32)
        return fail(AMC_ERR_BAD_ARG, "amc_create: unknown state_dtype %d", state_dtype);
    const int param_dtype = cfg->struct_size == sizeof(amc_config) ? cfg->param_dtype : (int)AMC_DTYPE_F64;
    if (param_dtype != AMC_DTYPE_F64 && param_dtype != AMC_DTYPE_F32)
        return fail(AMC_ERR_BAD_ARG, "amc_create: unknown param_dtype %d", param_dtype);
    const bool param_f32 = param_dtype == AMC_DTYPE_F32;
    if (param_f32 && state_dtype != AMC_DTYPE_F32)
        return fail(AMC_ERR_BAD_ARG, "amc_create: param_dtype = AMC_DTYPE_F32 requires state_dtype = AMC_DTYPE_F32 (a Float32 sigma under "
                                     "Float64 state promotes to the Float64 arithmetic: ask for param_dtype = AMC_DTYPE_F64)");
    if (param_f32 && (!spec.scale.empty() || !spec.classes.empty()))
        return fail(AMC_ERR_BAD_ARG, "amc_create: script-defined policies are not available with param_dtype = AMC_DTYPE_F32 "
                                     "(Float32 policy parameters: the built-in Gaussian policy only)");
    if (cfg->n_chains < 1) return fail(AMC_ERR_BAD_ARG, "amc_create: n_chains must be >= 1");
    if (cfg->chain_offset < 0 || (cfg->chain_offset & 1))
        return fail(AMC_ERR_BAD_ARG, "amc_create: chain_offset must be even and >= 0 (shards split on chain pairs)");
    if (cfg->n_chains_global < cfg->chain_offset + cfg->n_chains)
        return fail(AMC_ERR_BAD_ARG, "amc_create: n_chains_global < chain_offset + n_chains");
    if (cfg->n_moves < 1 || cfg->n_moves > AMC_MAX_MOVES)
        return fail(AMC_ERR_BAD_ARG, "amc_create: n_moves must be in [1, %d]", AMC_MAX_MOVES);
    if (cfg->sweepstep < 1) return fail(AMC_ERR_BAD_ARG, "amc_create: sweepstep must be >= 1");
    if (cfg->potential == AMC_POTENTIAL_CUSTOM) {
        if (spec.potential.empty())
            return fail(AMC_ERR_BAD_ARG, "amc_create: AMC_POTENTIAL_CUSTOM needs its expression: use amc_create_custom");
        int rc_expr = validate_potential_expr(spec.potential.c_str());
        if (rc_expr == AMC_OK && !spec.reward.empty()) rc_expr = validate_potential_expr(spec.reward.c_str(), "custom reward", "delta");
        if (rc_expr == AMC_OK && !spec.scale.empty()) rc_expr = validate_potential_expr(spec.scale.c_str(), "proposal-width scale", "x");
        if (rc_expr == AMC_OK) rc_expr = validate_classes(spec);
        if (rc_expr != AMC_OK) return rc_expr;
    } else if (!spec.potential.empty()) {
        return fail(AMC_ERR_BAD_ARG, "amc_create_custom: cfg->potential must be AMC_POTENTIAL_CUSTOM");
    } else if (cfg->potential != AMC_POTENTIAL_HARMONIC && cfg->potential != AMC_POTENTIAL_DOUBLE_WELL) {
        return fail(AMC_ERR_BAD_ARG, "amc_create: unknown potential id %d", cfg->potential);
    }
    if (!cfg->sigma || !cfg->weight) return fail(AMC_ERR_BAD_ARG, "amc_create: sigma/weight is NULL");
    double wsum = 0.0;
    for (int k = 0; k < cfg->n_moves; ++k) {
        if (param_f32) {
            AMC_TRY(check_sigma_f32("amc_create", k, cfg->sigma[k]));
        } else if (!(cfg->sigma[k] >= 1e-100) || !(cfg->sigma[k] <= 1e100))
            return fail(AMC_ERR_BAD_ARG, "amc_create: sigma[%d] must lie in [1e-100, 1e100]", k);
        if (!(cfg->weight[k] >= 0.0) || !std::isfinite(cfg->weight[k]))
            return fail(AMC_ERR_BAD_ARG, "amc_create: weight[%d] must be finite and >= 0", k);
        wsum += cfg->weight[k];
    }
    // Categorical(weights) requires a probability vector (isprobvec: sum ~ 1, rtol sqrt(eps))
    if (std::fabs(wsum - 1.0) > 1.4901161193847656e-08)
        return fail(AMC_ERR_BAD_ARG, "amc_create: weights must sum to 1 (got %.17g)", wsum);

    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev < 1)
        return fail(AMC_ERR_NO_DEVICE, "amc_create: no HIP device (%s); this engine has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "count = 0");
    if (cfg->device < 0 || cfg->device >= n_dev)
        return fail(AMC_ERR_BAD_ARG, "amc_create: device %d out of range [0, %d)", cfg->device, n_dev);
    AMC_HIP(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    AMC_HIP(hipGetDeviceProperties(&prop, cfg->device));

    amc_handle* h = new (std::nothrow) amc_handle();
    if (!h) return fail(AMC_ERR_OOM, "amc_create: host allocation failed");
    h->device = cfg->device;
    h->knobs = amc_knobs();
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        // "gfx950:sramecc+:xnack-" -> "gfx950": run-time compiled kernels target the device they will run on; the offline
        // kernels of this library were built for AMC_BUILD_ARCH and cannot run anywhere else
        std::string arch(prop.gcnArchName);
        const size_t colon = arch.find(':');
        if (colon != std::string::npos) arch.erase(colon);
        if (!arch.empty()) h->arch = arch;
        if (h->arch != AMC_BUILD_ARCH) {
            delete h;
            return fail(AMC_ERR_NO_DEVICE, "amc_create: device %d is %s, this libamc.so was built for %s (make ARCH=%s)", cfg->device,
                        arch.c_str(), AMC_BUILD_ARCH, arch.c_str());
        }
    }
    // 8 resident blocks per CU; the single-step launch of the K = 1 pool-wide-counter sweep (no step log) measures 5 %
    // faster with 6 (29.4 vs 31.2 us at 1e7 chains; its fused launches and all other forms are fastest at 8)
    // (round 5: the K > 1 single-step launch holds 7 blocks per CU -- 70 VGPRs -- and ONE round of them is 4 % faster than 8 on
    // 7 slots, 31.1 against 32.4 us; env AMC_BLOCKS_PER_CU_SINGLE)
    h->blocks_per_cu = 8;
    h->blocks_per_cu_single = (cfg->n_moves == 1 && !cfg->per_chain_counters) ? 6 : (cfg->n_moves > 1 ? 7 : 8);
    if (h->knobs.blocks_per_cu) h->blocks_per_cu = h->blocks_per_cu_single = h->blocks_per_cu_pg = h->knobs.blocks_per_cu;
    if (h->knobs.blocks_per_cu_single) h->blocks_per_cu_single = h->knobs.blocks_per_cu_single;
    if (h->knobs.blocks_per_cu_reduce) h->blocks_per_cu_red = h->knobs.blocks_per_cu_reduce;
    if (h->knobs.sweep_slices) h->sweep_slices = h->knobs.sweep_slices;
    if (h->knobs.sweep_slice_blocks_per_cu) h->slice_blocks_per_cu = h->knobs.sweep_slice_blocks_per_cu;
    if (h->knobs.sweep_slice_min_chains >= 0) h->slice_min_chains = h->knobs.sweep_slice_min_chains;
    h->M = cfg->n_chains;
    // padding: unclamped 16-B tail loads stay in bounds; rows of every per-chain array start on a 256-byte boundary
    // (M_pad is a multiple of 256): a wave's 128-byte step-log store then covers exactly one aligned line
    h->M_pad = ((cfg->n_chains + AMC_PAD_DOUBLES + 255) / 256) * 256;
    h->offset = cfg->chain_offset;
    h->M_global = cfg->n_chains_global;
    h->potential = cfg->potential;
    h->f32 = state_dtype == AMC_DTYPE_F32;
    h->param_f32 = param_f32;
    h->use_rtc = h->f32 || cfg->potential == AMC_POTENTIAL_CUSTOM;
    // the model, and what the other units read of it
    h->model = spec;
    h->model.f32 = h->f32;
    h->model.param_f32 = param_f32;
    h->scaled_policy = !spec.scale.empty();
    h->script_policy = !spec.classes.empty();
    h->script_dlogq = h->script_policy && !spec.classes[0].dlogq.empty();
    h->n_params = spec.n_params;
    if (spec.classes.size() > 1) {
        h->n_classes = (int)spec.classes.size();
        for (int k = 0; k < cfg->n_moves; ++k) h->class_of_move[k] = spec.class_of_move[k];
    }
    h->K = cfg->n_moves;
    h->sweepstep = cfg->sweepstep;
    h->counters = cfg->per_chain_counters != 0 || cfg->n_moves > 1;
    h->beta = cfg->beta;
    h->seed = cfg->seed;

    int rc = AMC_OK;
    auto bail = [&](int code) { amc_destroy(h); return code; };
#define CREATE_HIP(call)                                                                \
    do {                                                                                \
        hipError_t e2_ = (call);                                                        \
        if (e2_ != hipSuccess) {                                                        \
            rc = fail(e2_ == hipErrorOutOfMemory ? AMC_ERR_OOM : AMC_ERR_HIP,           \
                      "%s failed: %s", #call, hipGetErrorString(e2_));                  \
            return bail(rc);                                                            \
        }                                                                               \
    } while (0)

    if (cfg->stream) {
        h->stream = (hipStream_t)cfg->stream;
    } else {
        CREATE_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    CREATE_HIP(hipMalloc(&h->d_x, (size_t)h->M_pad * sizeof(double)));
    CREATE_HIP(hipMemsetAsync(h->d_x, 0, (size_t)h->M_pad * sizeof(double), h->stream));
    if (h->counters) {
        // u16 planes suit a handle with K <= 4 (the register-resident fold); AMC_WIDE_COUNTERS keeps plain u32 arrays
        CREATE_HIP(alloc_counters(h, h->K <= 4 && !h->knobs.wide_counters));
        // Half a byte (K <= 8) or one byte per chain and MH step; folding costs a read-modify-write of every counter, so a
        // deeper log amortises it over more steps: 128 rows where rows of one byte per chain fit in 2 GiB (0.64 / 1.28 GB at
        // 1e7 chains), never below 16.
        {
            const int64_t fit = (int64_t)(2147483648ll / h->M_pad);
            h->log_depth = (int)(fit > 128 ? 128 : (fit < 16 ? 16 : fit));
        }
        if (h->knobs.log_depth) h->log_depth = h->knobs.log_depth;
        // K <= AMC_PACKED_LOG_MOVES: two chains per byte (store_log_pair)
        const size_t row_bytes = log_form(h) == AMC_LOG_PACKED ? (size_t)h->M_pad / 2 : (size_t)h->M_pad;
        CREATE_HIP(hipMalloc(&h->d_log, (size_t)h->log_depth * row_bytes));
        CREATE_HIP(hipMemsetAsync(h->d_log, 0, (size_t)h->log_depth * row_bytes, h->stream));
    }
    CREATE_HIP(hipMalloc(&h->d_ptab, (size_t)amc::PT_ROWS * AMC_MAX_MOVES * sizeof(double)));
    CREATE_HIP(hipMemsetAsync(h->d_ptab, 0, (size_t)amc::PT_ROWS * AMC_MAX_MOVES * sizeof(double), h->stream));
    CREATE_HIP(hipMalloc(&h->d_pick, AMC_PICK_CELLS));
    CREATE_HIP(hipMemsetAsync(h->d_pick, 0, AMC_PICK_CELLS, h->stream));
    CREATE_HIP(hipMalloc(&h->d_totals, 2 * AMC_MAX_MOVES * sizeof(unsigned long long)));
    CREATE_HIP(hipMemsetAsync(h->d_totals, 0, 2 * AMC_MAX_MOVES * sizeof(unsigned long long), h->stream));
    // room for two rounds of the estimator kernels' resident blocks (pg_plan: up to 2 x 5 per CU) beside the sweeps' 8 per CU
    const int slots_per_cu = std::max(std::max(std::max(h->blocks_per_cu, h->blocks_per_cu_single), h->blocks_per_cu_red), 10);
    h->n_slots = h->n_cu * slots_per_cu;
    CREATE_HIP(hipMalloc(&h->d_acc_slots, (size_t)h->n_slots * sizeof(unsigned long long)));
    CREATE_HIP(hipMemsetAsync(h->d_acc_slots, 0, (size_t)h->n_slots * sizeof(unsigned long long), h->stream));
    h->red_blocks = grid_for(h, h->M, slots_per_cu);
    CREATE_HIP(hipMalloc(&h->d_partials, (size_t)(h->red_blocks + amc::PG_GROUP) * PG_MAX_COLS * amc::XS_ROW_R * sizeof(amc::xs_word)));   // whole groups
    for (int i = 0; i < RED_TICKETS; ++i) {
        RedTicket& t = h->red[i];
        CREATE_HIP(hipHostMalloc((void**)&t.h_rows, (size_t)h->n_slots * RED_HOST_STRIDE * sizeof(amc::xs_word), 0));
        CREATE_HIP(hipHostMalloc((void**)&t.h_ratio, (size_t)h->n_slots * RATIO_STRIDE * amc::XS_ROW_Q * sizeof(amc::xs_word), 0));
        CREATE_HIP(hipMalloc(&t.d_ratio_acc, (size_t)AMC_MAX_MOVES * 3 * sizeof(unsigned long long)));
        CREATE_HIP(hipHostMalloc((void**)&t.h_ratio_acc, (size_t)AMC_MAX_MOVES * 3 * sizeof(unsigned long long), 0));
        CREATE_HIP(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming));
    }
    CREATE_HIP(hipMalloc(&h->d_out, (size_t)PG_MAX_COLS * amc::xs::XS_WORDS * sizeof(double)));
    CREATE_HIP(hipHostMalloc((void**)&h->h_pg_out, (size_t)AMC_MAX_LEARN * PG_NP_MAX_COLS * amc::xs::XS_WORDS * sizeof(double), 0));
    CREATE_HIP(hipMalloc(&h->d_gd_acc, (size_t)AMC_MAX_MOVES * AMC_GD_STRIDE_MAX * sizeof(double)));
    CREATE_HIP(hipMemsetAsync(h->d_gd_acc, 0, (size_t)AMC_MAX_MOVES * AMC_GD_STRIDE_MAX * sizeof(double), h->stream));
    CREATE_HIP(hipMalloc(&h->d_status, sizeof(int)));
    CREATE_HIP(hipMemsetAsync(h->d_status, 0, sizeof(int), h->stream));
    {
        const size_t groups = (size_t)(h->n_slots + amc::PG_GROUP - 1) / amc::PG_GROUP + 1;
        CREATE_HIP(hipMalloc(&h->d_pg_tickets, (groups + 1) * sizeof(uint32_t)));
        CREATE_HIP(hipMemsetAsync(h->d_pg_tickets, 0, (groups + 1) * sizeof(uint32_t), h->stream));
        CREATE_HIP(hipMalloc(&h->d_pg_groups, (size_t)2 * amc::PG_PARITY_WORDS * sizeof(amc::xs_word)));   // group rows, by the parity of the estimator step
        CREATE_HIP(hipMalloc(&h->d_theta_ring, (size_t)2 * AMC_MAX_LEARN * sizeof(double)));
        CREATE_HIP(hipMemsetAsync(h->d_theta_ring, 0, (size_t)2 * AMC_MAX_LEARN * sizeof(double), h->stream));
        CREATE_HIP(hipMalloc(&h->d_pg_tail, sizeof(amc::PgTail)));
    }
    CREATE_HIP(hipEventCreate(&h->ev0));
    CREATE_HIP(hipEventCreate(&h->ev1));
    CREATE_HIP(hipEventCreateWithFlags(&h->ev_params, hipEventDisableTiming));
    CREATE_HIP(hipHostMalloc((void**)&h->h_params, (size_t)AMC_MAX_NP * AMC_MAX_MOVES * sizeof(double), 0));
#undef CREATE_HIP
    rc = push_params(h, cfg->sigma, cfg->weight);
    if (rc != AMC_OK) return bail(rc);
    if (h->n_classes > 1) {            // the moves' classes: a row of the parameter table (amc_kernels.h PT_CLASS)
        double cls[AMC_MAX_MOVES];
        for (int k = 0; k < AMC_MAX_MOVES; ++k) cls[k] = (double)h->class_of_move[k];
        if (hipMemcpy(h->d_ptab + amc::PT_CLASS * AMC_MAX_MOVES, cls, sizeof(cls), hipMemcpyHostToDevice) != hipSuccess)
            return bail(fail(AMC_ERR_HIP, "amc_create_mixed_model: copying the class table failed"));
    }
    if (h->use_rtc) {
        // compile the smallest kernel now so that a malformed expression fails HERE, with the compiler's message
        hipFunction_t fn = nullptr;
        rc = rtc_function(h, "amc::energy_kernel<" + std::to_string(h->potential) + ">", &fn);
        if (rc != AMC_OK) return bail(rc);
    }
    if (h->f32) {
        hipError_t e64 = hipMalloc(&h->d_x64, (size_t)h->M_pad * sizeof(double));
        if (e64 != hipSuccess) return bail(fail(AMC_ERR_OOM, "amc_create: %s", hipGetErrorString(e64)));
    }
    *out = h;
    return AMC_OK;
}

int amc_create(const amc_config* cfg, amc_handle** out) { return create_impl(cfg, ModelSpec(), out); }

int amc_create_custom(const amc_config* cfg, const char* potential_expr, amc_handle** out)
{
    if (!potential_expr) return fail(AMC_ERR_BAD_ARG, "amc_create_custom: potential_expr is NULL");
    ModelSpec spec;
    spec.potential = given(potential_expr);
    return create_impl(cfg, spec, out);
}

// The one path of the creators of run-time compiled models (class_checks: model_spec's, for the entry that takes arrays; the other
// arguments as model_spec's).  The potential is the script's, or the built-in's own expression where the script names
// cfg->potential -- compiled at run time it is the built-in bit for bit; with Float32 state the double well subtracts a Float32 one,
// as Julia's `(x^2 - 1)^2` does --, and the handle is made from the caller's config as an AMC_POTENTIAL_CUSTOM one (a 0.1 caller's
// struct is shorter).
static int create_model(const char* who, bool class_checks, const amc_config* cfg, const char* potential_expr, const char* reward_expr,
                        const char* scale_expr, int n_params, int n_classes, const int* class_of_move, const char* const* sample_exprs,
                        const char* const* logq_exprs, const char* const* dlogq_exprs, const char* const* perform_exprs,
                        const char* const* invert_exprs, amc_handle** out)
{
    ModelSpec spec;
    AMC_TRY(model_spec(class_checks ? who : nullptr, " (No sample_action! / log_proposal_density is defined)", potential_expr, reward_expr, scale_expr, n_params,
                       n_classes, sample_exprs, logq_exprs, dlogq_exprs, perform_exprs, invert_exprs, &spec));
    if (!potential_expr) {
        const bool f32 = cfg->struct_size == sizeof(amc_config) && cfg->state_dtype == AMC_DTYPE_F32;
        if (cfg->potential == AMC_POTENTIAL_HARMONIC) spec.potential = "x*x";
        else if (cfg->potential == AMC_POTENTIAL_DOUBLE_WELL) spec.potential = f32 ? "(x*x - 1.0f)*(x*x - 1.0f)" : "(x*x - 1.0)*(x*x - 1.0)";
        else return fail(AMC_ERR_BAD_ARG, "%s: potential_expr is NULL and cfg->potential names no built-in", who);
    }
    if (class_of_move) spec.class_of_move.assign(class_of_move, class_of_move + cfg->n_moves);
    amc_config c2;
    std::memset(&c2, 0, sizeof(c2));
    std::memcpy(&c2, cfg, cfg->struct_size < sizeof(c2) ? (cfg->struct_size >= 4 ? cfg->struct_size : 4) : sizeof(c2));
    c2.potential = AMC_POTENTIAL_CUSTOM;
    return create_impl(&c2, spec, out);
}

int amc_create_model(const amc_config* cfg, const char* potential_expr, const char* reward_expr, amc_handle** out)
{
    if (!cfg) return fail(AMC_ERR_BAD_ARG, "amc_create_model: NULL argument");
    // (a built-in potential with a custom reward: the built-in's own expression, compiled at run time)
    return create_model("amc_create_model", false, cfg, potential_expr, reward_expr, nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out);
}

int amc_create_policy_model(const amc_config* cfg, const char* potential_expr, const char* reward_expr, const char* scale_expr,
                            amc_handle** out)
{
    if (!cfg) return fail(AMC_ERR_BAD_ARG, "amc_create_policy_model: NULL argument");
    if (!scale_expr) return amc_create_model(cfg, potential_expr, reward_expr, out);
    return create_model("amc_create_policy_model", false, cfg, potential_expr, reward_expr, scale_expr, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out);
}

int amc_create_proposal_model(const amc_config* cfg, const char* potential_expr, const char* reward_expr, const char* sample_expr,
                              const char* logq_expr, const char* dlogq_expr, amc_handle** out)
{
    return amc_create_action_model(cfg, potential_expr, reward_expr, sample_expr, logq_expr, dlogq_expr, nullptr, nullptr, out);
}

int amc_create_vector_policy_model(const amc_config* cfg, int n_params, const char* potential_expr, const char* reward_expr,
                            const char* sample_expr, const char* logq_expr, const char* const* dlogq_exprs, const char* perform_expr,
                            const char* invert_expr, amc_handle** out)
{
    if (!cfg) return fail(AMC_ERR_BAD_ARG, "amc_create_vector_policy_model: NULL argument");
    if (n_params < 1 || n_params > AMC_MAX_NP)
        return fail(AMC_ERR_BAD_ARG, "amc_create_vector_policy_model: n_params must be in [1, %d]", AMC_MAX_NP);
    if (!sample_expr || !logq_expr)
        return fail(AMC_ERR_BAD_ARG, "amc_create_vector_policy_model: sample_expr and logq_expr are both required (No sample_action! / log_proposal_density is defined)");
    if (dlogq_exprs)
        for (int p = 0; p < n_params; ++p)
            if (!dlogq_exprs[p]) return fail(AMC_ERR_BAD_ARG, "amc_create_vector_policy_model: dlogq_exprs[%d] is NULL (one expression per parameter, or none at all)", p);
    return create_model("amc_create_vector_policy_model", false, cfg, potential_expr, reward_expr, nullptr, n_params, 1, nullptr, &sample_expr, &logq_expr,
                        dlogq_exprs, &perform_expr, &invert_expr, out);
}

int amc_create_action_model(const amc_config* cfg, const char* potential_expr, const char* reward_expr, const char* sample_expr,
                            const char* logq_expr, const char* dlogq_expr, const char* perform_expr, const char* invert_expr,
                            amc_handle** out)
{
    if (!cfg) return fail(AMC_ERR_BAD_ARG, "amc_create_proposal_model: NULL argument");
    if (!sample_expr || !logq_expr)
        return fail(AMC_ERR_BAD_ARG, "amc_create_proposal_model: sample_expr and logq_expr are both required (No sample_action! / log_proposal_density is defined)");
    return create_model("amc_create_proposal_model", false, cfg, potential_expr, reward_expr, nullptr, 1, 1, nullptr, &sample_expr, &logq_expr, &dlogq_expr,
                        &perform_expr, &invert_expr, out);
}

int amc_create_mixed_model(const amc_config* cfg, int n_classes, const int* class_of_move, const char* potential_expr,
                           const char* reward_expr, const char* const* sample_exprs, const char* const* logq_exprs,
                           const char* const* dlogq_exprs, const char* const* perform_exprs, const char* const* invert_exprs,
                           amc_handle** out)
{
    if (!cfg || !class_of_move || !sample_exprs || !logq_exprs) return fail(AMC_ERR_BAD_ARG, "amc_create_mixed_model: NULL argument");
    if (n_classes < 1 || n_classes > AMC_MAX_CLASSES)
        return fail(AMC_ERR_BAD_ARG, "amc_create_mixed_model: n_classes must be in [1, %d]", AMC_MAX_CLASSES);
    if (cfg->n_moves < 1 || cfg->n_moves > AMC_MAX_MOVES) return fail(AMC_ERR_BAD_ARG, "amc_create_mixed_model: n_moves must be in [1, %d]", AMC_MAX_MOVES);
    for (int k = 0; k < cfg->n_moves; ++k)
        if (class_of_move[k] < 0 || class_of_move[k] >= n_classes)
            return fail(AMC_ERR_BAD_ARG, "amc_create_mixed_model: class_of_move[%d] = %d is no class", k, class_of_move[k]);
    return create_model("amc_create_mixed_model", true, cfg, potential_expr, reward_expr, nullptr, 1, n_classes, class_of_move, sample_exprs,
                        logq_exprs, dlogq_exprs, perform_exprs, invert_exprs, out);
}

int amc_model_check(int n_params, int n_classes, const char* potential_expr, const char* reward_expr, const char* const* sample_exprs,
                    const char* const* logq_exprs, const char* const* dlogq_exprs, const char* const* perform_exprs,
                    const char* const* invert_exprs, char* log, int log_capacity)
{
    if (log && log_capacity > 0) log[0] = 0;
    if (!sample_exprs || !logq_exprs) return fail(AMC_ERR_BAD_ARG, "amc_model_check: NULL argument");
    if (n_classes < 1 || n_classes > AMC_MAX_CLASSES) return fail(AMC_ERR_BAD_ARG, "amc_model_check: n_classes must be in [1, %d]", AMC_MAX_CLASSES);
    if (n_params < 1 || n_params > AMC_MAX_NP || (n_params > 1 && n_classes > 1))
        return fail(AMC_ERR_BAD_ARG, "amc_model_check: n_params must be in [1, %d], and 1 for a pool of several classes", AMC_MAX_NP);
    ModelSpec spec;
    int rc = model_spec("amc_model_check", "", potential_expr ? potential_expr : "x*x", reward_expr, nullptr, n_params, n_classes, sample_exprs, logq_exprs,
                        dlogq_exprs, perform_exprs, invert_exprs, &spec);
    if (rc != AMC_OK) return rc;
    // several parameters: dlogq_exprs holds the P partials of the one class (all or none); several classes: one entry per class, NULL entries allowed
    if (n_params > 1 && dlogq_exprs)
        for (int q = 0; q < n_params; ++q)
            if (!dlogq_exprs[q]) return fail(AMC_ERR_BAD_ARG, "amc_model_check: dlogq_exprs[%d] is NULL (one expression per parameter, or none at all)", q);
    rc = validate_potential_expr(spec.potential.c_str());
    if (rc == AMC_OK && !spec.reward.empty()) rc = validate_potential_expr(spec.reward.c_str(), "custom reward", "delta");
    if (rc == AMC_OK) rc = validate_classes(spec);
    if (rc != AMC_OK) return rc;
    const AmcKnobs knobs = amc_knobs();
    spec.f32 = knobs.model_check_f32;
    // the estimator kernel is the one that uses every expression (sample, logq, its derivative, perform / invert, reward); with
    // AMC_RTC_CACHE_DIR the code object lands in a file that llvm-objdump reads (tools/rtc_isa.py)
    const RtcCode* code = nullptr;
    std::string text;
    const std::string inst = knobs.model_check_inst.empty() ? "amc::pg_estimate_kernel<2,1,false,0,0,false>" : knobs.model_check_inst;
    rc = rtc_compile(spec, inst, AMC_BUILD_ARCH, knobs, &code, &text);
    if (log && log_capacity > 0) {
        std::strncpy(log, text.c_str(), (size_t)log_capacity - 1);
        log[log_capacity - 1] = 0;
    }
    return rc;
}

int amc_destroy(amc_handle* h)
{
    if (!h) return AMC_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    comm_release(h);
    for (hipModule_t m : h->rtc_mods) (void)hipModuleUnload(m);
    (void)hipFree(h->d_gd_acc);
    (void)hipFree(h->d_status);
    (void)hipFree(h->d_pg_tickets);
    (void)hipFree(h->d_pg_groups);
    (void)hipFree(h->d_theta_ring);
    (void)hipFree(h->d_pg_tail);
    (void)hipFree(h->d_x);
    (void)hipFree(h->d_x64);
    (void)hipFree(h->d_beta);
    (void)hipFree(h->d_acc);
    (void)hipFree(h->d_tot);
    (void)hipFree(h->d_acc16);
    (void)hipFree(h->d_tot16);
    (void)hipFree(h->d_acc_hi);
    (void)hipFree(h->d_tot_hi);
    (void)hipFree(h->d_acc_base);
    (void)hipFree(h->d_tot_base);
    (void)hipFree(h->d_log);
    (void)hipFree(h->d_ptab);
    (void)hipFree(h->d_pick);
    (void)hipFree(h->d_totals);
    (void)hipFree(h->d_acc_slots);
    (void)hipFree(h->d_partials);
    for (int i = 0; i < RED_TICKETS; ++i) {
        RedTicket& t = h->red[i];
        if (t.h_rows) (void)hipHostFree(t.h_rows);
        if (t.h_ratio) (void)hipHostFree(t.h_ratio);
        (void)hipFree(t.d_ratio_acc);
        if (t.h_ratio_acc) (void)hipHostFree(t.h_ratio_acc);
        if (t.ev) (void)hipEventDestroy(t.ev);
    }
    (void)hipFree(h->d_out);
    if (h->h_pg_out) (void)hipHostFree(h->h_pg_out);
    for (int i = 0; i < amc::AMC_MAX_SLICES - 1; ++i) {
        if (h->slice_stream[i]) { (void)hipStreamSynchronize(h->slice_stream[i]); (void)hipStreamDestroy(h->slice_stream[i]); }
        if (h->slice_join[i]) (void)hipEventDestroy(h->slice_join[i]);
    }
    if (h->slice_fork) (void)hipEventDestroy(h->slice_fork);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev_params) (void)hipEventDestroy(h->ev_params);
    (void)hipFree(h->d_hist);
    ladder_release(h->lad);
    anneal_release(h->ann);
    corr_release(h->corr);
    bins_release(h->ehist);
    bins_release(h->emom);
    chain_stats_release(h->cstat);
    blocks_release(h->blocks);
    if (h->h_params) (void)hipHostFree(h->h_params);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return AMC_OK;
}

}  // extern "C"
