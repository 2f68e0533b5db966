/*
 * amc.h -- C ABI of libamc.so: the MI355X (gfx950) many-chain Metropolis engine.
 *
 * This is the drop-in boundary for ONE path of Arianna.jl
 * (TheDisorderedOrganization/MonteCarlo @ 2025-03-02): the sweep
 *     make_step!(::Simulation, ::Metropolis)        src/metropolis.jl:302-309
 *       -> mc_sweep!                                src/metropolis.jl:203-212
 *         -> mc_step!                               src/metropolis.jl:176-190
 * over M independent particle_1d chains (example/particle_1d/particle_1d.jl:9-70),
 * the callback reductions that read its state (callback_energy particle_1d.jl:68-70,
 * callback_acceptance metropolis.jl:319-321) and the policy-gradient estimator that
 * sits on it (src/PolicyGuided/estimator.jl:111-134, gradients.jl:93-121).
 *
 * The reference is pure Julia and has no FFI of its own; these entry points are
 * what an `AriannaAlgorithm` subtype (src/algorithms.jl:6-37) binds with `ccall`
 * -- see INTEGRATION.md for the Julia stub -- and what montecarlo_amd/ (the
 * Python mirror of that plugin interface) binds with ctypes.
 *
 * Conventions
 *  - plain C types only; the caller owns every host buffer for the duration of
 *    the call; the library owns all device memory.
 *  - every function returns 0 on success or a negative amc_status; the message
 *    is available from amc_last_error() (thread-local).  Nothing throws.
 *  - one handle <-> one device <-> one HIP stream.  Calls on one handle must be
 *    serialised by the caller.  amc_sweep / amc_init_uniform are asynchronous on
 *    the handle's stream; every call that returns data to the host synchronises.
 *  - there is NO CPU fallback: without a usable gfx950 device amc_create fails.
 */
#ifndef AMC_H
#define AMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The entry points declared here are the library's WHOLE dynamic symbol table: libamc.so is built with hidden visibility
 * (montecarlo_amd/csrc/Makefile) and these declarations carry the default one. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define AMC_VERSION_MAJOR 0
#define AMC_VERSION_MINOR 1
#define AMC_MAX_MOVES 64        /* K: moves in a pool (Move, metropolis.jl:140-147) */
#define AMC_MAX_LEARN 8         /* learnable moves per estimator call */
#define AMC_MAX_QBATCH 256      /* q_batch_size * n_learn must stay < 4096 (12-bit draw id) */
#define AMC_MAX_RUNGS 64        /* R: rungs of a temperature ladder (amc_set_ladder) */

typedef enum amc_status {
    AMC_OK = 0,
    AMC_ERR_BAD_ARG = -1,
    AMC_ERR_HIP = -2,
    AMC_ERR_OOM = -3,
    AMC_ERR_NO_DEVICE = -4,
    AMC_ERR_STATE = -5,
    AMC_ERR_COMM = -6,
    /* a script-defined model could not be BUILT for a reason that is not the script's: the run-time compiler died (a fatal
     * error inside LLVM), did not come back in time, or could not be started.  It runs in a child process that never touches
     * the GPU (amc_rtc_worker, beside libamc.so), so the caller's process is alive and amc_last_error() holds the compiler's
     * last words.  An expression that does not compile is the caller's error: AMC_ERR_BAD_ARG with the first diagnostic.
     * Reference convention: raise, do not die -- error("No ... is defined"), src/metropolis.jl:35. */
    AMC_ERR_COMPILE = -7
} amc_status;

/* potential(x): free function the driver script defines
 * (harmonic_oscillator/MC_harmonic_oscillator.jl:4).  A user Julia closure cannot
 * cross a C ABI, so the engine offers the particle_1d family by id. */
typedef enum amc_potential {
    AMC_POTENTIAL_HARMONIC = 0,     /* x*x            (reference) */
    AMC_POTENTIAL_DOUBLE_WELL = 1,  /* (x*x - 1)^2    (BASELINE config 3) */
    AMC_POTENTIAL_CUSTOM = 2        /* a C expression in x, compiled for gfx950 at run time: amc_create_custom */
} amc_potential;

/* Particle{T} / Displacement{T} are generic in T <: AbstractFloat (particle_1d.jl:9,26).  Float64 is what the reference's
 * scripts use and the type every parity figure is quoted on.  AMC_DTYPE_F32 keeps x, beta, e, delta and the log-target
 * difference in Float32 exactly where Julia's promotion rules would: the policy parameters, the
 * normal variate, log_proposal_density, the acceptance probability and the uniforms stay Float64.  The state then crosses
 * HBM as 4 + 4 bytes per update; the kernels are the same sources, compiled at run time (hiprtc) on first use.  Host
 * buffers of this ABI stay `double` whatever the state type: uploads are rounded to Float32 (round to nearest even),
 * downloads are exact.  Script-defined expressions then see x (and delta) as `float`: arithmetic against double literals
 * promotes as in Julia (2.0*x is Float64), overloaded calls take their float form (sqrt(x), fabs(x), fma(x, x, c) are
 * Float32 operations, as Julia's would be), and the value is converted to Float32 where the model stores it. */
typedef enum amc_state_dtype {
    AMC_DTYPE_F64 = 0,
    AMC_DTYPE_F32 = 1
} amc_state_dtype;

/* The policy parameters have a type of their own (amc_config.param_dtype, an amc_state_dtype value).  AMC_DTYPE_F64 is the above:
 * ComponentArray(sigma = 0.1) next to any Particle{T}.  AMC_DTYPE_F32 is the all-Float32 model, ComponentArray(sigma = 0.1f0) next
 * to Particle(0f0, 2f0): sigma, the normal variate (randn(rng, Float32)), delta = sigma * z and the
 * quotient -(delta^2) / (2 sigma^2) of log_proposal_density are Float32; log(2 pi sigma^2) / 2 (2 pi is a Float64 in Julia), the
 * acceptance probability and the uniforms stay Float64.  It requires state_dtype = AMC_DTYPE_F32 (a Float32 sigma under Float64
 * state promotes back to the Float64 arithmetic: AMC_ERR_BAD_ARG rather than an alias).  cfg->sigma[k], and what amc_set_parameters
 * takes, must then be Float32 VALUES -- a parameter is checked, not rounded: AMC_ERR_BAD_ARG if (double)(float)s != s -- in
 * [AMC_SIGMA_F32_MIN, AMC_SIGMA_F32_MAX] = [2^-63, 2^60]: sigma^2 >= 2^-126 keeps sigma * sigma and 2 sigma^2 normal Float32s, and
 * sigma <= 2^60 keeps delta^2 = (sigma z)^2 <= 2^120 * 73.5 finite for every normal variate (|z| <= 8.58), so the acceptance
 * argument is never NaN; 2 sigma^2 <= 2^121 does not overflow.
 * Such a handle sweeps (every amc_sweep* / amc_reduce* / counter / state entry; amc_create and amc_create_custom); the estimator
 * (amc_pg_*, amc_pgmc_*: AMC_ERR_STATE) and the creators of script-defined policies (amc_create_policy_model with a scale,
 * amc_create_proposal_model, _action_model, _vector_policy_model, _mixed_model: AMC_ERR_BAD_ARG) refuse it. */
#define AMC_SIGMA_F32_MIN 0x1.0p-63
#define AMC_SIGMA_F32_MAX 0x1.0p+60

typedef struct amc_handle amc_handle;

/* Mirrors Metropolis(chains; pool, sweepstep=1, seed=1, ...) metropolis.jl:288-291
 * plus what the chains/pool objects carry on the Julia side. */
typedef struct amc_config {
    uint32_t struct_size;        /* = sizeof(amc_config); ABI guard */
    int32_t  device;             /* HIP device ordinal */
    int64_t  n_chains;           /* chains held by THIS handle (local shard) */
    int64_t  chain_offset;       /* global id of local chain 0; must be even */
    int64_t  n_chains_global;    /* total chains over all shards (>= offset + n_chains) */
    int32_t  potential;          /* amc_potential */
    int32_t  n_moves;            /* K = length(pool) */
    double   beta;               /* Particle.beta (particle_1d.jl:11), shared by all chains
                                    unless amc_upload_state passes a per-chain array */
    const double *sigma;         /* [K] StandardGaussian parameters sigma_k (particle_1d.jl:50),
                                    each in [1e-100, 1e100]; param_dtype = AMC_DTYPE_F32: Float32 values in
                                    [AMC_SIGMA_F32_MIN, AMC_SIGMA_F32_MAX] */
    const double *weight;        /* [K] Move.weight (metropolis.jl:144); must sum to ~1 */
    uint64_t seed;               /* Metropolis.seed (metropolis.jl:235) -> Philox key */
    int32_t  sweepstep;          /* Metropolis.sweepstep (metropolis.jl:234), >= 1 */
    int32_t  per_chain_counters; /* 1: keep Move.accepted_calls/total_calls per chain (needed
                                    for amc_download_counters; forced on when K > 1).
                                    0 (K = 1 only): keep only the pool-wide accepted total */
    void    *stream;             /* optional hipStream_t to run on; NULL -> library-owned */
    int32_t  state_dtype;        /* amc_state_dtype.  Callers built against the 0.1 layout (struct_size 88, without
                                    this field) get AMC_DTYPE_F64 */
    int32_t  param_dtype;        /* amc_state_dtype of the policy parameters (see above).  0 = AMC_DTYPE_F64: every caller
                                    that wrote the 0 this field ("reserved") used to demand */
} amc_config;
#define AMC_CONFIG_SIZE_V0_1 88u

/* Layout of amc_reduce's output (doubles). */
enum {
    AMC_RED_SUM_E = 0,       /* sum_c e_c                  -> callback_energy = /M      */
    AMC_RED_SUM_X = 1,       /* sum_c x_c                                              */
    AMC_RED_SUM_XX = 2,      /* sum_c x_c^2   (statistic of test/distribution_test.jl:36-37) */
    AMC_RED_COUNT = 3,       /* local chain count as double                             */
    AMC_RED_SUM_RATIO0 = 4,  /* + k: sum_c accepted_ck / total_ck -> callback_acceptance = /M */
    AMC_RED_HEADER = 4
};
/* amc_reduce writes AMC_RED_HEADER + K doubles. */

/* amc_pg_estimate writes 5 doubles per learnable move: GradientData for P = 1
 * (gradients.jl:41-47): j, grad_j, grad_logq_forward, g, n -- SUMS over the local
 * chains x q_batch samples (the `+` fold of gradients.jl:68-76), n as double. */
enum { AMC_GD_J = 0, AMC_GD_GRAD_J = 1, AMC_GD_GRAD_LOGQ = 2, AMC_GD_G = 3, AMC_GD_N = 4,
       AMC_GD_STRIDE = 5 };

const char *amc_last_error(void);
int  amc_version(void);                          /* major*1000 + minor */
int  amc_device_count(int *count);

/* Metropolis(chains; ...) constructor, metropolis.jl:240-267 / :288-291.  Asserts
 * what the reference asserts (weights/parameters well-formed); allocates SoA
 * state x[M] (+ per-chain counters) in HBM.  State starts at x = 0. */
int  amc_create(const amc_config *cfg, amc_handle **out);
int  amc_destroy(amc_handle *h);

/* The reference lets the driver script define `potential(x)` freely (a global Julia function,
 * harmonic_oscillator/MC_harmonic_oscillator.jl:4; docs/src/man/system.md).  amc_create_custom is that hook on
 * the GPU path: cfg->potential = AMC_POTENTIAL_CUSTOM and potential_expr is the body as ONE C expression in the
 * double `x`, e.g. "x*x*x*x - 2.0*x*x + 0.25*x".  The sweep / reduction / estimator kernels are instantiated for
 * it with hiprtc on first use (about 1 s per kernel form, cached per process).  Vocabulary with bit-reproducible
 * results on any IEEE-754 host: + - * / (never contracted into fma), sqrt, fabs, fma, and the engine's own
 * amc_exp / amc_log.  Other device math functions (exp, sin, pow ...) compile too but
 * are only accurate to the device library's ulps.  Allowed characters: printable ASCII except # \ ; { } " ' ` $ @.
 * A malformed expression fails here with the compiler's first diagnostics in amc_last_error().
 * Environment: AMC_RTC_CACHE_DIR=<dir> keeps the compiled code objects on disk (one file per expression and kernel
 * form, keyed by a hash that includes the kernel sources), so later processes skip the compile. */
int  amc_create_custom(const amc_config *cfg, const char *potential_expr, amc_handle **out);
/* The same with the model's `reward(action, system)` (src/PolicyGuided/gradients.jl:20, evaluated at :100 right after
 * perform_action!; particle_1d.jl:42-44 defines delta^2) as a second expression, in `delta` and the NEW position `x`
 * -- what the policy-gradient estimator maximises (E[reward * alpha]).  potential_expr NULL: the built-in potential named
 * by cfg->potential (its own expression, compiled at run time); reward_expr NULL: delta^2. */
int  amc_create_model(const amc_config *cfg, const char *potential_expr, const char *reward_expr, amc_handle **out);
/* The same with a script-defined POLICY of the Gaussian-displacement family.  The reference hands `system` to
 * sample_action! and log_proposal_density (src/metropolis.jl:177-182; particle_1d.jl:52-59), so a policy's width may depend
 * on the state: scale_expr is ONE C expression in the CURRENT position `x`, and the proposal is
 *     delta = rand(rng, Normal(0, sigma_k * scale(x)))
 *     log_proposal_density = -(delta)^2 / (2 (sigma_k scale(x))^2) - log(2 pi (sigma_k scale(x))^2) / 2
 * with the forward density evaluated at the old state and the backward density at the new one, as mc_step! does
 * (metropolis.jl:178,182): the proposal ratio no longer cancels and enters the acceptance.  scale_expr NULL: scale = 1,
 * the reference's StandardGaussian (amc_create_model).  The policy-gradient estimator then takes the forward density
 * and its sigma-derivative at the old state and the backward ones at the new state (gradients.jl:97,102,106). */
int  amc_create_policy_model(const amc_config *cfg, const char *potential_expr, const char *reward_expr,
                             const char *scale_expr, amc_handle **out);
/* A script-defined PROPOSAL in full: the model's own sample_action! and log_proposal_density (the generic functions of
 * src/metropolis.jl:35-62; example/particle_1d/particle_1d.jl:52-59 are the particle_1d model's methods), each as ONE C
 * expression, compiled at run time like the potential:
 *     sample_expr   delta = f(z, x, sigma): the displacement from one standard normal variate `z` (the engine's
 *                   Box-Muller draw of the step), the current position `x` and the move's parameter `sigma`
 *                   -- e.g. a drifted (Langevin) proposal "-sigma*sigma*x + sigma*z"
 *     logq_expr     log q(delta | x, sigma), the log-density of what sample_expr returns (normalisation included where it
 *                   depends on x or sigma); mc_step! evaluates it for the forward action at the old state and for the
 *                   inverted action (-delta) at the new state (metropolis.jl:178,182)
 *     dlogq_expr    d logq / d sigma -- what the reference obtains from ForwardDiff / Enzyme / Zygote
 *                   (src/PolicyGuided/gradients.jl:28-33) and never asks its user for.  OPTIONAL: NULL and the engine
 *                   differentiates logq_expr itself -- the expression evaluated over dual numbers (forward mode,
 *                   ForwardDiff's rules: montecarlo_amd/csrc/amc_dual.h), the parameters carrying the partials, delta and x
 *                   constants, exactly ForwardDiff.gradient(p -> log_proposal_density(action, policy, p, system), parameters).
 *                   Given, the expression is used as given (a hand-derived form may order its operations differently:
 *                   equal to a few ulp, tests/test_autodiff.py).
 * Variables: z, x, sigma, delta; vocabulary as for amc_create_custom.  potential_expr NULL: cfg->potential's built-in.
 * Float32 state (cfg->state_dtype): x and delta are floats in the expressions -- C's usual arithmetic conversions restate Julia's
 * promotion rules for the same text; parameters, z and the densities stay Float64. */
int  amc_create_proposal_model(const amc_config *cfg, const char *potential_expr, const char *reward_expr,
                               const char *sample_expr, const char *logq_expr, const char *dlogq_expr, amc_handle **out);
/* The same for a policy with SEVERAL parameters: Move.parameters is an array in the reference (src/metropolis.jl:140-147),
 * GradientData keeps grad j and grad logq_forward as arrays of its shape and g as their P x P outer product
 * (src/PolicyGuided/gradients.jl:41-61,104-108), and the natural-gradient optimisers invert g + eps I
 * (learning.jl:103-104,130-133,159-163).  n_params = P in [1, AMC_MAX_PARAMS]; the expressions see the move's parameters as
 * theta0 .. theta{P-1} (`sigma` stays a name of theta0), dlogq_exprs[p] = d logq / d theta_p (all P of them, or NULL: logq_expr is
 * differentiated by the engine, see amc_create_proposal_model), perform_expr / invert_expr as in amc_create_action_model (both NULL: the displacement).  E.g. a Gaussian
 * with a learnable drift, delta = theta0 + theta1 z:
 *     sample "theta0 + theta1*z"     logq "-((delta-theta0)*(delta-theta0))/(2.0*theta1*theta1) - amc_log(theta1)"
 *     dlogq  { "(delta-theta0)/(theta1*theta1)", "((delta-theta0)*(delta-theta0))/(theta1*theta1*theta1) - 1.0/theta1" }
 * Parameter 0 of every move starts at cfg->sigma[k] (which must pass its range check), the others at 0: set the vector
 * with amc_set_parameters(h, k, theta, P) -- any finite values.  With P > 1:
 *   - every output that holds GradientData has AMC_GD_STRIDE_P(P) = 2 + 2P + P^2 doubles (records) per learnable move:
 *     j, grad j [P], grad logq_forward [P], g [P][P] row by row, n  (P = 1: the five of AMC_GD_*);
 *   - the estimator takes one launch per learnable move (1 + 2P + P(P+1)/2 reproducible column sums: g is symmetric), the
 *     accumulate and update steps ride in that launch's own tail on a single shard (between shards: records, all-reduce, one tiny
 *     launch each); with ONE learnable move amc_pgmc_steps takes the whole time step -- sweep, estimator, learning step -- in one
 *     launch, with several the sweep rides in the first move's launch (amc_pg_route says which route a call gets);
 *   - a learning step that leaves a parameter non-finite, or meets a singular g + eps I, is not applied (as for P = 1:
 *     reported by amc_pg_get_accumulated);
 *   - inv(g + eps I) is Gauss-Jordan elimination with partial pivoting (amc::pg_inv_small) where Julia calls LAPACK's
 *     getrf / getri: equal up to rounding (a few ulp times the condition number), exactly 1 / a for P = 1. */
#define AMC_MAX_PARAMS 4
#define AMC_GD_STRIDE_P(P) (2 + 2 * (P) + (P) * (P))
int  amc_create_vector_policy_model(const amc_config *cfg, int n_params, const char *potential_expr, const char *reward_expr,
                                    const char *sample_expr, const char *logq_expr, const char *const *dlogq_exprs,
                                    const char *perform_expr, const char *invert_expr, amc_handle **out);
/* P and AMC_GD_STRIDE_P(P) of a handle (either pointer may be NULL). */
int  amc_n_params(amc_handle *h, int *n_params, int *gd_stride);
/* Pools that MIX policy and action types.  In the reference every Move carries its own `action` and `policy`
 * (src/metropolis.jl:140-162; the pool's moves need only agree across CHAINS, :249-260), and sample_action! /
 * log_proposal_density / perform_action! / invert_action! dispatch on their types.  Here: up to AMC_MAX_CLASSES expression sets
 * ("classes"), class_of_move[k] in [0, n_classes) names the one move k uses; sample_exprs / logq_exprs have one entry per class,
 * dlogq_exprs one per class with NULL entries, or a NULL array, for the classes whose logq the engine differentiates itself
 * (amc_create_proposal_model), perform_exprs / invert_exprs one per class with NULL entries (or NULL arrays) for the displacement.  One parameter (sigma) per move.  E.g. a plain Gaussian displacement beside a Langevin
 * (drifted) proposal and a scaling action in one pool.  Everything else -- counters, step log, callbacks, estimator, learning
 * steps, sharding -- is that of amc_create_action_model. */
#define AMC_MAX_CLASSES 4
int  amc_create_mixed_model(const amc_config *cfg, int n_classes, const int *class_of_move, const char *potential_expr,
                            const char *reward_expr, const char *const *sample_exprs, const char *const *logq_exprs,
                            const char *const *dlogq_exprs, const char *const *perform_exprs, const char *const *invert_exprs,
                            amc_handle **out);
/* Compile-only check of a script-defined model, amc_potential_check's sibling (no GPU needed): builds the estimator kernel -- the
 * one that uses every expression: sample, logq, its derivative (given, or by forward-mode differentiation where dlogq is NULL),
 * perform / invert, reward -- for the library's target ISA.  n_classes = 1: sample_exprs[0] ... describe the one policy and, with
 * n_params = P > 1, dlogq_exprs holds its P partials (or is NULL); n_classes > 1: one entry per class as for amc_create_mixed_model
 * (n_params = 1).  potential_expr NULL: the harmonic x*x.  Returns AMC_OK, AMC_ERR_BAD_ARG with the first diagnostic when the
 * text does not compile (an operator the dual numbers lack shows up here), AMC_ERR_COMPILE when the compiler itself failed. */
int  amc_model_check(int n_params, int n_classes, const char *potential_expr, const char *reward_expr,
                     const char *const *sample_exprs, const char *const *logq_exprs, const char *const *dlogq_exprs,
                     const char *const *perform_exprs, const char *const *invert_exprs, char *log, int log_capacity);
/* How an estimator call over n_learn learnable moves of this handle would run.  Returns
 *     2   (asked with `fused` != 0 only) the whole time step -- sweep + estimator [+ update] -- is ONE launch (amc_pgmc_steps)
 *     1   one estimator launch takes every learnable move, as the reference's make_step!(::PolicyGradientEstimator) loops over all
 *         of them in one step whatever their policy types (estimator.jl:111-134) -- (more than four learnable moves of the built-in
 *         policy with a q_batch that calls for the kernel's flushing form: launches of four moves, the form a CU holds more blocks of)
 *     0   one launch per learnable move
 *    < 0  an amc_status.
 * Only a pool of several classes can answer 0 for one-parameter policies: its several-move kernel form is asked of the run-time
 * compiler on first use, and where the compiler fails on it (hipcc 7.2 meets a back-end error on some pools; the compiler runs in a
 * child process, AMC_ERR_COMPILE) the calls fall back to the one-move form -- same samples, same sums, same bits.  `why` (may be
 * NULL) then receives the compiler's last words.  The call itself triggers that first build, so it doubles as a warm-up.
 * Policies with several parameters: 0, except n_learn == 1 (1, or 2 for the fused step on a single shard). */
int  amc_pg_route(amc_handle *h, int n_learn, int q_batch, int fused, char *why, int why_capacity);
/* The same with a script-defined ACTION -- the reference's Action interface (src/metropolis.jl:15-119; the displacement's
 * methods are example/particle_1d/particle_1d.jl:30-40) for a one-parameter action on the position:
 *     perform_expr   the position after perform_action!(system, action), from `x` and `delta`      (displacement: x + delta)
 *     invert_expr    the parameter of the inverted action, invert_action!(action, system), from `delta` and the NEW
 *                    position `x`                                                                 (displacement: -delta)
 * A rejected step re-applies the inverted action (perform_action_cached!, metropolis.jl:119,187).  Both NULL: the
 * displacement (= amc_create_proposal_model); they come together.  log_proposal_density must be the density of the move
 * in state space where the action is not a translation (e.g. scaling x -> x exp(delta): logq carries -log|x exp(delta)|). */
int  amc_create_action_model(const amc_config *cfg, const char *potential_expr, const char *reward_expr,
                             const char *sample_expr, const char *logq_expr, const char *dlogq_expr,
                             const char *perform_expr, const char *invert_expr, amc_handle **out);
/* Compile-only check of a potential expression (needs no GPU); the compiler log, if any, is copied to log. */
int  amc_potential_check(const char *potential_expr, char *log, int log_capacity);

/* initialise(): upload chains[c].x (and optionally a per-chain beta array,
 * Particle.beta).  e is not uploaded: e == potential(x) by construction
 * (particle_1d.jl:13-15) and is recomputed on device. */
int  amc_upload_state(amc_handle *h, const double *x, const double *beta_or_null);
/* Synthetic ensemble: x_c = lo + (hi-lo)*u_c, u from the INIT Philox stream keyed by
 * the GLOBAL chain id (MC_harmonic_oscillator.jl:13 uses 4rand(rng)-2). */
int  amc_init_uniform(amc_handle *h, double lo, double hi);
/* finalise(): chains[c].x / chains[c].e back to the host (either may be NULL). */
int  amc_download_state(amc_handle *h, double *x, double *e);
/* pools[c][k].accepted_calls / total_calls, move-major [k*n_chains + c].  Int (Int64) in the reference
 * (src/metropolis.jl:145-146).  The device counts in 32-bit arrays and CARRIES: before the launch that would count step 2^32
 * every counter is added into a 64-bit base of its own and the arrays restart at zero (once per 2^32 counted steps; what the
 * calls below return is base + array), so a run counts on -- up to 2^52 steps, the range in which callback_acceptance's
 * Int / Int is exact.  After the first carry the acceptance ratios are formed by a pass over arrays and bases instead of
 * inside the fold of the step log.  The pool-wide count of a K = 1 handle without per-chain counters is 64-bit.
 * (Storage detail, invisible here: with K <= 4 a counter is two u16 halves in separate arrays, and the high halves take
 * part in the folds only from the call that would count step 65 536 on; environment AMC_WIDE_COUNTERS=1 keeps plain u32.) */
int  amc_download_counters(amc_handle *h, int64_t *accepted, int64_t *total);
/* Pool-wide sums over local chains: accepted[k], total[k] (exact integers). */
int  amc_counter_totals(amc_handle *h, int64_t *accepted, int64_t *total);

/* Resume: restore pools[c][k].accepted_calls / total_calls ([k*n_chains + c], total may be NULL for
 * K = 1) on a handle with per-chain counters -- the total_calls of a chain must add up to the same number of steps on
 * every chain, as they do in the reference, where every chain takes the same steps (mc_sweep!, metropolis.jl:205-210); or, for a K = 1 handle without them, the pool-wide
 * accepted total and the number of counted steps.  Together with amc_upload_state, amc_set_step,
 * amc_set_estimator_step and amc_set_parameters this restores a run exactly (the reference's
 * StoreBackups, src/algorithms.jl:264-303, is write-only and saves neither RNG state nor counters). */
int  amc_upload_counters(amc_handle *h, const int64_t *accepted, const int64_t *total);
int  amc_set_counter_totals(amc_handle *h, const int64_t *accepted, uint64_t steps_counted);

/* Device-side stand-ins for the per-chain text trajectories (StoreTrajectories, src/algorithms.jl:154-210;
 * the pooled positions are what test/distribution_test.jl:33-37 and the density plot consume):
 * histogram over n_bins half-open bins of [lo, hi), bin = floor((x - lo) * (n_bins / (hi - lo)));
 * counts has n_bins + 3 entries: bins, then x < lo, x >= hi, NaN.  Local shard only (sum across shards). */
int  amc_histogram(amc_handle *h, double lo, double hi, int n_bins, uint64_t *counts);
/* The same histogram ACCUMULATED on the device over many calls (a density sampled every few sweeps): _accumulate queues one
 * pass over the positions as of this point of the stream and returns at once; _fetch waits, returns the running counts
 * (layout as above) and, with reset != 0, zeroes them.  The first _accumulate fixes (lo, hi, n_bins) until the next reset. */
int  amc_histogram_accumulate(amc_handle *h, double lo, double hi, int n_bins);
int  amc_histogram_fetch(amc_handle *h, uint64_t *counts, int n_bins, int reset);
/* x[first + i*stride], i < count: a strided binary snapshot of this shard. */
int  amc_download_strided(amc_handle *h, int64_t first, int64_t stride, int64_t count, double *x);

/* n x make_step!(simulation, ::Metropolis) (metropolis.jl:302-309): each is
 * `sweepstep` mc_step!s per chain.  The n*sweepstep steps run fused in one launch
 * (state stays in registers); results are identical to n separate calls. */
int  amc_sweep(amc_handle *h, int64_t n_sweeps);
/* n x make_step!(simulation, ::Metropolis) as n LAUNCHES of one sweep each, queued by one host call: what run!'s time loop issues
 * when every t is observed by nobody in between but the caller wants the state to make its HBM round trip per sweep (the
 * benchmark's definition of a step; src/simulation.jl:184-191 calls make_step! once per t).  Identical to n calls of
 * amc_sweep(h, 1), minus n - 1 crossings of the language boundary. */
int  amc_sweep_launches(amc_handle *h, int64_t n_launches);
/* Replica exchange (parallel tempering) along a temperature ladder -- an EXTENSION: the reference has no such algorithm of its own,
 * a user writes it as an AriannaAlgorithm whose make_step! walks simulation.chains (the plugin protocol, src/algorithms.jl:6-37);
 * here the chains live on the device, so the engine provides the cross-chain move.
 * amc_set_ladder(h, R), 2 <= R <= AMC_MAX_RUNGS: ladder l is the R consecutive GLOBAL chain ids [l R, (l + 1) R), the rung of chain c is
 * c mod R, its beta whatever the per-chain beta array holds (typically beta[c] = ladder[c mod R]).  Needs a per-chain beta array
 * (amc_upload_state with beta: AMC_ERR_STATE otherwise) and n_chains_global, chain_offset, n_chains all multiples of R -- no ladder
 * straddles a shard -- (AMC_ERR_BAD_ARG naming the number).  R may be odd.  R = 0 clears the ladder.  Setting a ladder zeroes the gap
 * counters (the gaps of another ladder are other gaps); amc_upload_state leaves them alone, like the Move counters.  The exchange step
 * index t_x is a property of the HANDLE, not of the ladder: it starts at 0 at creation and survives clearing and re-setting the ladder,
 * so the parity and the draws of the next exchange step continue where the last one stopped (amc_set_exchange_step changes it).
 * A handle without a ladder behaves as it always did.
 * Exchange step n (n = the exchange step index t_x, a counter of its own beside amc_get_step / amc_get_estimator_step): in every ladder
 * the gaps r -- chains a = l R + r and b = a + 1 -- with r mod 2 == n mod 2 and r + 1 < R are attempted,
 *     delta = (((-e_b) beta_a) + ((-e_a) beta_b)) - (((-e_a) beta_a) + ((-e_b) beta_b)),   e = potential(x)   (particle_1d.jl:20-22)
 *     accept iff min(1, exp(delta)) > u  (strict; NaN rejects),  u = rand(Float64) of draw (id = global id of chain a, t = n, draw 0, stream 3)
 * and an accepted swap exchanges x_a and x_b; beta, the Move counters and the step log stay with the rung.  Float32 state: e, beta and
 * delta are Float32, exp and u Float64.  amc_exchange leaves the MH step index, the estimator step index and every Move counter alone.
 * All asynchronous on the handle's stream except where a result comes back. */
int  amc_set_ladder(amc_handle *h, int n_rungs);
int  amc_exchange(amc_handle *h, int64_t n_steps);
/* n_rounds x [ amc_sweep(h, sweeps_per_round); amc_exchange(h, 1) ] queued by one host call; identical to the separate calls. */
int  amc_sweep_exchange(amc_handle *h, int64_t n_rounds, int64_t sweeps_per_round);
/* Per gap r in [0, R - 1): swaps accepted / attempted over the local ladders since the ladder was set (or what
 * amc_set_exchange_counters restored): exact integers, add across shards.  Synchronises. */
int  amc_exchange_counters(amc_handle *h, int64_t *accepted, int64_t *attempted);
int  amc_set_exchange_counters(amc_handle *h, const int64_t *accepted, const int64_t *attempted);
int  amc_get_exchange_step(amc_handle *h, uint64_t *t);
int  amc_set_exchange_step(amc_handle *h, uint64_t t);
/* amc_histogram by rung: counts[r * (n_bins + 3) + i], r < R, layout of a row as amc_histogram's.  Local shard only (sum across shards). */
int  amc_histogram_rungs(amc_handle *h, double lo, double hi, int n_bins, uint64_t *counts);
/* Per-rung reproducible sums ("Reproducible sums" below): for rung r and column c the kind-R sum over the
 * local ladders l of ONE chain's summand, chain l R + r -- double(potential(x)) (the potential in the state type), double(x),
 * fl(double(x) * double(x)).  The level of a sum is fixed by the largest summand of its own rung and column; NaN / +-Inf flag their own
 * record.  Integer sums: independent of lanes, blocks, grid and shards -- the shards' records merged and rounded once are the bits of a
 * single handle holding all ladders; every rung has n_chains / R local summands.
 * records[(r * 3 + c) * AMC_XSUM_WORDS ...], r < R, c = 0 sum e, 1 sum x, 2 sum x^2 over the LOCAL ladders; columns: AMC_REDUCE_* bits,
 * a column not asked for is an all-zero record.  Synchronises.  Merge across shards with amc_xsum_merge / amc_allreduce_xsum.
 * Runs on the handle's stream behind whatever is queued; leaves the step indices, the step log, every counter and the reductions in
 * flight alone.  AMC_ERR_STATE without a ladder; AMC_ERR_BAD_ARG for columns == 0 or bits outside AMC_REDUCE_ALL. */
int  amc_reduce_rungs_exact(amc_handle *h, int columns, double *records);
/* Bridge sums (DESIGN.md section 3.13 "Bridge sums"): what free-energy differences along the ladder, log(Z_(r+1) / Z_r), and the heat
 * capacity per rung are formed from -- per rung the reproducible sums of the energy, its square and the neighbour-reweighting factors,
 * accumulated on the device over many snapshots.  For chain i = l R + r, e = potential(x_i) in the state type T, beta the per-chain array:
 *   E  double(e)                                       EE  fl(double(e) * double(e))
 *   WF exp(double((-e) * (beta_(i+1) - beta_i)))       MF  min(1, WF)      for r + 1 < R      (products and differences in T)
 *   WB exp(double((-e) * (beta_(i-1) - beta_i)))       MB  min(1, WB)      for r >= 1         (a NaN stays a NaN)
 * A record is the kind-R sum of one slot's summands over the local ladders and over every accumulated snapshot, its level fixed by the
 * largest summand of that rung and column; NaN / +-Inf flag the one record they belong to (MF and MB lie in [0, 1]: no Inf flag).
 * Integer sums: the same bits on any grid, in any order of the snapshots, and -- merged with amc_xsum_merge / amc_allreduce_xsum -- on
 * any split into shards of whole ladders.
 * amc_bridge_accumulate queues one snapshot of the state behind whatever is on the stream and returns at once (a pending learning
 * step is taken first, as before an exchange step).  The first call after a reset fixes `columns`, AMC_BRIDGE_* bits, until the next
 * reset -- amc_bridge_fetch with reset != 0, amc_set_bridge, amc_set_ladder --; another mask is AMC_ERR_STATE.
 * amc_bridge_fetch waits and returns records[(r * 6 + c) * AMC_XSUM_WORDS ...], r < R, c in the order E, EE, WF, WB, MF, MB, of the
 * LOCAL shard and the number of snapshots in them; reset != 0 zeroes both.  All-zero records: WF and MF at rung R - 1, WB and MB at rung
 * 0, every column outside the mask, and everything when nothing has been accumulated (n_snapshots = 0).
 * amc_set_bridge restores an accumulator (checkpoints); NULL or n_snapshots = 0 clears it.  The mask is read off the records: a column
 * is in it exactly when its records are not all zero (a slot that had a summand is never an all-zero record).
 * amc_set_ladder clears the accumulator on every call that succeeds.  A respacing that is taken (status 0) zeroes the records and the
 * count on the device, as it zeroes the gap counters -- sums taken at other beta belong to another ladder --; the mask stays fixed.
 * amc_upload_state and amc_tune_rung_sigma leave it alone.  None of the three touches the step indices, the step log, any counter, the
 * reductions in flight, the labels or the widths per rung and their window; a handle that never accumulates allocates nothing for it.
 * AMC_ERR_STATE without a ladder; AMC_ERR_BAD_ARG for columns == 0 or bits outside AMC_BRIDGE_ALL, and for records amc_set_bridge
 * cannot have been given by amc_bridge_fetch.  A refused call leaves the handle as it was. */
enum { AMC_BRIDGE_E = 1, AMC_BRIDGE_EE = 2, AMC_BRIDGE_WF = 4, AMC_BRIDGE_WB = 8, AMC_BRIDGE_MF = 16, AMC_BRIDGE_MB = 32, AMC_BRIDGE_ALL = 63 };
int  amc_bridge_accumulate(amc_handle *h, int columns);
int  amc_bridge_fetch(amc_handle *h, double *records, uint64_t *n_snapshots, int reset);
int  amc_set_bridge(amc_handle *h, const double *records_or_null, uint64_t n_snapshots);
/* Walker tracking (DESIGN.md section 3.13 "Walker tracking"): which replica sits at which rung, round trips and flow.  One label byte
 * per local chain, lab = w | (d << 6): w in [0, R) the walker id -- the rung the replica sat at when tracking was turned on --, d the end
 * it last visited: 0 none yet, 1 "up" (last at rung 0), 2 "down" (last at rung R - 1); d = 3 never occurs.
 * amc_set_tracking(h, 1) needs a ladder (AMC_ERR_STATE otherwise), sets lab[l R + r] = r | (d0(r) << 6) with d0(0) = 1, d0(R - 1) = 2 and 0
 * elsewhere, and zeroes the two trip counters; amc_set_tracking(h, 0) frees the labels.  amc_set_ladder turns tracking off on every
 * call that succeeds, n_rungs = 0 included (another ladder has other walkers); amc_upload_state leaves the labels alone.
 * With tracking on an exchange step (amc_exchange, amc_sweep_exchange) decides as it always does and an accepted swap of gap r
 * exchanges the two labels along with x; then, if r == 0, the label now at rung 0 counts a round trip when its d is 2 and gets d = 1,
 * and if r + 1 == R - 1 the label now at rung R - 1 counts an up trip when its d is 1 and gets d = 2.  x, e, every counter and every
 * step index of a tracked handle equal those of an untracked one bit for bit; a handle without tracking launches what it always did.
 * Every entry below except amc_set_tracking returns AMC_ERR_STATE while tracking is off.
 * amc_download_labels / amc_upload_labels: n_chains bytes of the local shard; both synchronise.  amc_upload_labels checks on the host,
 * before anything reaches the device, and refuses with AMC_ERR_BAD_ARG naming the first offending chain: w >= R, d == 3, a label at
 * rung 0 whose d is not 1, a label at rung R - 1 whose d is not 2, a ladder whose walker ids are no permutation of 0 .. R - 1.
 * amc_flow_rungs: counts[r * 3 + d] = local chains at rung r whose label has direction d (sum across shards; the flow fraction is
 * f(r) = counts[r][1] / (counts[r][1] + counts[r][2])).  amc_tracking_counters: round trips (a "down" label arrived at rung 0) and up
 * trips (an "up" label arrived at rung R - 1) over the local ladders since tracking was turned on (or what amc_set_tracking_counters
 * restored): exact integers, add across shards.  Both run on the handle's stream behind whatever is queued, synchronise and change nothing. */
int  amc_set_tracking(amc_handle *h, int on);
int  amc_download_labels(amc_handle *h, uint8_t *labels);
int  amc_upload_labels(amc_handle *h, const uint8_t *labels);
int  amc_flow_rungs(amc_handle *h, uint64_t *counts);
int  amc_tracking_counters(amc_handle *h, int64_t *round_trips, int64_t *up_trips);
int  amc_set_tracking_counters(amc_handle *h, int64_t round_trips, int64_t up_trips);
/* Proposal widths per rung (DESIGN.md section 3.13 "Widths per rung"): sigma[k * R + r] is the width of move k for the chains at rung r
 * (r = global chain id mod R), n = K * R <= AMC_MAX_MOVES.  While a table is set, every sweep steps chain c with the widths of its rung:
 * bit for bit chain c of a handle without a table whose pool has sigma_k = sigma[k * R + (c mod R)].  The move pick (the pool's weights),
 * the step log and the Move counters know nothing of rungs; exchange steps, tracking, rung sums and histograms are untouched: sigma stays
 * with the rung, like beta.  amc_set_parameters / amc_get_parameters go on writing and reading the pool's shared sigma_k, which the sweeps
 * then do not use.  sigma == NULL or n == 0 clears the table (never an error); amc_set_ladder clears it on every call that succeeds.
 * Stream-ordered behind what is queued (a pending learning step is taken first); does not synchronise.
 * AMC_ERR_STATE: no ladder, per_chain_counters = 0, param_dtype = AMC_DTYPE_F32, a handle made by amc_create_policy_model /
 * _proposal_model / _vector_policy_model / _mixed_model (script-defined policies, classes, actions).  AMC_ERR_BAD_ARG naming the entry:
 * K * R > AMC_MAX_MOVES, n != K * R, a sigma that is not finite in [1e-100, 1e100]; the handle stays as it was.  While a table is set every
 * estimator entry (amc_pg_*, amc_pgmc_steps*) returns AMC_ERR_STATE before any launch: the estimator learns one sigma per move.
 * amc_get_rung_sigma: the table as it was given (AMC_ERR_STATE when none is set). */
int  amc_set_rung_sigma(amc_handle *h, const double *sigma, int n);
int  amc_get_rung_sigma(amc_handle *h, double *sigma, int n);
/* Move.accepted_calls / total_calls summed over the local ladders per (move, rung): accepted[k * R + r], total[k * R + r], exact 64-bit
 * integers formed on the device (add across shards); their sum over r is amc_counter_totals.  Needs a ladder and per-chain counters
 * (AMC_ERR_STATE otherwise), with or without widths per rung.  Folds pending rows of the step log first, synchronises, changes nothing.
 * Either output may be NULL. */
int  amc_rung_counter_totals(amc_handle *h, int64_t *accepted, int64_t *total);
/* Respacing the ladder (DESIGN.md section 3.13 "Respacing", which holds the rule operation by operation): new beta values for the
 * interior rungs, computed on the device from the swap counts per gap (AMC_RESPACE_ACCEPTANCE: equalise the rejection rate) or from the
 * flow counts per rung (AMC_RESPACE_FLOW: the feedback-optimised ladder, rung density ~ sqrt(df/dbeta / dbeta)); gamma in (0, 1] damps the
 * move of every rung, eps in [0, 1) is the floor of a gap's weight as a share of the mean weight.  The end rungs keep their bits.
 * counts == NULL: the handle's own device counters -- right only when the handle holds every ladder; nothing synchronises and nothing is
 * read back.  Otherwise counts are the GLOBAL counts, summed over all shards by the caller, and travel with the launch:
 * AMC_RESPACE_ACCEPTANCE attempted[R - 1] then accepted[R - 1], AMC_RESPACE_FLOW n[R][3] as amc_flow_rungs gives them; every shard given
 * the same counts computes the same ladder.  Stream-ordered behind what is queued (a pending learning step is taken first); does not
 * synchronise.  The ladder at hand is read from the first local ladder.
 * Status (amc_respace_status, of the last call): 0 respaced; 1 no weight to spread (W is not positive and finite); 2 a count the rule
 * divides by is zero (a gap never attempted; a rung without a label that has visited an end); 3 the ladder at hand is not finite or not
 * strictly monotone; 4 the new ladder is not.  Status 0 writes beta_c = T(out[c mod R]) for every local chain (a Float32 ladder is
 * rounded once, here), zeroes the gap counters and, with tracking on, sets the labels back to r | (d0(r) << 6) and zeroes both trip
 * counters: a new ladder restarts the measurement.  Any other status leaves the handle exactly as it was.  x, the step indices, the step
 * log, the Move counters and the widths per rung are left alone in every case.
 * AMC_ERR_STATE: no ladder; rule AMC_RESPACE_FLOW with counts == NULL while tracking is off.  AMC_ERR_BAD_ARG naming the argument: an
 * unknown rule, gamma outside (0, 1], eps outside [0, 1) (NaN included), counts with more accepted than attempted swaps.
 * amc_respace_status: the status of the last respacing (0 before the first) and the number of status-0 respacings since the ladder was
 * set (amc_set_ladder resets it, amc_upload_state leaves it alone; amc_set_respaced restores it on resume).  amc_get_ladder: the R beta
 * values of the first local ladder as the device holds them.  Both synchronise. */
#define AMC_RESPACE_ACCEPTANCE 1
#define AMC_RESPACE_FLOW 2
int  amc_respace_ladder(amc_handle *h, int rule, double gamma, double eps, const uint64_t *counts);
int  amc_respace_status(amc_handle *h, int *status, int64_t *n_respaced);
int  amc_set_respaced(amc_handle *h, int64_t n_respaced);
int  amc_get_ladder(amc_handle *h, double *betas);
/* Tuning the widths per rung (DESIGN.md section 3.13 "Tuning the widths", which holds the rule operation by operation): every entry
 * e = k * R + r of the table moves by one damped fixed-point step sigma <- sigma * a / target, a = accepted / total calls of move k at
 * rung r over the current WINDOW, limited to a factor of two per call and clamped to [sigma_lo, sigma_hi]; gamma in (0, 1] damps the step,
 * an entry with fewer than min_calls calls in the window keeps its width.  Computed on the device from the table the device holds; the
 * four derived rows of a tuned entry are rewritten as amc_set_rung_sigma forms them, so the sweeps that follow are those of a pool with
 * the new widths, bit for bit.  Stream-ordered behind what is queued (a pending learning step is taken first); with counts == NULL
 * nothing synchronises and nothing is read back.
 * The window: per (move, rung) the Move counters' totals (amc_rung_counter_totals) minus their value at the start of the window, a
 * device array that exists from its first use (zero then: the first window is "since the counters began").  A tuning ends the window and
 * starts the next in every case; amc_rung_window_restart does so without tuning.  amc_set_ladder drops the base; nothing else touches
 * it, and the Move counters themselves are never written.  A cell whose counter is below its base (counters uploaded behind it) is
 * inconsistent: status 2, not an error.
 * counts == NULL: the handle's own window -- right only when the handle holds every ladder.  Otherwise counts is the GLOBAL window, summed
 * over all shards by the caller, accepted[K * R] then total[K * R], and travels with the launch: every shard given the same counts
 * computes the same table.
 * Status per entry (amc_tune_status, of the last call): 0 tuned; 1 fewer than min_calls calls, sigma keeps its bits; 2 inconsistent
 * window, sigma keeps its bits; 3 tuned and clamped.  n_tuned counts the calls that tuned at least one entry (status 0 or 3) since the
 * table was set: amc_set_rung_sigma and amc_set_ladder reset the record, amc_set_tuned restores the count on resume.
 * Once a tuning has been queued amc_get_rung_sigma returns the table as the device holds it (and synchronises).
 * AMC_ERR_STATE: no ladder, per_chain_counters = 0, no table set.  AMC_ERR_BAD_ARG naming the argument: target outside (0, 1), gamma
 * outside (0, 1], min_calls < 1, sigma_lo or sigma_hi outside [1e-100, 1e100] or sigma_lo > sigma_hi (NaN included), counts that are
 * negative or hold more accepted calls than calls.  A refused call leaves the handle as it was.
 * amc_rung_window_counts: the local window per cell, -1 in both outputs for an inconsistent cell; synchronises, changes nothing.
 * amc_rung_window_base / amc_set_rung_window_base: the base itself, for exact resume.  The amc_rung_window_* entries need a ladder,
 * per-chain counters and K * R <= AMC_MAX_MOVES (AMC_ERR_STATE otherwise), with or without a table. */
int  amc_tune_rung_sigma(amc_handle *h, double target, double gamma, int64_t min_calls, double sigma_lo, double sigma_hi, const int64_t *counts);
int  amc_tune_status(amc_handle *h, int *st, int n, int64_t *n_tuned);
int  amc_set_tuned(amc_handle *h, int64_t n_tuned);
int  amc_rung_window_counts(amc_handle *h, int64_t *accepted, int64_t *total);
int  amc_rung_window_restart(amc_handle *h);
int  amc_rung_window_base(amc_handle *h, int64_t *accepted, int64_t *total);
int  amc_set_rung_window_base(amc_handle *h, const int64_t *accepted, const int64_t *total);

/* Population annealing (which holds the step operation by operation): amc_anneal moves the handle's shared
 * beta to beta_new and resamples the WHOLE ensemble in proportion to exp(-(beta_new - beta) e_c): with a_c = double((-e_c) delta),
 * delta = T(beta_new) - T(beta) in the state's type, and a_max their maximum, chain c has the integer weight
 * W_c = floor(2^AMC_ANNEAL_WEIGHT_BITS amc_exp(a_c - a_max)); T_w = sum W_c and the inclusive prefix C_c are exact 64-bit integers;
 * one Philox draw per step (id 0, t = the annealing step index, draw 0, stream 4) gives the offset U = mulhi64(w.x | w.y << 32, T_w);
 * the parent of child slot j is the unique i with C_(i-1) M <= j T_w + U < C_i M (systematic resampling, 128-bit integers), and
 * x'_j = x_parent(j).  Chain i gets floor(M W_i / T_w) or ceil(M W_i / T_w) children, a chain with W = 0 none; beta_new == beta (no NaN
 * energies) is the identity.  Everything is an integer or a maximum: the same bits on any grid.
 * Asynchronous, stream-ordered behind what is queued (a pending learning step is taken first, as before an exchange step); every
 * launch queued afterwards uses beta_new.  The Move counters, the step log, the MH and estimator step indices and reductions in flight
 * stay with the slot.  The second position buffer and the step's scratch are allocated at the first call: a handle that never anneals
 * has none.  Every step appends one record of AMC_ANNEAL_RECORD_WORDS 64-bit words to a log on the device: status, the bits of beta
 * before, the bits of beta_new, the bits of a_max, T_w, U, n_parents (chains with at least one child), max_children.  Status 0: resampled;
 * 1: every a_c was NaN; 2: a_max = +Inf; 3: a_max = -Inf (no chain has a weight).  With a status other than 0 the positions are left
 * alone and T_w, U, n_parents, max_children read 0 (a_max reads a NaN with status 1); beta moves and the step counts in every case.
 * log(Z(beta_new) / Z(beta)) ~ a_max + log T_w - log M - AMC_ANNEAL_WEIGHT_BITS log 2, formed by the caller from the record.
 * AMC_ERR_STATE: a per-chain beta array, a ladder, a handle that does not hold the whole ensemble (chain_offset != 0 or
 * n_chains != n_chains_global: resampling across devices is not done), a full log (AMC_ANNEAL_MAX_RECORDS).  AMC_ERR_BAD_ARG: beta_new
 * not finite, n_chains >= 2^33.  A refused call leaves the handle as it was.
 * amc_anneal_fetch: *n = records in the log; with records != NULL the records themselves (capacity in records, AMC_ERR_BAD_ARG when it
 * is below *n), synchronises; reset empties the log.  amc_set_anneal_records puts n records back (resume; NULL or n = 0 empties it).
 * amc_get_anneal_step / amc_set_anneal_step: annealing steps done (the step index of the offset's draw; below 2^48), settable for
 * resume.  amc_get_beta: the shared beta as the launches queued from now on use it; amc_set_beta puts one back without resampling
 * (resume: a fresh handle starts at the beta of its creation; AMC_ERR_BAD_ARG when it is not finite). */
#define AMC_ANNEAL_WEIGHT_BITS 30
#define AMC_ANNEAL_MAX_RECORDS 4096
#define AMC_ANNEAL_RECORD_WORDS 8
int  amc_anneal(amc_handle *h, double beta_new);
int  amc_anneal_fetch(amc_handle *h, uint64_t *records, int capacity, int *n, int reset);
int  amc_set_anneal_records(amc_handle *h, const uint64_t *records, int n);
int  amc_get_anneal_step(amc_handle *h, uint64_t *t);
int  amc_set_anneal_step(amc_handle *h, uint64_t t);
int  amc_get_beta(amc_handle *h, double *beta);
int  amc_set_beta(amc_handle *h, double beta);
/* Choosing the next beta (DESIGN.md section 3.14 "Choosing the next beta", which holds the rule operation by operation):
 * amc_anneal_next_beta finds on the device the largest step from the shared beta towards beta_limit whose reweighting keeps the
 * effective-sample fraction rho = (sum W)^2 / (M sum W^2) at or above `target` (strictly between 0 and 1), by `rounds` (1 .. 16) rounds
 * of AMC_ANNEAL_SEARCH_CANDIDATES candidates over a bracket that starts at [0, T(beta_limit) - T(beta)]: the span is resolved to
 * 8^-rounds of itself.  The weights are those of amc_anneal (the products in the state's type, the same integer W), the sums exact
 * integers: the answer is the same on any grid and bit-exact against a host twin.  *beta_new is what to hand to amc_anneal; it never
 * passes beta_limit and is beta_limit bit for bit when the whole span passes.  The entry changes neither beta nor the positions; it
 * queues 2 rounds + 1 launches behind what is queued and then SYNCHRONISES once to read the answer: beta is a host field that goes into
 * the launch arguments of the sweeps, so the host has to know it.  A pending learning step is taken first.  The energies reuse the
 * word per chain of amc_anneal; a scratch of a few KB is allocated at the first call.
 * diag (optional): AMC_ANNEAL_SEARCH_WORDS words: status, rounds decided, bits of the step chosen, rho at the bracket's low end (1 for
 * a step of 0), bits of the bracket's high end, rho there, bits of the largest and of the smallest -e.  trace (optional):
 * rounds * AMC_ANNEAL_SEARCH_CANDIDATES * 3 words, every candidate's S1 = sum W, S2h = sum (W^2 >> 30), S2l = sum (W^2 & (2^30 - 1)); rounds
 * that were not run read 0.
 * Status AMC_ANNEAL_SEARCH_OK: a step inside the span.  _LIMIT: every candidate passed (or the span is 0, then nothing is launched
 * and diag reads 0 behind the status): *beta_new = beta_limit.  _BELOW_RESOLUTION: every candidate of every round failed, the step is
 * the smallest one resolved, so that a run always advances.  _STALLED: T(beta) + T(step) == T(beta); *beta_new = beta.  _ALL_NAN,
 * _INF, _NO_WEIGHT: no usable weights (every energy a NaN; the largest log-weight of the whole span +Inf; -Inf): *beta_new =
 * beta_limit, and the amc_anneal that follows records its own status and leaves x alone.
 * AMC_ERR_STATE, as amc_anneal: a per-chain beta array, a ladder, a handle that does not hold the whole ensemble.  AMC_ERR_BAD_ARG: a
 * NULL handle or beta_new, beta_limit not finite (or a span that is not finite in the state's type), target outside (0, 1), rounds
 * outside [1, 16], n_chains >= 2^33.  A refused call leaves the handle as it was. */
#define AMC_ANNEAL_SEARCH_CANDIDATES 8
#define AMC_ANNEAL_SEARCH_WORDS 8
#define AMC_ANNEAL_SEARCH_MAX_ROUNDS 16
#define AMC_ANNEAL_SEARCH_OK 0
#define AMC_ANNEAL_SEARCH_LIMIT 1
#define AMC_ANNEAL_SEARCH_BELOW_RESOLUTION 2
#define AMC_ANNEAL_SEARCH_STALLED 3
#define AMC_ANNEAL_SEARCH_ALL_NAN 4
#define AMC_ANNEAL_SEARCH_INF 5
#define AMC_ANNEAL_SEARCH_NO_WEIGHT 6
int  amc_anneal_next_beta(amc_handle *h, double beta_limit, double target, int rounds, double *beta_new, uint64_t *diag, uint64_t *trace);
/* Families, population annealing's own diagnostic: amc_set_anneal_families(h, 1) gives every chain a 32-bit family id, fam[c] = c
 * (n_chains <= 2^32 - 1; calling it again starts the families afresh), and every annealing step from then on gathers the ids along
 * with the positions; (h, 0) frees them.  amc_anneal_family_stats synchronises and returns exact integers: the families that have a
 * member, sum_f n_f^2 and max_f n_f (counted with atomics into a scratch array zeroed per call); rho_t = sum_sq / n_chains is what tells
 * whether the population is large enough.  amc_download_families / amc_upload_families: the ids themselves, for checkpoints; an id
 * >= n_chains is AMC_ERR_BAD_ARG.  All but amc_set_anneal_families need families on (AMC_ERR_STATE).  With families off nothing is
 * allocated or gathered. */
int  amc_set_anneal_families(amc_handle *h, int on);
int  amc_anneal_family_stats(amc_handle *h, uint64_t *n_families, uint64_t *sum_sq, uint64_t *largest);
int  amc_download_families(amc_handle *h, uint32_t *families);
int  amc_upload_families(amc_handle *h, const uint32_t *families);
/* Error bars for population annealing (DESIGN.md section 3.14 "Error bars"): blocks of slots stop being independent at the first
 * resampling (see amc_set_blocks below, which keeps refusing amc_anneal), blocks of FAMILIES do not -- descendants of different
 * ancestors never share a parent.  amc_set_anneal_blocks(h, n_blocks, chunk) sets the partition "block of chain c =
 * (fam[c] div chunk) mod n_blocks", a function of the family id and nothing else: n_blocks = 0 turns it off, otherwise
 * 2 <= n_blocks <= AMC_MAX_JK_BLOCKS; chunk = 0 asks for ceil(n_chains / n_blocks), every block one contiguous range of ancestors.  It
 * needs families on and excludes amc_set_blocks, in either order (AMC_ERR_STATE); every successful call empties the log below, and so do
 * amc_set_anneal_families(h, 0) and amc_set_anneal_families(h, 1), which turn the partition off.
 * While it is set, every amc_anneal appends a BLOCK RECORD of 2 n_blocks 64-bit words to a second log, aligned with the records' log:
 * n_b, the chains of block b before the resampling, then T_b, the sum of W_c over them -- the integer weights the step resamples by, so
 * sum_b T_b = T_w and sum_b n_b = n_chains exactly, on any grid.  With a status other than 0, n_b is still counted and T_b reads 0.  One
 * more launch per step (and one memset); a handle without the partition launches and allocates what it always did.  A full log
 * (AMC_ANNEAL_MAX_RECORDS block records) makes amc_anneal AMC_ERR_STATE.
 * amc_anneal_fetch_blocks: *n = block records in the log, *n_blocks = B; with records == NULL the sizes alone, without waiting and
 * without resetting; otherwise records[(s * 2 + k) * B + b], k = 0: n_b, k = 1: T_b (capacity in block records), synchronises, reset
 * empties this log -- amc_anneal_fetch and its reset do not touch it: a caller drains both in one place to keep them aligned.
 * amc_set_anneal_block_records puts n block records back (resume; n_blocks must be B; NULL or n = 0 empties the log).
 * amc_anneal_block_counts: counts[b] = the n_b of the chains as they stand (one launch; synchronises).
 * All but amc_set_anneal_blocks are AMC_ERR_STATE without the partition.
 * Energy histograms per block of families: while this partition is set (and amc_set_blocks, which excludes it, is not),
 * amc_energy_histogram_accumulate_blocks / _fetch_blocks / amc_set_energy_histogram_blocks (below) work under IT: counts[b][n_bins + 3],
 * ONE group (a ladder is AMC_ERR_STATE), chain c counted in the row of its family's block; LDS cells while n_blocks (n_bins + 3) <= 12288,
 * one global atomic per chain beyond.  The sum over the blocks is the plain histogram cell for cell; *n_snapshots = (sum of all
 * cells) / n_chains, and amc_set_energy_histogram_blocks checks that total instead of every row (a block's share of the chains changes
 * with every resampling).  Turning the partition off, or setting another, folds a standing accumulator of this form into a plain one. */
int  amc_set_anneal_blocks(amc_handle *h, int n_blocks, int64_t chunk);
int  amc_anneal_fetch_blocks(amc_handle *h, uint64_t *records, int capacity, int *n, int *n_blocks, int reset);
int  amc_set_anneal_block_records(amc_handle *h, const uint64_t *records, int n, int n_blocks);
int  amc_anneal_block_counts(amc_handle *h, uint64_t *counts);

/* MH steps done per chain so far (the Philox step index); settable for resume. */
int  amc_get_step(amc_handle *h, uint64_t *t);
int  amc_set_step(amc_handle *h, uint64_t t);
/* estimator make_step! calls done so far (the estimator stream's step index). */
int  amc_get_estimator_step(amc_handle *h, uint64_t *t);
int  amc_set_estimator_step(amc_handle *h, uint64_t t);

/* Reproducible sums.  Everything that crosses chains on this path is a sum -- callback_energy (particle_1d.jl:68-70: mean),
 * callback_acceptance (metropolis.jl:319-321: mean), the GradientData fold (estimator.jl:113-131: reducer(+, ...)) -- and the
 * reference adds Float64s in whatever order its reducer takes.  Here each such sum is defined so that the order of the
 * additions cannot enter the result (montecarlo_amd/csrc/amc_xsum.h): every summand is rounded once to
 * a multiple of a power of two fixed by order-independent facts (the move's sigma; the largest magnitude among the
 * summands), the multiples are added as integers, the total is rounded once to Float64.  The value is therefore the same
 * for every grid, every split of the chains into shards and every number of GPUs, bit for bit.
 * Between shards a partial sum travels as a RECORD of AMC_XSUM_WORDS doubles -- each word an integer below 2^53 in
 * magnitude, so a record survives any f64 channel unchanged; all-zero words are the empty sum.  amc_xsum_merge adds
 * records (into[i] += from[i], i < n_records), amc_xsum_round yields the Float64 of each; both are plain host functions.
 * amc_allreduce_xsum (below, with the communicator) leaves on every shard the merged records of all shards. */
#define AMC_XSUM_WORDS 12
int  amc_xsum_merge(double *into, const double *from, int n_records);
int  amc_xsum_round(const double *records, int n_records, double *out);

/* callback_energy (particle_1d.jl:68-70) / callback_acceptance (metropolis.jl:319-321)
 * / position moments as LOCAL sums (reproducible sums, above): per-block integer partial sums on the device, added up by the
 * host.  out: AMC_RED_HEADER + K doubles.  For one shard these are the final sums; across shards exchange the RECORDS
 * (amc_reduce_end_exact + amc_allreduce_xsum / amc_xsum_merge) -- adding the shards' rounded doubles would make the
 * result depend on the split.  Divide by the global chain count. */
int  amc_reduce(amc_handle *h, double *out);
/* The same reduction split in two so the host need not drain the stream: _begin enqueues the kernels
 * and returns; _end waits for THAT reduction only (sweeps queued after _begin keep
 * running) and returns the values as of _begin.  Up to TWO reductions may be in flight per handle; _end finishes the
 * oldest (a host that writes a callback's row while the next callback's sums are being formed never waits). */
int  amc_reduce_begin(amc_handle *h);
/* n make_step!s followed by amc_reduce_begin of the resulting state.  The sums over x are formed inside the last sweep
 * launch (K <= 4: no second pass over the chains); with per-chain counters the acceptance ratios come from the fold of the
 * step log that follows it. */
int  amc_sweep_reduce_begin(amc_handle *h, int64_t n_sweeps);
int  amc_reduce_end(amc_handle *h, double *out);
/* Which of the sums over x the reductions begun from now on form: callback_energy (particle_1d.jl:68-70) needs sum e alone,
 * the moments of test/distribution_test.jl:36-37 sum x and sum x^2; callback_acceptance (metropolis.jl:319-321) none of the
 * three.  Every sum costs the launch that forms it nine vector instructions per chain pair, so a caller that knows its
 * callbacks names them (default: all).  A sum that was not formed reads NaN (amc_reduce_end) / is an all-zero record
 * (amc_reduce_end_exact). */
enum { AMC_REDUCE_E = 1, AMC_REDUCE_X = 2, AMC_REDUCE_XX = 4, AMC_REDUCE_ALL = 7 };
int  amc_set_reduce_columns(amc_handle *h, int columns);
/* The same as records: (AMC_RED_HEADER + K) * AMC_XSUM_WORDS doubles, column order as above (the count is a record too).
 * steps_counted (may be NULL) receives the MH steps counted per chain at _begin.  On a K = 1 handle without per-chain
 * counters record AMC_RED_SUM_RATIO0 holds the pool-wide accepted TOTAL (an integer); sum_c accepted_c / total_c is its
 * Float64 divided by steps_counted (every chain has the same total_calls). */
int  amc_reduce_end_exact(amc_handle *h, double *records, uint64_t *steps_counted);

/* Move.parameters (shared by all chains, metropolis.jl:252-260): read / replace
 * sigma_k on the device copy, e.g. after learning_step! (update.jl:50-57). */
int  amc_set_parameters(amc_handle *h, int k, const double *p, int n);
int  amc_get_parameters(amc_handle *h, int k, double *p, int n);
/* The same read without making the caller wait for the queued steps (StoreParameters on a schedule, metropolis.jl:433-440,
 * beside device-resident learning steps): _begin queues a copy of sigma_0 .. sigma_{K-1} AS OF THIS POINT of the handle's
 * stream into pinned memory, _end returns them (sigma[K]) once that copy is done -- typically a callback period later, when
 * it long is.  One such read in flight per handle (AMC_ERR_STATE otherwise). */
int  amc_parameters_begin(amc_handle *h);
int  amc_parameters_end(amc_handle *h, double *sigma);
/* ... for a policy with several parameters (amc_create_vector_policy_model): all of them, parameters[k * P + p] of move k;
 * n = K * P.  (amc_parameters_end returns parameter 0 of every move.) */
int  amc_parameters_end_all(amc_handle *h, double *parameters, int n);

/* make_step!(simulation, ::PolicyGradientEstimator) (estimator.jl:111-134) for the
 * moves learn_ids[0..n_learn) (0-based), q_batch samples per chain per move, in the
 * reference's order (move-major, then sample).  Like the reference, every sample
 * leaves x at (x+delta)-delta (gradients.jl:98,103).  out: n_learn*AMC_GD_STRIDE. */
int  amc_pg_estimate(amc_handle *h, int n_learn, const int *learn_ids, int q_batch,
                     double *out);
/* The same fold as records (reproducible sums): n_learn * AMC_GD_STRIDE * AMC_XSUM_WORDS doubles, what shards exchange. */
int  amc_pg_estimate_exact(amc_handle *h, int n_learn, const int *learn_ids, int q_batch,
                           double *records);

/* Device-resident variant of the estimator/update pair (no host round trip per step):
 *   amc_pg_accumulate  = make_step!(::PolicyGradientEstimator): the same kernel as amc_pg_estimate, then
 *                        (if amc_comm_init was called) ONE in-place RCCL all-reduce on the engine's stream that gathers
 *                        the shards' records (4 n_learn AMC_XSUM_WORDS doubles per shard), then the integer merge, one
 *                        rounding and gradients_data[k] += gd on the device (estimator.jl:130): the same bits on every
 *                        shard as on a single shard holding all the chains.
 *   amc_pg_update      = make_step!(::PolicyGradientUpdate) (update.jl:50-57): average, learning_step! for
 *                        P = 1 with optimiser ids below and their two hyper-parameters (eta or delta, eps_id),
 *                        reset, refresh the device copy of sigma and its derived table.  Asynchronous.
 *   amc_pg_get_accumulated  reads the running sums (j, grad_j, grad_logq, g, n) per move (synchronises);
 *                        returns AMC_ERR_STATE if some step produced a sigma outside [1e-100, 1e100]. */
typedef enum amc_optimiser {      /* src/PolicyGuided/learning.jl:16-164 */
    AMC_OPT_STATIC = 0, AMC_OPT_VPG = 1, AMC_OPT_BLPG = 2, AMC_OPT_BLAPG = 3,
    AMC_OPT_NPG = 4, AMC_OPT_ANPG = 5, AMC_OPT_BLANPG = 6
} amc_optimiser;
int  amc_pg_accumulate(amc_handle *h, int n_learn, const int *learn_ids, int q_batch);
int  amc_pg_update(amc_handle *h, int n_learn, const int *learn_ids, const int *optimiser,
                   const double *hyper0, const double *hyper1);
int  amc_pg_get_accumulated(amc_handle *h, int n_learn, const int *learn_ids, double *out);
/* Resume: replace the running sums of the moves learn_ids[] by in[n_learn*AMC_GD_STRIDE] (what amc_pg_get_accumulated
 * returned when the run was checkpointed) -- gradients_data of estimator.jl:84 is part of the state whenever
 * PolicyGradientUpdate is scheduled less often than the estimator. */
int  amc_pg_set_accumulated(amc_handle *h, int n_learn, const int *learn_ids, const double *in);
/* n_steps x [ make_step!(::Metropolis); make_step!(::PolicyGradientEstimator); make_step!(::PolicyGradientUpdate)
 * if do_update ] -- the three algorithms run! calls back to back at one time step (src/simulation.jl:185-190,
 * PGMC_harmonic_oscillator.jl:24-33) -- enqueued by ONE host call: amc_sweep(h, 1), amc_pg_accumulate, amc_pg_update
 * in that order per step, results identical to the separate calls.  For hosts whose per-call cost (Julia ccall,
 * ctypes) would otherwise exceed the ~0.1 ms of device work per step. */
int  amc_pgmc_steps(amc_handle *h, int64_t n_steps, int n_learn, const int *learn_ids, int q_batch,
                    int do_update, const int *optimiser, const double *hyper0, const double *hyper1);
/* The same followed by amc_reduce_begin of the state the last time step leaves -- what callback_energy / callback_acceptance
 * scheduled at that t observe: run! calls them after the three algorithms (src/simulation.jl:185-190;
 * PGMC_harmonic_oscillator.jl:34 lists StoreCallbacks behind them).  When the time step is ONE launch (sweepstep = 1, at most
 * two learnable moves, K <= 4) that launch also forms the sums over x, and the acceptance ratios come from the fold of the
 * step log that follows it: no pass re-reads the chains, and amc_reduce_end returns the values as of this call however
 * many time steps have been queued since. */
int  amc_pgmc_steps_reduce_begin(amc_handle *h, int64_t n_steps, int n_learn, const int *learn_ids, int q_batch,
                                 int do_update, const int *optimiser, const double *hyper0, const double *hyper1);

/* Time correlation: how fast an observable of the chains decorrelates, from ONE time origin and the M chains
 * as independent series.  With a_i = O(x_i) at the mark and O_i = O(x_i) at a later sample, per group g and slot s the reproducible
 * (kind-R) sums of   O: O_i   OO: fl(O_i O_i)   AO: fl(a_i O_i)   -- Float64 products, one multiplication each, no fma -- give
 *   C_g(k) = <a O_k> - <a><O_k>.   O(x) = double(potential_T(x)) for AMC_CORR_E, double(x) for AMC_CORR_X (both conversions exact).
 * Groups: a handle with a ladder has G = R of them, group r the chains l R + r (the series of RUNG r, whatever replicas pass through
 * it); a handle without a ladder has one, g = 0, over all local chains.  Every record's level is fixed by the largest summand of its
 * own group, column and slot; NaN and +-Inf flag their own record and no other.  The same bits on any grid and any split into shards.
 * amc_corr_mark queues one pass behind whatever is on the stream and returns at once (a pending learning step is taken first, as
 * before amc_bridge_accumulate): it stores a_i for every local chain (a buffer of n_chains doubles, allocated at its first use),
 * forgets the samples of an earlier mark and takes sample 0 of the new origin in the same launch -- there O = a, so slot 0 holds
 * sum a, sum a^2, sum a a --, steps[0] = amc_get_step's value.  amc_corr_sample queues one pass over x and the origin into the next
 * free slot s, steps[s] = the MH step index at the call (two samples at one index are allowed); with sliced sweep launches it runs
 * behind their join, where a bridge snapshot runs.
 * amc_corr_fetch waits and returns records[((s * G + g) * AMC_CORR_COLS + c) * AMC_XSUM_WORDS ...] of the LOCAL shard (merge across
 * shards with amc_xsum_merge / amc_allreduce_xsum), s < *n_samples (slot 0 included), and steps[s]; capacity counts the slots the
 * caller's arrays hold; *observable = 0 and *n_samples = 0 when nothing is marked.  Fetch resets nothing.
 * amc_corr_download_origin (n_chains doubles) and amc_set_corr serve checkpoints: amc_set_corr restores a mark with its samples,
 * the records checked as amc_set_bridge checks them -- kind-R records, every word an integer below 2^53 --, steps non-decreasing.
 * amc_corr_clear drops the mark and keeps the memory.
 * The mark is CLEARED by every call that reassigns chain slots -- amc_upload_state, amc_init_uniform, amc_set_ladder, an amc_anneal
 * that was queued (resampling moves positions between slots: a product across it has no meaning) -- and KEPT by amc_exchange (the
 * series is that of rung r, the thing a ladder is meant to shorten), by sweeps, reductions and the estimator, and by
 * amc_respace_ladder and amc_tune_rung_sigma: those two are burn-in tools whose status the host does not know without a
 * synchronisation, so they cannot clear it; a series marked across one of them mixes two ladders / widths and is the caller's to discard.
 * None of these entries touches the step indices, the step log, a counter, reductions in flight, labels, widths or the bridge sums.
 * AMC_ERR_STATE: amc_corr_sample / amc_corr_download_origin without a mark, amc_corr_sample with all AMC_CORR_MAX_LAGS slots used.
 * AMC_ERR_BAD_ARG: an observable outside {E, X}; capacity < *n_samples; amc_set_corr with records amc_corr_fetch cannot have given,
 * n_samples outside [1, AMC_CORR_MAX_LAGS] or decreasing steps.  A refused call leaves the handle as it was. */
enum { AMC_CORR_E = 1, AMC_CORR_X = 2 };
#define AMC_CORR_MAX_LAGS 256
enum { AMC_CORR_O = 0, AMC_CORR_OO = 1, AMC_CORR_AO = 2, AMC_CORR_COLS = 3 };
int  amc_corr_mark(amc_handle *h, int observable);
int  amc_corr_sample(amc_handle *h);
int  amc_corr_fetch(amc_handle *h, double *records, uint64_t *steps, int capacity, int *n_samples, int *observable);
int  amc_corr_download_origin(amc_handle *h, double *origin);
int  amc_set_corr(amc_handle *h, int observable, const double *origin, const double *records, const uint64_t *steps, int n_samples);
int  amc_corr_clear(amc_handle *h);

/* Energy histograms: per group a histogram of the chains' energies, accumulated on the device over as many
 * snapshots as the caller queues -- all that multiple-histogram reweighting (Ferrenberg-Swendsen / WHAM) needs to give <e>, C and
 * log Z BETWEEN the simulated temperatures.  Counts are integers: the same on any grid, in any snapshot order and on any split into
 * shards.  Groups are those of the time correlation: G = R with a ladder (group r = the chains l R + r), G = 1 without one, over all
 * local chains.
 * Binning rule: for chain i, e = potential_T(x_i) in the state type T, read from the state buffer itself (Float32 state: the Float32 x),
 * as the bridge sums form it; v = double(e) (exact); with inv_w = (double)n_bins / (hi - lo) the cell is
 *   n_bins + 2  if v is NaN,   n_bins  if v < lo,   n_bins + 1  if v >= hi,   otherwise  min((int)((v - lo) * inv_w), n_bins - 1)
 * -- Float64 subtraction and product, truncation; the clamp serves (hi - ulp - lo) * inv_w rounding up to n_bins --, amc_histogram's
 * rule applied to e.  Row layout per group is n_bins + 3 cells: counts[g * (n_bins + 3) + cell].  Arguments as amc_histogram takes
 * them: 1 <= n_bins <= 8192, finite lo < hi.
 * amc_energy_histogram_accumulate queues one pass behind whatever is on the stream and returns at once (a pending learning step is
 * taken first, as before amc_bridge_accumulate; with sliced sweep launches it runs behind their join, where a bridge snapshot runs).
 * The first call after a reset allocates and zeroes G * (n_bins + 3) 64-bit counters on the device and fixes (lo, hi, n_bins); a later
 * call with other values is AMC_ERR_STATE.
 * amc_energy_histogram_fetch waits and returns the LOCAL shard's counts (counts add across shards), *n_groups = G, *n_bins, *lo, *hi,
 * and *n_snapshots = (sum of row 0) / (n_chains / G): every chain lands in exactly one of the n_bins + 3 cells of its group, so EVERY
 * row sums to n_snapshots * n_chains / G exactly.  With nothing accumulated it writes no counts, sets *n_bins = 0 and
 * *n_snapshots = 0 and returns AMC_OK.  capacity_cells counts the 64-bit cells the caller's array holds; fewer than G * (n_bins + 3)
 * is AMC_ERR_BAD_ARG.  counts = NULL is allowed: the call then returns the sizes and the bins alone (*n_snapshots = 0), without waiting
 * for the stream, copying or resetting -- what a caller sizes its array by.  reset != 0 frees the accumulator: the next accumulate may
 * bring other bins.
 * amc_set_energy_histogram restores the accumulator (checkpoints): counts = NULL or n_snapshots = 0 clears it; otherwise
 * counts[G * (n_bins + 3)] whose rows do not ALL sum to n_snapshots * n_chains / G are AMC_ERR_BAD_ARG.
 * CLEARED by amc_set_ladder on success (the groups change).  A respacing that is taken (status 0) ZEROES the cells on the device, in
 * stream order, exactly as it zeroes the bridge records -- counts taken at other beta belong to another ladder --; the bins stay
 * fixed, and one that is not taken leaves the cells alone.
 * KEPT by sweeps, exchange steps, reductions, the estimator, tuning, amc_upload_state, amc_init_uniform, amc_set_blocks (a histogram
 * kept per jackknife block is folded into a plain one, see "Energy histograms per jackknife block" below), and -- on purpose -- by amc_anneal and amc_set_beta: a histogram belongs to ONE beta per group,
 * so the caller fetches with reset before beta moves (the Python layer does); the engine cannot know whether the caller is done.
 * None of the three entries touches a step index, the step log, a counter, reductions in flight, labels, widths, the bridge sums or
 * the mark of the time correlation.  A refused call leaves the handle as it was. */
int  amc_energy_histogram_accumulate(amc_handle *h, double lo, double hi, int n_bins);
int  amc_energy_histogram_fetch(amc_handle *h, uint64_t *counts, int64_t capacity_cells, int *n_groups, int *n_bins,
                                double *lo, double *hi, uint64_t *n_snapshots, int reset);
int  amc_set_energy_histogram(amc_handle *h, double lo, double hi, int n_bins, const uint64_t *counts_or_null, uint64_t n_snapshots);

/* Convergence per group: running sums PER CHAIN over time, and their reproducible sums over the chains of a
 * group -- what the Gelman-Rubin potential scale reduction (split or not) and a batch-means tau_int are formed from on the host.
 * Groups and observable are those of the time correlation: G = R with a ladder (group r = the slots l R + r), G = 1 without one;
 * O(x) = double(potential_T(x)) for AMC_CORR_E, double(x) for AMC_CORR_X.
 * Per local chain i and part p in {0, 1} (the two halves of the caller's window) the device keeps S[p][i] and Q[p][i], Float64: a
 * sample into part p does S[p][i] <- S[p][i] + o_i, Q[p][i] <- Q[p][i] + fl(o_i o_i), one rounding per operation, nothing
 * contracted; sequential in time per chain, so independent of grid, slices and shards.
 * amc_chain_stats_accumulate queues one pass behind whatever is on the stream and returns at once (a pending learning step is taken
 * first; with sliced sweep launches it runs behind their join, where a sample of the time correlation runs).  The first call after a
 * clear allocates (once) and zeroes 4 * n_chains doubles and fixes the observable; a later call with another one is AMC_ERR_STATE.
 * amc_chain_stats_fetch queues the sums by group, waits, and returns records[(g * AMC_CHAIN_STATS_COLS + c) * AMC_XSUM_WORDS ...] of
 * the LOCAL shard (kind R; merge across shards with amc_xsum_merge), columns S0, S0S0, Q0, S1, S1S1, Q1, S0S1 with the summands
 * S[0][i], fl(S[0][i] S[0][i]), Q[0][i], the same three of part 1, fl(S[0][i] S[1][i]); n[p] = the samples part p holds, *groups = G.
 * The device divides nothing.  A non-finite summand flags the sums it belongs to, as in the time correlation.  records = NULL returns
 * *groups, *observable and n alone, without waiting.  capacity_words counts the doubles the caller's array holds; fewer than
 * G * AMC_CHAIN_STATS_COLS * AMC_XSUM_WORDS is AMC_ERR_BAD_ARG.  With nothing accumulated it writes no records, sets *observable = 0
 * and n = {0, 0} and returns AMC_OK.  It never changes the accumulators.
 * amc_chain_stats_download (sums[(p * 2 + k) * n_chains + i], k = 0: S, 1: Q; AMC_ERR_STATE with nothing accumulated) and
 * amc_set_chain_stats serve checkpoints; amc_set_chain_stats with sums = NULL, n = NULL or n = {0, 0} clears, as amc_chain_stats_clear does
 * (the memory stays).
 * CLEARED by amc_set_ladder on success, amc_upload_state and amc_init_uniform.  KEPT by sweeps, exchange steps, reductions, the
 * estimator, tuning, amc_set_blocks (the sums are not kept per jackknife block), the bridge sums, the time correlation, the energy
 * histograms -- none of which they touch either -- and, on purpose, by amc_anneal, amc_set_beta and amc_respace_ladder: the caller clears
 * when beta moves (the Python layer refuses such a schedule).
 * AMC_ERR_BAD_ARG: part outside {0, 1}, an observable outside {E, X}.  A refused call leaves the handle as it was. */
enum { AMC_CHAIN_STATS_PARTS = 2, AMC_CHAIN_STATS_COLS = 7 };
int  amc_chain_stats_accumulate(amc_handle *h, int observable, int part);
int  amc_chain_stats_fetch(amc_handle *h, double *records, int capacity_words, uint64_t *n, int *groups, int *observable);   /* n[2] */
int  amc_chain_stats_download(amc_handle *h, double *sums);
int  amc_set_chain_stats(amc_handle *h, int observable, const uint64_t *n, const double *sums);   /* n[2] */
int  amc_chain_stats_clear(amc_handle *h);

/* Jackknife blocks: the bridge sums and the time correlation kept per BLOCK of ladders, so that a
 * delete-one-block jackknife over the B blocks gives an error bar for any function of the sums -- the ladders (the chains, without a
 * ladder) are independent systems, whatever the correlation in time or between the rungs of one ladder.
 * The partition is the pair (B, C), 2 <= B <= AMC_MAX_JK_BLOCKS blocks and a chunk of C >= 1 ladders: the block of a ladder is
 *   b(l) = (l_global div C) mod B,   l_global = chain_offset / G + l_local   (64-bit; G = R of the ladder, 1 without one: a "ladder"
 * is then one chain).  It depends on nothing else -- not the grid, not the launch split, not the split into shards --, and a ladder
 * stays in its block for the whole run: exchange steps move positions within a ladder only.
 * amc_set_blocks(h, n_blocks, chunk): n_blocks = 0 turns the partition off (the state of every handle that never called it); chunk = 0
 * asks for the default, max(1, 256 div G) ladders.  On success it clears the bridge accumulator and forgets the mark of the time
 * correlation, as amc_set_ladder does; amc_set_ladder turns the partition off on every call that succeeds.
 * While a partition is set, amc_bridge_accumulate, amc_corr_mark and amc_corr_sample keep one row per (block, group, column) --
 * allocated at their first use, sized by B and G --, and amc_bridge_fetch / amc_corr_fetch return the merge over the blocks: bit for
 * bit the records of a handle without a partition (kind-R merges are integer additions, their order is immaterial).
 * amc_bridge_fetch_blocks: records[((b * R + r) * 6 + c) * AMC_XSUM_WORDS ...], b < *n_blocks, capacity_blocks >= B; a block without
 * a local ladder gives all-zero records.  amc_corr_fetch_blocks: records[(((b * S + s) * G + g) * AMC_CORR_COLS + c) * AMC_XSUM_WORDS
 * ...] with S = *n_samples <= capacity: B * S * G * 3 records are written, densely (the caller's array holds B * capacity * G * 3), and
 * steps[s] as amc_corr_fetch gives them; with records = NULL or steps = NULL it returns *n_blocks, *n_samples and *observable alone,
 * without waiting for the stream (what a caller sizes its arrays by).  Both are AMC_ERR_STATE without a partition.
 * A respacing that is taken zeroes every block's rows; amc_upload_state, amc_init_uniform forget the blocked mark as they forget the
 * plain one.  amc_anneal is AMC_ERR_STATE while a partition is set: resampling makes copies of one parent share blocks, so the blocks
 * stop being independent and a jackknife over them has no meaning (blocks of FAMILIES stay independent: amc_set_anneal_blocks above is
 * population annealing's own partition; the two cannot be set together, AMC_ERR_STATE).
 * amc_set_bridge_blocks / amc_set_corr_blocks serve checkpoints: they restore the blocked accumulators from what the _blocks fetches
 * gave (n_blocks = B of the partition, set beforehand with the same chunk), every block's records checked as amc_set_bridge /
 * amc_set_corr check theirs and refused the same way; besides, a block without a local ladder must be all zero and the blocks with one
 * share one column mask.  amc_set_bridge_blocks with records = NULL or n_snapshots = 0 clears.  Both are AMC_ERR_STATE without a
 * partition; amc_set_bridge (with records) and amc_set_corr are AMC_ERR_STATE WITH one: the accumulator in use is then the blocked
 * one, merged records cannot be split into its blocks, and taking them into the plain accumulator would drop them silently.
 * Synchronisation: the calls above stay stream-ordered, with one exception -- when a blocked accumulator is (re)allocated the call
 * waits for the stream first: amc_bridge_accumulate at its first use under a partition and after a change of B, amc_corr_mark /
 * amc_corr_sample at the first mark and whenever the samples outgrow the room (slot 16, 32, 64, 128).  A graph capture or a timing
 * loop should take one snapshot and as many samples as it will use beforehand.
 * AMC_ERR_BAD_ARG: n_blocks outside {0} and [2, AMC_MAX_JK_BLOCKS], chunk < 0 or above AMC_MAX_JK_CHUNK, a capacity too small, a NULL argument. */
#define AMC_MAX_JK_BLOCKS 64
#define AMC_MAX_JK_CHUNK (1ll << 40)
int  amc_set_blocks(amc_handle *h, int n_blocks, int64_t chunk);
int  amc_bridge_fetch_blocks(amc_handle *h, double *records, int capacity_blocks, int *n_blocks, uint64_t *n_snapshots, int reset);
int  amc_corr_fetch_blocks(amc_handle *h, double *records, uint64_t *steps, int capacity, int *n_blocks, int *n_samples, int *observable);
int  amc_set_bridge_blocks(amc_handle *h, const double *records, int n_blocks, uint64_t n_snapshots);
int  amc_set_corr_blocks(amc_handle *h, int observable, const double *origin, const double *records, const uint64_t *steps, int n_blocks,
                         int n_samples);

/* Energy histograms per jackknife block (DESIGN.md section 3.17 "Per block"): the energy histograms with a set of rows per block of
 * the partition (amc_set_blocks), so that a delete-one-block jackknife gives an error bar for anything formed from the counts -- the
 * reweighted curve log Z(beta), <e>(beta), C(beta), log g(E), f_r.  The form is opt-in: amc_energy_histogram_accumulate, _fetch and
 * amc_set_energy_histogram do what they always did, and a handle that never calls the entries below allocates and launches what it
 * always did, with or without a partition.
 * amc_energy_histogram_accumulate_blocks queues one pass, as amc_energy_histogram_accumulate does, in which chain i of local ladder l
 * is counted by the same binning rule into the row of (b(l), group): counts[(b * G + g) * (n_bins + 3) + cell].  It needs a partition
 * (AMC_ERR_STATE without one).  The first call after a reset allocates and zeroes B * G * (n_bins + 3) 64-bit counters, fixes
 * (lo, hi, n_bins) and the accumulator's FORM, "blocked under (B, C)"; it waits for the stream at that allocation, as the other
 * blocked accumulators do, and is stream-ordered otherwise.  More than AMC_EHIST_BLK_MAX_CELLS = 2^22 cells (32 MiB) are
 * AMC_ERR_BAD_ARG.  An accumulator's form is fixed while it stands: amc_energy_histogram_accumulate on a blocked accumulator and
 * amc_energy_histogram_accumulate_blocks on a plain one are AMC_ERR_STATE (amc_energy_histogram_fetch with reset frees either), as
 * are other bins.
 * amc_energy_histogram_fetch_blocks waits and returns the LOCAL shard's counts, *n_blocks = B, *n_groups = G, the bins and
 * *n_snapshots; a block without a local ladder is all zero, and every (b, g) row sums to n_snapshots * (local ladders of block b).
 * Blocks are functions of the global ladder index, so shards add cell by cell.  capacity_cells below B * G * (n_bins + 3) is
 * AMC_ERR_BAD_ARG; counts = NULL returns the sizes and the bins alone (*n_snapshots = 0) without waiting; reset != 0 frees the
 * accumulator.  AMC_ERR_STATE unless a blocked accumulator stands.
 * amc_energy_histogram_fetch on a blocked accumulator returns the sum over the blocks (formed on the host behind the copy): the bits
 * a plain accumulator would hold, capacity_cells and the row-sum identity as documented there.
 * amc_set_energy_histogram_blocks restores a blocked accumulator (checkpoints) under the partition set beforehand: n_blocks = B;
 * counts = NULL or n_snapshots = 0 clears; rows that do not ALL sum to n_snapshots * (local ladders of their block) -- an empty
 * block's rows to zero -- are AMC_ERR_BAD_ARG, as are n_blocks != B and too many cells; AMC_ERR_STATE without a partition.
 * amc_set_energy_histogram replaces an accumulator of either form by a plain one.
 * Lifetimes: CLEARED by amc_set_ladder; a respacing that is taken zeroes the rows of EVERY block, one that is not leaves them; a
 * successful amc_set_blocks, with any arguments, FOLDS a standing blocked accumulator into a plain one -- exact integer sums on the
 * device, in stream order: nothing is lost, the bins stay, the form becomes plain --; kept by everything that keeps a plain one.
 * A refused call leaves the handle as it was. */
#define AMC_EHIST_BLK_MAX_CELLS 4194304
int  amc_energy_histogram_accumulate_blocks(amc_handle *h, double lo, double hi, int n_bins);
int  amc_energy_histogram_fetch_blocks(amc_handle *h, uint64_t *counts, int64_t capacity_cells, int *n_blocks, int *n_groups, int *n_bins,
                                       double *lo, double *hi, uint64_t *n_snapshots, int reset);
int  amc_set_energy_histogram_blocks(amc_handle *h, double lo, double hi, int n_bins, const uint64_t *counts_or_null, int n_blocks,
                                     uint64_t n_snapshots);

/* Moments per energy bin (DESIGN.md section 3.17 "Moments per bin"): the energy histograms' pass with, beside the count of every
 * cell, the sums of x, x^2 and [x > 0] over the chains of every bin -- S_gb = sum of o over the samples of group g that fell into bin b.
 * With the density of states g_b of WHAM they give a function of the POSITION at any beta: o_b = sum_g S_gb / sum_g n_gb and
 * <o>(beta) = sum_b g_b exp(-beta E_b) o_b / sum_b g_b exp(-beta E_b).  An accumulator of its own, independent of the energy
 * histograms': both may stand, and a handle that never calls these entries allocates and launches what it always did.
 * Rule per chain, in this order: e = potential_T(x), v = double(e) and the cell by the binning rule above; xd = double(x) (exact).
 * A chain whose cell is a bin but for which !(fabs(xd) <= x_bound) -- NaN included -- goes into a FOURTH tail cell, n_bins + 3
 * ("x beyond x_bound"), and into no sum, so S_gb / n_gb stays a mean over the same samples.  A row has n_bins + 4 count cells; with no
 * chain beyond x_bound the first n_bins + 3 are bit for bit those of amc_energy_histogram_accumulate.  A chain of bin b adds, to the
 * columns that `mask` selects, the integer
 *   AMC_EMOM_X    k = RN(lsb1(xd) * 2^-E_X)
 *   AMC_EMOM_XX   k = RN(lsb1(v) * 2^-E_XX), v = xd * xd rounded to Float64 once (exact for Float32 state)
 *   AMC_EMOM_POS  1 if xd > 0
 * with eb = ilogb(x_bound) + 1, E_X = eb - 32, E_XX = 2 eb - 32, so |k| <= 2^32: kind Q of section 3.8 (lsb1 sets the last bit of
 * the significand: no tie exists), added as signed 64-bit integers -- the same on any grid, in any order, on any split.  A sum cell
 * times its quantum 2^E is the sum.  Layout: counts[g * (n_bins + 4) + cell] (unsigned), sums[(g * C + c) * n_bins + b] (signed),
 * C = popcount(mask), columns in mask-bit order.
 * amc_energy_moments_accumulate queues one pass and returns at once (stream-ordered; a pending learning step is taken first).  The
 * first call after a reset allocates and zeroes the cells and fixes the FORM (lo, hi, n_bins, mask, x_bound); a later call with
 * another form is AMC_ERR_STATE.  AMC_ERR_BAD_ARG: bins as amc_histogram refuses them, mask == 0 or bits outside AMC_EMOM_ALL,
 * x_bound not finite and positive or outside [2^-500, 2^500).  Capacity: a cell holds fewer than 2^31 deposits of at most 2^32
 * quanta; the handle counts the snapshots, and a call that would make n_snapshots * (n_chains / G) reach 2^31 is AMC_ERR_STATE before
 * anything is launched (fetch with reset).  A refused first call leaves nothing allocated.
 * amc_energy_moments_fetch waits and returns the LOCAL shard's cells (they add across shards), the form, *n_cols = C and
 * *n_snapshots = (sum of row 0) / (n_chains / G): every row of counts sums to n_snapshots * n_chains / G.  The capacities count
 * cells; too few are AMC_ERR_BAD_ARG.  counts = sums = NULL returns the sizes and the form alone (*n_snapshots = 0) without waiting;
 * with nothing accumulated it writes no cells, *n_bins = 0, *n_cols = 0, *mask = 0 and returns AMC_OK.  reset != 0 frees the accumulator.
 * amc_set_energy_moments restores it (checkpoints): counts = NULL, sums = NULL or n_snapshots = 0 clears; AMC_ERR_BAD_ARG for rows of
 * counts that do not ALL sum to n_snapshots * n_chains / G, for n_snapshots * n_chains / G >= 2^31, for a sum cell whose magnitude
 * exceeds (count of its bin) * 2^32, and for a POS cell that is negative or exceeds its count.
 * Lifetimes are the energy histograms': CLEARED by amc_set_ladder; ZEROED on the device, in stream order, by a respacing that is taken
 * (one that is not leaves the cells); kept by everything else, amc_anneal and amc_set_beta included.  amc_set_blocks leaves a plain
 * accumulator alone (a blocked one: "Moments per block" below); a form per temperature of a population annealing does not exist. */
enum { AMC_EMOM_X = 1, AMC_EMOM_XX = 2, AMC_EMOM_POS = 4, AMC_EMOM_ALL = 7 };
int  amc_energy_moments_accumulate(amc_handle *h, double lo, double hi, int n_bins, int mask, double x_bound);
int  amc_energy_moments_fetch(amc_handle *h, uint64_t *counts, int64_t *sums, int64_t capacity_counts, int64_t capacity_sums,
                              int *n_groups, int *n_bins, int *n_cols, double *lo, double *hi, int *mask, double *x_bound,
                              uint64_t *n_snapshots, int reset);
int  amc_set_energy_moments(amc_handle *h, double lo, double hi, int n_bins, int mask, double x_bound, const uint64_t *counts_or_null,
                            const int64_t *sums_or_null, uint64_t n_snapshots);

/* Moments per energy bin per jackknife block (DESIGN.md section 3.17 "Moments per block"): the moments per bin with a set of cells per
 * block of the partition (amc_set_blocks), so that a delete-one-block jackknife gives an error bar for <x>(beta), <x^2>(beta) and
 * P(x > 0)(beta).  The form is opt-in: the three entries above do what they always did, and a handle that never calls the entries
 * below allocates and launches what it always did, with or without a partition.
 * amc_energy_moments_accumulate_blocks queues one pass in which chain i of local ladder l is counted and summed by the rule above into
 * the set of block b(l).  It needs a partition (AMC_ERR_STATE without one).  The first call after a reset allocates and zeroes B sets of
 * G * (n_bins + 4) + G * C * n_bins 64-bit words and fixes the form, "blocked under (B, C)"; it waits for the stream at that
 * allocation and is stream-ordered otherwise.  More than AMC_EMOM_BLK_MAX_WORDS = 2^22 words (32 MiB) are AMC_ERR_BAD_ARG, as is all
 * that amc_energy_moments_accumulate refuses.  The capacity rule is the plain one, (n_snapshots + 1) * (n_chains / G) < 2^31: it is
 * conservative per block and keeps a later fold valid.  An accumulator's form is fixed while it stands: the plain entry on a blocked
 * accumulator and the blocked entry on a plain one are AMC_ERR_STATE (amc_energy_moments_fetch with reset frees either), as is
 * another (lo, hi, n_bins, mask, x_bound).  A refused first call leaves nothing allocated.
 * amc_energy_moments_fetch_blocks waits and returns the LOCAL shard's cells, counts[(b * G + g) * (n_bins + 4) + cell] and
 * sums[((b * G + g) * C + c) * n_bins + bin], *n_blocks = B, the form and *n_snapshots (from the first block that has a local
 * ladder); a block without a local ladder is all zero, and every (b, g) row of counts sums to n_snapshots * (local ladders of block b).
 * Shards add cell by cell.  The capacities count cells of all blocks; counts = sums = NULL returns the sizes and the form alone
 * without waiting; reset != 0 frees the accumulator.  AMC_ERR_STATE unless a blocked accumulator stands.
 * amc_energy_moments_fetch on a blocked accumulator returns the sum over its blocks: the integers a plain accumulator would hold.
 * amc_set_energy_moments_blocks restores a blocked accumulator (checkpoints) under the partition set beforehand: n_blocks = B;
 * counts = NULL, sums = NULL or n_snapshots = 0 clears; AMC_ERR_BAD_ARG for rows that do not ALL sum to n_snapshots * (local ladders
 * of their block), for a sum cell its bin's count cannot hold (as amc_set_energy_moments), for n_blocks != B and for too many words;
 * AMC_ERR_STATE without a partition.  amc_set_energy_moments replaces an accumulator of either form by a plain one.
 * Lifetimes: CLEARED by amc_set_ladder; a respacing that is taken zeroes the words of EVERY block; a successful amc_set_blocks, with
 * any arguments, FOLDS a standing blocked accumulator into a plain one -- exact integer sums on the device, in stream order (signed
 * sums add as unsigned words modulo 2^64): nothing is lost, the form becomes plain. */
#define AMC_EMOM_BLK_MAX_WORDS 4194304
int  amc_energy_moments_accumulate_blocks(amc_handle *h, double lo, double hi, int n_bins, int mask, double x_bound);
int  amc_energy_moments_fetch_blocks(amc_handle *h, uint64_t *counts, int64_t *sums, int64_t capacity_counts, int64_t capacity_sums,
                                     int *n_blocks, int *n_groups, int *n_bins, int *n_cols, double *lo, double *hi, int *mask,
                                     double *x_bound, uint64_t *n_snapshots, int reset);
int  amc_set_energy_moments_blocks(amc_handle *h, double lo, double hi, int n_bins, int mask, double x_bound, const uint64_t *counts_or_null,
                                   const int64_t *sums_or_null, int n_blocks, uint64_t n_snapshots);

int  amc_sync(amc_handle *h);
/* hipStream_t the handle launches on (for event timing / graph capture by the host). */
int  amc_get_stream(amc_handle *h, void **stream);
/* HIP-event timing on the handle's stream: begin records an event, end records a second
 * one, waits for it and returns the elapsed device time between the two in ms. */
int  amc_timing_begin(amc_handle *h);
int  amc_timing_end(amc_handle *h, double *elapsed_ms);
/* Optional: records the END event now, without waiting (amc_timing_end then only waits and reads), so that a host can
 * put its own synchronisation point between the two without paying for two blocking waits. */
int  amc_timing_mark(amc_handle *h);

/* Cross-shard sum over RCCL (xGMI) for hosts without torch.distributed (Julia):
 * nccl_unique_id is the 128-byte ncclUniqueId made by amc_comm_unique_id on rank 0
 * and shipped to the other ranks by the caller. */
/* RCCL is resolved with dlopen at the first of these calls (librccl.so.1, as any RCCL the host process has loaded already);
 * AMC_RCCL_LIBRARY=<file> names the library to use instead -- a site's own build, or the shared-memory stand-in of the
 * tests that lets several ranks share one GPU (tests/aux/fake_rccl.c). */
int  amc_comm_unique_id(void *id128);
int  amc_comm_init(amc_handle *h, int rank, int n_ranks, const void *id128);
/* The sum runs on a stream of its own (the host waits for it without draining the sweeps queued on the engine's stream),
 * ordered behind the collectives the estimator has queued on the engine's stream with the same communicator. */
int  amc_allreduce_sum(amc_handle *h, double *buf, int n);
/* records[i] <- the merged records i of ALL shards (reproducible sums): one ncclAllReduce in which every shard fills its own
 * slot of a zeroed buffer -- a gather that is exact whatever order RCCL adds in -- then amc_xsum_merge over the slots.
 * Every shard ends with the same bits, those a single shard holding all the chains would have.  Identity without a communicator. */
int  amc_allreduce_xsum(amc_handle *h, double *records, int n_records);
/* *forced = 1 when the environment variable AMC_RCCL_LIBRARY replaced librccl in this process (a site's own build, or the
 * tests' shared-memory stand-in): a multi-GPU figure obtained that way has to say so. */
int  amc_comm_library_forced(int *forced);
/* Drop the communicator: the handle is a single shard again (a later amc_comm_init may give it a new one).  For ranks whose
 * amc_comm_init succeeded in a launch where another rank's failed. */
int  amc_comm_destroy(amc_handle *h);
/* What the communicator says about itself (ncclCommCount, ncclCommUserRank), the RCCL version (ncclGetVersion) and the file
 * the RCCL symbols were resolved from -- so that a multi-GPU result can show that RCCL really spanned N ranks and which
 * library carried it.  Without a communicator: 1 rank, rank 0, version 0, empty path.  Any output pointer may be NULL. */
int  amc_comm_info(amc_handle *h, int *n_ranks, int *rank, int *rccl_version, char *librccl_path, int path_capacity);
/* hipRuntimeGetVersion of the HIP runtime this library is bound to in this process, and the file it was loaded from: a
 * process that imported torch first binds torch's bundled runtime, a bare one the system's (/opt/rocm). */
int  amc_runtime_info(int *hip_runtime_version, char *hip_runtime_path, int path_capacity);

/* Parity-test hooks: evaluate arithmetic-spec primitives on the device.
 * fn: 0 exp(a), 1 log(a), 2 sinpi(a), 3 cospi(a), 4 sqrt(a), 5 a/b (IEEE), 6 a/b by the kernel's
 * reciprocal-correction sequence (must equal 5 bit for bit), 7 the Box-Muller log, 8 the Box-Muller
 * radius sqrt (must equal 4 bit for bit on {0} U [2^-52, 80]); 9 log_proposal_density(delta = a, sigma = b)
 * (particle_1d.jl:52-54) and 10 its derivative with respect to sigma (withgrad_log_proposal_density!, gradients.jl:28-33),
 * both in the reference's operation order (ForwardDiff's dual rules written out) -- the values test/ad_backends_test.jl:31-32
 * pins, and what the host-side withgrad_log_proposal_density returns; 11 the same derivative as the estimator KERNEL forms
 * it (one fma chain with a split coefficient, within a few ulp of 10: the estimator's summands are tolerance-matched,
 * DESIGN.md section 3.6b).  Host buffers. */
int  amc_selftest_math(int device, int fn, const double *a, const double *b_or_null,
                       double *out, int64_t n);
/* The sweep kernel settles most accept decisions from a float estimate of exp(dlogp) whose error interval is rigorous
 * (DESIGN.md section 3.6); this hook walks EVERY float t in [t_to, t_from] (t_to <= t_from <= 0) on the device and
 * returns the largest relative deviation of that estimate from the arithmetic spec's f64 exp(t). */
int  amc_selftest_accept_filter(int device, float t_from, float t_to, double *max_rel_err);
/* The K == 1 harmonic sweeps settle those decisions from y = an estimate of dlogp * log2(e) formed WITHOUT the exact dlogp, from
 * -beta delta (x + xn) in Float32 under a guard that turns it into NaN where it may not be used (amc_model.h, harmonic_filter_y).
 * y[i]: that value as a sweep lane forms it for position x[i] and displacement delta[i] in a launch of this beta and sigma
 * (sigma bounds delta, checked once per launch).  Host buffers. */
int  amc_selftest_filter_argument(int device, double beta, double sigma, const double *x, const double *delta, float *y,
                                  int64_t n);
/* out4[i] = Philox4x32-10(key = seed, counter of draw (pair[i], t[i], draw, stream)). */
int  amc_selftest_philox(int device, uint64_t seed, const uint64_t *pair, const uint64_t *t,
                         uint32_t draw, uint32_t stream, uint32_t *out4, int64_t n);

/* The kernels' wave-wide integer totals (every reproducible sum ends in one): values is [6][64] -- six 64-bit integers per lane
 * of one wavefront --, totals[0..5] their sums through the six-value form, [6..7] values 4, 1 through the two-value form,
 * [8..10] values 5, 0, 2 through the three-value form, [11] value 3 alone, [12] the largest low 32-bit word of row 0;
 * totals_plain[0..5]: the six sums by plain DPP rounds.  Sums are modulo 2^64. */
int  amc_selftest_wave_totals(int device, const int64_t *values, int64_t *totals, int64_t *totals_plain);
/* The math tables as a block holds them in LDS: one block stages them the way every kernel does and copies its LDS out;
 * out546: 546 doubles (the rotated layout, the LOGC entries times -2: amc_math.h).  Host buffer. */
int  amc_selftest_staged_tables(int device, double *out546);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
