/* f32_param_twin.c -- host twin of the all-Float32 model (Float32 state AND Float32 policy parameters).
 *
 * Restates in plain C floats what a handle with param_dtype = Float32 computes: the Float32 Box-Muller pair of a Philox word
 * (radius uniform, -2 log u, sqrt, sincospi), the Float32 quotient of log_proposal_density, one mc_step! and mc_sweep! of a chain.
 * Everything that does not change with the parameter type -- Philox, the counter layout, the spare bits, the accept and
 * move-pick uniforms, the categorical walk, the Float32 potentials, exp / log of the arithmetic spec -- is taken from the
 * oracle's exported functions, so this file shares no source and no header with the product.  Its table constants come
 * from tools/gen_math_tables.py (f32_param_tables.inc).
 * Build: cc -O2 -ffp-contract=off (tests/f32_param_twin.py), linked against oracle/libamc_oracle.so.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "f32_param_tables.inc"

/* the oracle's exported pieces (oracle/amc_oracle.h) */
void     amo_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
void     amo_counter(uint64_t pair, uint64_t t, uint32_t draw, uint32_t stream, uint32_t ctr[4]);
double   amo_exp(double x);
double   amo_log(double x);
uint32_t amo_spare_accept12(const uint32_t v[4], int half);
uint32_t amo_spare_pick12(const uint32_t v[4], int half);
double   amo_uniform_accept(uint32_t accept12, uint32_t lo, uint32_t hi);
double   amo_uniform_pick(uint32_t pick12, uint32_t lo);
double   amo_uniform_co(uint32_t lo, uint32_t hi);
float    amo_potential_f32(int pot, float x);
int      amo_categorical(const double *weights, int K, double r);

enum { TWIN_STREAM_INIT = 0, TWIN_STREAM_METROPOLIS = 1, TWIN_DRAW_NORMAL = 0, TWIN_DRAW_ACCEPT = 1 };

static float as_float(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t as_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

/* u in (0, 1]: the odd 53-bit integer N = 2 ((hi:lo) >> 12) + 1, high word exact, low word and sum rounded to nearest */
float twin_uniform_oc_f32(uint32_t lo, uint32_t hi)
{
    const uint64_t n52 = (((uint64_t)hi << 32) | lo) >> 12;
    const uint64_t N = 2u * n52 + 1u;
    const float f_hi = (float)(uint32_t)(N >> 32), f_lo = (float)(uint32_t)N;
    return fmaf(f_hi, 0x1.0p+32f, f_lo) * 0x1.0p-53f;
}

/* a = -2 log u */
float twin_neg2log_f32(float u)
{
    const uint32_t ux = as_bits(u);
    int32_t k = (int32_t)(ux >> 23) - 127;
    uint32_t mx = ux & 0x007fffffu;
    const uint32_t i = (mx + 0x004afb0du) & 0x00800000u;
    k += (int32_t)(i >> 23);
    mx |= i ^ 0x3f800000u;
    const float m = as_float(mx);
    const uint32_t idx = ((mx >> 16) & 0xffu) - TWIN_LOG_IDX_MIN;
    const float invc = TWIN_LOGF[2 * idx], n2logc = TWIN_LOGF[2 * idx + 1];
    const float r = fmaf(m, invc, -1.0f);
    float p = 0.5f;
    p = fmaf(p, r, -0x1.555556p-1f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, -2.0f);
    const float dk = (float)k;
    const float hi = fmaf(dk, -2.0f * 0x1.62e300p-1f, n2logc);
    return fmaf(p, r, fmaf(dk, -2.0f * 0x1.2fefa4p-17f, hi));
}

/* (sin, cos)(pi w), w = A 2^-23, A = 2^24 - (word >> 8) */
void twin_sincospi_f32(uint32_t word, float *sp, float *cp)
{
    const int32_t A = (int32_t)(0x01000000u - (word >> 8));
    const int32_t n = (A + 0x10000) >> 17;                   /* nearest multiple of 2^17 (= 1/64 in w) */
    const float r = (float)(A - n * 0x20000) * 0x1.0p-23f;   /* exact: |A - n 2^17| <= 2^16 */
    const float z = r * r;
    const float sr = fmaf(z, -0x1.4abbcep+2f, 0x1.921fb6p+1f) * r;
    const float cr = fmaf(fmaf(z, 0x1.03c1f0p+2f, -0x1.3bd3ccp+2f), z, 1.0f);
    const float S = TWIN_SINCOSF[2 * (n & 127)], C = TWIN_SINCOSF[2 * (n & 127) + 1];
    *sp = fmaf(S, cr, C * sr);
    *cp = fmaf(C, cr, -(S * sr));
}

void twin_box_muller_f32(const uint32_t v[4], float z[2])
{
    const float s = sqrtf(twin_neg2log_f32(twin_uniform_oc_f32(v[0], v[1])));
    float sn, cs;
    twin_sincospi_f32(v[3], &sn, &cs);
    z[0] = sn * s;
    z[1] = cs * s;
}

/* n words (4 x uint32 each) -> their normals, and the intermediate values the accuracy test compares in Float64 */
void twin_box_muller_words(int64_t n, const uint32_t *words, float *z, float *u_out)
{
    for (int64_t i = 0; i < n; ++i) {
        twin_box_muller_f32(words + 4 * i, z + 2 * i);
        if (u_out) u_out[i] = twin_uniform_oc_f32(words[4 * i], words[4 * i + 1]);
    }
}

/* the NORMAL draws of the pairs pair0 .. pair0 + n - 1 at step t (what the sweep reads), as words */
void twin_normal_words(uint64_t seed, uint64_t pair0, int64_t n, uint64_t t, uint32_t *words)
{
    const uint32_t key[2] = { (uint32_t)seed, (uint32_t)(seed >> 32) };
    for (int64_t i = 0; i < n; ++i) {
        uint32_t ctr[4];
        amo_counter(pair0 + (uint64_t)i, t, TWIN_DRAW_NORMAL, TWIN_STREAM_METROPOLIS, ctr);
        amo_philox4x32_10(ctr, key, words + 4 * i);
    }
}

static double julia_min(double a, double b)
{
    if (a != a) return a;
    if (b != b) return b;
    return b < a ? b : a;
}

/* log_proposal_density (particle_1d.jl:52-54) with sigma::Float32: the quotient is Float32, 2 pi is Float64 */
double twin_logq(float delta, float sigma)
{
    const double TWO_PI = 0x1.921fb54442d18p+2;
    const float s2 = sigma * sigma;
    const float q = (-(delta * delta)) / (2.0f * s2);
    return (double)q - amo_log(TWO_PI * (double)s2) / 2.0;
}

/* One mc_step! (metropolis.jl:176-190) on Particle{Float32} with a Float32 sigma, z = randn(rng, Float32), u = rand(rng). */
int twin_mc_step(int pot, float beta, float sigma, float z, double u, float *x, float *e)
{
    float delta = 0.0f + sigma * z;                               /* :177 sample_action! */
    const double logq_f = twin_logq(delta, sigma);                /* :178 */
    const float e1 = *e;                                          /* :179 perform_action! */
    *x = *x + delta;
    *e = amo_potential_f32(pot, *x);
    const float e2 = *e;
    const float dlogp = ((-e2) * beta) - ((-e1) * beta);          /* :180 */
    delta = -delta;                                               /* :181 invert_action! */
    const double logq_b = twin_logq(delta, sigma);                /* :182 */
    const double alpha = julia_min(1.0, amo_exp(((double)dlogp + logq_b) - logq_f));   /* :183 */
    if (alpha > u) return 1;                                      /* :184 */
    *x = *x + delta;                                              /* :187 perform_action_cached! */
    *e = amo_potential_f32(pot, *x);
    return 0;
}

/* Particle(Float32(lo + (hi - lo) rand(rng)), beta): the INIT stream of the chain's pair, as the Float32-state form has it */
void twin_init_uniform(uint64_t seed, int64_t offset, int64_t M, int pot, double lo, double hi, float *x, float *e)
{
    const uint32_t key[2] = { (uint32_t)seed, (uint32_t)(seed >> 32) };
    for (int64_t c = 0; c < M; ++c) {
        const uint64_t g = (uint64_t)(offset + c);
        const int half = (int)(g & 1u);
        uint32_t ctr[4], v[4];
        amo_counter(g >> 1, 0, 0, TWIN_STREAM_INIT, ctr);
        amo_philox4x32_10(ctr, key, v);
        x[c] = (float)(lo + (hi - lo) * amo_uniform_co(v[2 * half], v[2 * half + 1]));
        e[c] = amo_potential_f32(pot, x[c]);
    }
}

/* mc_sweep! (metropolis.jl:203-212) of M chains (global ids offset ..), steps [t0, t0 + n_steps): x, e in place, and
 * accepted / total calls per move and chain ([K][M]) added to.  force_z / force_u (or NULL): the step's variate and uniform of
 * every chain are also written there ([n_steps][M]) for the independent restatement of the tests. */
void twin_sweep(uint64_t seed, int64_t offset, int64_t M, int pot, const float *beta, int K, const float *sigma,
                const double *weight, uint64_t t0, int64_t n_steps, float *x, float *e, int64_t *accepted, int64_t *total,
                float *z_out, double *u_out)
{
    const uint32_t key[2] = { (uint32_t)seed, (uint32_t)(seed >> 32) };
    for (int64_t c = 0; c < M; ++c) {
        const uint64_t g = (uint64_t)(offset + c);
        const uint64_t pair = g >> 1;
        const int half = (int)(g & 1u);
        for (int64_t i = 0; i < n_steps; ++i) {
            const uint64_t t = t0 + (uint64_t)i;
            uint32_t ctr[4], v[4], va[4];
            amo_counter(pair, t, TWIN_DRAW_NORMAL, TWIN_STREAM_METROPOLIS, ctr);
            amo_philox4x32_10(ctr, key, v);
            amo_counter(pair, t, TWIN_DRAW_ACCEPT, TWIN_STREAM_METROPOLIS, ctr);
            amo_philox4x32_10(ctr, key, va);
            int id = 0;
            if (K > 1) id = amo_categorical(weight, K, amo_uniform_pick(amo_spare_pick12(v, half), va[2 * half]));   /* :206 */
            float zz[2];
            twin_box_muller_f32(v, zz);
            const double u = amo_uniform_accept(amo_spare_accept12(v, half), va[2 * half], va[2 * half + 1]);
            if (z_out) z_out[i * M + c] = zz[half];
            if (u_out) u_out[i * M + c] = u;
            accepted[(int64_t)id * M + c] += twin_mc_step(pot, beta[c], sigma[id], zz[half], u, &x[c], &e[c]);   /* :208 */
            total[(int64_t)id * M + c] += 1;                                                                     /* :209 */
        }
    }
}
