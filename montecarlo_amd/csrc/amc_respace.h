// amc_respace.h -- the respacing rule of a temperature ladder (DESIGN.md section 3.13 "Respacing"): new beta values for the interior
// rungs from the swap counts per gap or from the flow counts per rung.  Short serial Float64 arithmetic -- + - * / sqrt, nothing
// contracted (the units that include this are built with -ffp-contract=off), in the order of the DESIGN text -- which lane 0 of
// ladder_respace_kernel (amc_exchange.h) runs; written as a host-and-device inline function, as amc_xsum.h is, so that the same
// text runs on the CPU under the sanitizers (tests/aux/respace_rule_host.cpp).  The host twin is tests/respace_twin.py.
#pragma once

#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#define AMC_RS_HD __host__ __device__ inline

namespace amc {
namespace rs {

enum { RS_MAX_RUNGS = 64 };
enum { RS_ACCEPTANCE = 1, RS_FLOW = 2 };      // AMC_RESPACE_ACCEPTANCE, AMC_RESPACE_FLOW of include/amc.h
// status: 0 the ladder was respaced; 1 no weight (W is not a positive finite number); 2 a count the rule divides by is zero;
// 3 the ladder at hand is not finite or not strictly monotone; 4 the new ladder is not finite or not strictly monotone
enum { RS_OK = 0, RS_NO_WEIGHT = 1, RS_NO_COUNTS = 2, RS_BAD_LADDER = 3, RS_COLLAPSED = 4 };

AMC_RS_HD bool rs_finite(double v) { return v - v == 0.0; }       // (Inf - Inf and NaN - NaN are NaN)

// strictly monotone in the direction of its first step, every value finite (R >= 2)
AMC_RS_HD bool rs_monotone(const double* v, int R, bool up)
{
    for (int r = 0; r < R; ++r)
        if (!rs_finite(v[r])) return false;
    for (int r = 0; r + 1 < R; ++r)
        if (!(up ? v[r + 1] > v[r] : v[r + 1] < v[r])) return false;
    return true;
}

// b[R]: the ladder at hand.  counts: RS_ACCEPTANCE attempted[R - 1] then accepted[R - 1]; RS_FLOW n[R][3] (amc_flow_rungs' layout).
// out[R]: the new ladder; it means something only with status 0.  w[R], G[R]: the caller's work space (LDS in the kernel, where
// arrays of the function's own would live in scratch memory).  Returns the status.
AMC_RS_HD int respace_rule(int rule, int R, const double* b, const uint64_t* counts, double gamma, double eps, double* out, double* w, double* G)
{
    if (rule == RS_ACCEPTANCE) {
        const uint64_t *att = counts, *acc = counts + (R - 1);
        for (int j = 0; j + 1 < R; ++j) {
            if (att[j] == 0) return RS_NO_COUNTS;
            w[j] = (double)(att[j] - acc[j]) / (double)att[j];
        }
    } else {
        for (int r = 0; r < R; ++r)
            if (counts[3 * r + 1] + counts[3 * r + 2] == 0) return RS_NO_COUNTS;
        for (int j = 0; j + 1 < R; ++j) {
            const double f0 = (double)counts[3 * j + 1] / (double)(counts[3 * j + 1] + counts[3 * j + 2]);
            const double f1 = (double)counts[3 * j + 4] / (double)(counts[3 * j + 4] + counts[3 * j + 5]);
            const double d = f0 - f1;
            w[j] = __builtin_sqrt(d > 0.0 ? d : 0.0);
        }
    }
    const bool up = b[1] > b[0];
    if (!rs_monotone(b, R, up)) return RS_BAD_LADDER;
    double W = 0.0;
    for (int j = 0; j + 1 < R; ++j) W = W + w[j];
    if (!(W > 0.0) || !rs_finite(W)) return RS_NO_WEIGHT;
    const double m = (eps * W) / (double)(R - 1);
    G[0] = 0.0;
    for (int j = 0; j + 1 < R; ++j) {
        w[j] = w[j] < m ? m : w[j];               // wf
        G[j + 1] = G[j] + w[j];
    }
    for (int k = 1; k + 1 < R; ++k) {
        const double t = ((double)k * G[R - 1]) / (double)(R - 1);
        int j = 0;
        while (j < R - 2 && !(G[j + 1] > t)) ++j;
        const double frac = (t - G[j]) / w[j];
        const double nb = b[j] + (b[j + 1] - b[j]) * frac;
        out[k] = b[k] + gamma * (nb - b[k]);
    }
    out[0] = b[0];
    out[R - 1] = b[R - 1];
    if (!rs_monotone(out, R, up)) return RS_COLLAPSED;
    return RS_OK;
}

}  // namespace rs
}  // namespace amc
