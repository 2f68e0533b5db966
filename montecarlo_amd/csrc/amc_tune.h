// amc_tune.h -- the tuning rule of a proposal width per (move, rung) (DESIGN.md section 3.13 "Tuning the widths"): one damped
// fixed-point step sigma <- sigma a / target from the accepted and total calls of a window, limited to a factor of two per call and
// clamped to [lo, hi].  Float64 + - * / and comparisons, nothing contracted (the units that include this are built with
// -ffp-contract=off), in the order of the DESIGN text; every lane of rung_sigma_tune_kernel (amc_exchange.h) runs it for its own
// entry.  Written as a host-and-device inline function, as amc_respace.h is, so that the same text runs on the CPU under the
// sanitizers (tests/aux/tune_rule_host.cpp).  The host twin is tests/tune_twin.py.
#pragma once

#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#define AMC_TN_HD __host__ __device__ inline

namespace amc {
namespace tn {

// status of one entry: 0 tuned; 1 fewer than min_calls calls in the window (sigma keeps its bits); 2 the window is inconsistent -- a
// counter below its base, or more accepted than total calls -- (sigma keeps its bits); 3 tuned and clamped to lo or hi
enum { TN_OK = 0, TN_FEW_CALLS = 1, TN_INCONSISTENT = 2, TN_CLAMPED = 3 };

// s: the width at hand.  A, T: accepted and total calls of the window; inconsistent: the window could not be formed.  Returns the
// status; *out is the new width (the bits of s with status 1 and 2).
AMC_TN_HD int tune_rule(double s, uint64_t A, uint64_t T, bool inconsistent, double target, double gamma, uint64_t min_calls, double lo, double hi,
                        double* out)
{
    *out = s;
    if (inconsistent || A > T) return TN_INCONSISTENT;
    if (T < min_calls) return TN_FEW_CALLS;
    const double a = (double)A / (double)T;
    double q = a / target;
    q = q < 0.5 ? 0.5 : (q > 2.0 ? 2.0 : q);
    const double sq = s * q;
    const double d = sq - s;
    const double gd = gamma * d;
    double v = s + gd;
    int st = TN_OK;
    if (v < lo) { v = lo; st = TN_CLAMPED; }
    if (v > hi) { v = hi; st = TN_CLAMPED; }
    *out = v;
    return st;
}

}  // namespace tn
}  // namespace amc
