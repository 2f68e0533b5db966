// tune_rule_host.cpp -- the tuning rule of the widths per rung (montecarlo_amd/csrc/amc_tune.h, tune_rule: what every lane of
// rung_sigma_tune_kernel runs for its entry) on the host.
//
//   tune_rule_host <target> <gamma> <lo> <hi> <min_calls>  <  entries
// target, gamma, lo, hi as hexadecimal floating-point text (strtod reads it exactly), min_calls as a decimal integer.  Every line of the
// standard input is one entry: <s> <A> <T> <inconsistent: 0 or 1>, s as hexadecimal floating-point text, A and T as decimal unsigned
// 64-bit integers.  Prints per entry the status and the new width as hexadecimal floating-point text.
// Build: c++ -std=c++17 -ffp-contract=off, with -fsanitize=address,undefined (tests/test_tune_host.py); the header is plain host C++
// once the two qualifiers are empty.
#define __host__
#define __device__
#include "amc_tune.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const double target = std::strtod(argv[1], nullptr), gamma = std::strtod(argv[2], nullptr);
    const double lo = std::strtod(argv[3], nullptr), hi = std::strtod(argv[4], nullptr);
    const uint64_t min_calls = std::strtoull(argv[5], nullptr, 10);
    char s_text[64], a_text[32], t_text[32];
    int bad = 0;
    while (std::scanf("%63s %31s %31s %d", s_text, a_text, t_text, &bad) == 4) {
        const double s = std::strtod(s_text, nullptr);
        const uint64_t A = std::strtoull(a_text, nullptr, 10), T = std::strtoull(t_text, nullptr, 10);
        double out = 0.0;
        const int st = amc::tn::tune_rule(s, A, T, bad != 0, target, gamma, min_calls, lo, hi, &out);
        std::printf("%d %a\n", st, out);
    }
    return 0;
}
