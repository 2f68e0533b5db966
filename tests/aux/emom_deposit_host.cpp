// The deposit rule of the moments per energy bin (montecarlo_amd/csrc/amc_emom.h: emom_e_x / emom_e_xx, emom_deposit_x / _xx,
// emom_x_inside -- the __host__ __device__ functions energy_moments_kernel calls), compiled for the host:
//     emom_deposit_host <file of little-endian doubles> <x_bound>
// prints the two exponents on the first line, then per value "k_x k_xx pos inside".  tests/test_emom_twin_host.py compares the
// integers with the twin's (tests/emom_twin.py) and with exact rational arithmetic.
#define __host__
#define __device__
#include "amc_emom.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<double> v;
    double d;
    while (std::fread(&d, sizeof(d), 1, f) == 1) v.push_back(d);
    std::fclose(f);
    const double x_bound = std::strtod(argv[2], nullptr);
    const int e_x = amc::emom_e_x(x_bound), e_xx = amc::emom_e_xx(x_bound);
    std::printf("%d %d\n", e_x, e_xx);
    for (double xd : v)
        std::printf("%lld %lld %d %d\n", (long long)amc::emom_deposit_x(xd, e_x), (long long)amc::emom_deposit_xx(xd, e_xx), xd > 0.0 ? 1 : 0,
                    amc::emom_x_inside(xd, x_bound) ? 1 : 0);
    return 0;
}
