// unit_root_check.cpp -- csrc/unit_root.hpp point by point (tests/test_unit_root.py builds this with g++ -fsanitize=address,undefined and
// runs it): for every table length the kernels use and every exponent of two turns, the four axes are exact, every other point is the
// single rounding of the double angle's cosine and sine, and the exponent only counts modulo n.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "unit_root.hpp"

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main()
{
    const unsigned long long lengths[] = {256, 300, 512, 2048, 4096, 4800, 16384};
    unsigned long long failed = 0, axes = 0, points = 0;
    for (unsigned long long n : lengths)
        for (unsigned long long e = 0; e < 2 * n; ++e) {
            const sgx::UnitRoot w = sgx::unit_root(e, n);
            const unsigned long long r = e % n;
            float re, im;
            if (r == 0) { re = 1.0f; im = 0.0f; ++axes; }
            else if (4 * r == n) { re = 0.0f; im = -1.0f; ++axes; }
            else if (2 * r == n) { re = -1.0f; im = 0.0f; ++axes; }
            else if (4 * r == 3 * n) { re = 0.0f; im = 1.0f; ++axes; }
            else {
                const double ang = -2.0 * M_PI * (double)r / (double)n;
                re = (float)std::cos(ang);
                im = (float)std::sin(ang);
            }
            ++points;
            if (!same_bits(w.re, re) || !same_bits(w.im, im)) {
                if (failed++ < 10) std::printf("FAILED n %llu e %llu: (%a, %a), expected (%a, %a)\n", n, e, w.re, w.im, re, im);
            }
            const sgx::UnitRoot v = sgx::unit_root(e + n, n);
            if (!same_bits(v.re, w.re) || !same_bits(v.im, w.im)) {
                if (failed++ < 10) std::printf("FAILED n %llu: e %llu and e + n differ\n", n, e);
            }
        }
    std::printf("%llu points, %llu on the axes, %llu failed\n", points, axes, failed);
    if (failed) return 1;
    std::printf("unit root ok\n");
    return 0;
}
