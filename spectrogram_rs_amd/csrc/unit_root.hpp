// unit_root.hpp -- the root of unity every twiddle table is made of: host code only, no HIP, so that the CPU suite can compile it with
// g++ and check it point by point (tests/cpp/unit_root_check.cpp).
#pragma once

#include <cmath>

namespace sgx {

struct UnitRoot { float re, im; };

// e^{-2 pi i e / n} as two floats: the double angle of e mod n, rounded once; exact on the four axes.
inline UnitRoot unit_root(unsigned long long e, unsigned long long n)
{
    e %= n;
    if (e == 0) return {1.0f, 0.0f};
    if (4 * e == n) return {0.0f, -1.0f};
    if (2 * e == n) return {-1.0f, 0.0f};
    if (4 * e == 3 * n) return {0.0f, 1.0f};
    const double ang = -2.0 * M_PI * (double)e / (double)n;
    return {(float)std::cos(ang), (float)std::sin(ang)};
}

}  // namespace sgx
