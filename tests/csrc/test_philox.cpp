// Host run of heracles_amd/csrc/hx_philox.h, the code the generator kernel of hx_synalm runs: the known answers of Philox4x32-10,
// the uniforms at the edges of the bit range and the radius there.  g++ -O2 -std=c++17 tests/csrc/test_philox.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../heracles_amd/csrc/hx_philox.h"

using namespace hxphilox;

static int fails = 0;
#define CHECK(cond)                                             \
    do {                                                        \
        if (!(cond)) {                                          \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
            ++fails;                                            \
        }                                                       \
    } while (0)

static void known(const uint32_t (&c)[4], const uint32_t (&k)[2], const uint32_t (&want)[4])
{
    const Words w = philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
    for (int i = 0; i < 4; ++i) {
        if (w.x[i] != want[i]) {
            std::printf("FAIL known answer word %d: %08x, expected %08x\n", i, w.x[i], want[i]);
            ++fails;
        }
    }
}

int main()
{
    known({0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u});
    known({0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu});
    known({0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u});

    double u1, u2, a, b;
    const Words zero = {{0, 0, 0, 0}}, ones = {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}};
    uniforms(zero, &u1, &u2);
    CHECK(u1 == 0x1p-53);
    CHECK(u2 == 0.0);
    normal_pair(zero, &a, &b);
    CHECK(std::isfinite(a) && std::isfinite(b));
    CHECK(std::fabs(std::hypot(a, b) - std::sqrt(106.0 * std::log(2.0))) < 1e-14 * 8.6);  // r = sqrt(-2 ln 2^-53)
    CHECK(b == 0.0);                                                                       // the angle is exactly 0
    uniforms(ones, &u1, &u2);
    CHECK(u1 == 1.0);
    CHECK(u2 == 1.0 - 0x1p-53);
    normal_pair(ones, &a, &b);
    CHECK(std::isfinite(a) && std::isfinite(b));
    CHECK(a == 0.0 && b == 0.0);  // r = sqrt(-2 ln 1) = 0
    // u1 is never 0 and u2 never 1, one step inside the edges too
    const Words near = {{0xffffffffu, 0xffffffbfu, 0, 0x40u}};
    uniforms(near, &u1, &u2);
    CHECK(u1 == 1.0 - 0x1p-53);
    CHECK(u2 == 0x1p-53);

    // m = 0 is real, m > 0 carries 1 / sqrt 2 on both parts
    double re, im, re1, im1;
    complex_normal(5, 0, 1, 0, 7, 9, &re, &im);
    CHECK(im == 0.0 && std::signbit(im) == 0);
    normal_pair(philox4x32_10(5, 3, 1, 0, 7, 9), &a, &b);
    complex_normal(5, 3, 1, 0, 7, 9, &re1, &im1);
    CHECK(re1 == a * 0.70710678118654752440 && im1 == b * 0.70710678118654752440);

    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
