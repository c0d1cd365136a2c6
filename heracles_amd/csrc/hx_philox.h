// hx_philox.h -- the random numbers of hx_synalm: Philox4x32-10 (Salmon et al., SC'11) and the conversion of its four words to a
// pair of standard normals.  Pure functions, usable from device code and from the host test (tests/csrc/test_philox.cpp), which
// runs the very code the generator kernel runs.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define HX_PHILOX_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define HX_PHILOX_HD inline
#endif
#include <cstdint>

namespace hxphilox {

struct Words {
    uint32_t x[4];
};

// One call: counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit words.
HX_PHILOX_HD Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    Words w;
    w.x[0] = c0;
    w.x[1] = c1;
    w.x[2] = c2;
    w.x[3] = c3;
    return w;
}

// The two uniforms of one call, both exact in f64: u1 = (k1 + 1) 2^-53 in (0, 1], u2 = k2 2^-53 in [0, 1), with the 53-bit integers
// k1 = (x0 >> 5) 2^26 + (x1 >> 6), k2 = (x2 >> 5) 2^26 + (x3 >> 6).
HX_PHILOX_HD void uniforms(const Words &w, double *u1, double *u2)
{
    const uint64_t k1 = ((uint64_t)(w.x[0] >> 5) << 26) | (w.x[1] >> 6), k2 = ((uint64_t)(w.x[2] >> 5) << 26) | (w.x[3] >> 6);
    *u1 = (double)(k1 + 1) * 0x1p-53;
    *u2 = (double)k2 * 0x1p-53;
}

// Box-Muller: r = sqrt(-2 ln u1), (r cos 2 pi u2, r sin 2 pi u2); r <= sqrt(106 ln 2) = 8.58.
HX_PHILOX_HD void normal_pair(const Words &w, double *first, double *second)
{
    double u1, u2, s, c;
    uniforms(w, &u1, &u2);
    const double r = sqrt(-2.0 * log(u1));
    sincos(6.283185307179586476925 * u2, &s, &c);
    *first = r * c;
    *second = r * s;
}

// The complex standard normal z of coefficient (l, m) of component j: real at m = 0 (imaginary part exactly 0), else
// (first + i second) / sqrt 2, the division as a product with the f64 nearest to 1 / sqrt 2.
HX_PHILOX_HD void complex_normal(uint32_t l, uint32_t m, uint32_t j, uint32_t realisation, uint32_t k0, uint32_t k1, double *re, double *im)
{
    double a, b;
    normal_pair(philox4x32_10(l, m, j, realisation, k0, k1), &a, &b);
    if (m == 0) {
        *re = a;
        *im = 0.0;
    } else {
        *re = a * 0.70710678118654752440;
        *im = b * 0.70710678118654752440;
    }
}

}  // namespace hxphilox
