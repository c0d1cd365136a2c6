// hx_mockcat.h -- the definition of a Poisson-sampled mock catalogue as pure functions: the two Poisson samplers,
// the sub-pixel offsets and the position of a point (through the face coordinates of hx_healpix.h), and the noise of a value.  Usable
// from device code and from the host test (tests/csrc/test_mockcat.cpp), which runs the very code the kernels of hx_mockcat.hip run.
//
// Random bits: Philox4x32-10 (hx_philox.h), key (seed & 0xffffffff, seed >> 32), counter (RING pixel, index, 0x80000000 | stream,
// realisation).  Stream 0: the count draws of the pixel (index 0 the inversion uniform, index = iteration of the rejection sampler);
// stream 1: the position of the index-th point of the pixel; stream 2 + j: the noise of value column j of that point.
//
// Every function rounds operation by operation (no contraction into fused multiply-adds), so that the host and the device differ only
// where their exp / log / lgamma / sqrt do, and in the positions the sqrt / atan2 of hxpix::xyf2lonlat.
#pragma once
#include "hx_healpix.h"
#include "hx_philox.h"

namespace hxmock {

using hxpix::ring2xyf;    // RING pixel -> (face, ix, iy)
using hxpix::xyf2lonlat;  // (face, ix, iy, u, v) -> (lon, lat)

constexpr uint32_t STREAM_BIT = 0x80000000u;  // third counter word: disjoint from hx_synalm's components (< 64)
constexpr uint32_t STREAM_COUNT = 0, STREAM_POSITION = 1, STREAM_VALUE0 = 2;
constexpr double LAMBDA_SWITCH = 32.0;        // inversion below, PTRS from here on
constexpr double LAMBDA_MAX = 1073741824.0;   // 2^30
constexpr int INVERSION_KMAX = 200;           // the sequential search stops here (rounding can leave the cdf below the largest u)
constexpr int PTRS_MAXIT = 64;                // iterations of the rejection sampler; after that many rejections the count is floor(lambda)

HX_PHILOX_HD bool lambda_valid(double lam) { return lam >= 0.0 && lam <= LAMBDA_MAX; }  // (a NaN fails both)

// Inversion by sequential search, 0 < lam < 32, on the uniform u in [0, 1).
HX_PHILOX_HD long long poisson_inversion(double lam, double u)
{
    HX_PIX_NO_CONTRACT
    double p = exp(-lam), cdf = p;
    int k = 0;
    while (u >= cdf && k < INVERSION_KMAX) {
        ++k;
        p *= lam / (double)k;
        cdf += p;
    }
    return k;
}

// Hoermann's PTRS (transformed rejection with squeeze, 1993), 32 <= lam <= 2^30; (u1, u2) of one Philox call per iteration.
HX_PHILOX_HD long long poisson_ptrs(double lam, uint32_t pixel, uint32_t realisation, uint32_t k0, uint32_t k1)
{
    HX_PIX_NO_CONTRACT
    const double slam = sqrt(lam), loglam = log(lam);
    const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double inva = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    for (int it = 0; it < PTRS_MAXIT; ++it) {
        double u1, V;
        hxphilox::uniforms(hxphilox::philox4x32_10(pixel, (uint32_t)it, STREAM_BIT | STREAM_COUNT, realisation, k0, k1), &u1, &V);
        const double U = u1 - 0.5, us = 0.5 - fabs(U);
        const double kf = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return (long long)kf;
        if (kf < 0.0 || (us < 0.013 && V > us)) continue;
        if (log(V) + log(inva) - log(a / (us * us) + b) <= -lam + kf * loglam - lgamma(kf + 1.0)) return (long long)kf;
    }
    return (long long)floor(lam);
}

// n_p ~ Poisson(lam) of RING pixel `pixel`; lam must pass lambda_valid.  lam = 0 draws nothing.
HX_PHILOX_HD long long poisson_count(double lam, uint32_t pixel, uint32_t realisation, uint32_t k0, uint32_t k1)
{
    if (lam == 0.0) return 0;
    if (lam < LAMBDA_SWITCH) {
        double u1, u2;
        hxphilox::uniforms(hxphilox::philox4x32_10(pixel, 0u, STREAM_BIT | STREAM_COUNT, realisation, k0, k1), &u1, &u2);
        return poisson_inversion(lam, u2);
    }
    return poisson_ptrs(lam, pixel, realisation, k0, k1);
}

// The sub-pixel offsets of one position call: ((x >> 8) + 1/2) 2^-24, strictly inside (0, 1) with a margin of 2^-25.
HX_PHILOX_HD void offsets(const hxphilox::Words &w, double *u, double *v)
{
    *u = ((double)(w.x[0] >> 8) + 0.5) * 0x1p-24;
    *v = ((double)(w.x[1] >> 8) + 0.5) * 0x1p-24;
}

// The index-th point of RING pixel `pixel` (the counter word) at (face, ix, iy).
HX_PHILOX_HD void point_lonlat(long long nside, uint32_t pixel, uint32_t index, uint32_t realisation, uint32_t k0, uint32_t k1, double *lon,
                               double *lat)
{
    int face;
    long long ix, iy;
    double u, v;
    ring2xyf(nside, (long long)pixel, &face, &ix, &iy);
    offsets(hxphilox::philox4x32_10(pixel, index, STREAM_BIT | STREAM_POSITION, realisation, k0, k1), &u, &v);
    xyf2lonlat(nside, face, ix, iy, u, v, lon, lat);
}

// The noise of value column j of that point: the `first` normal of its call.
HX_PHILOX_HD double value_noise(uint32_t pixel, uint32_t index, uint32_t j, uint32_t realisation, uint32_t k0, uint32_t k1)
{
    double first, second;
    hxphilox::normal_pair(hxphilox::philox4x32_10(pixel, index, STREAM_BIT | (STREAM_VALUE0 + j), realisation, k0, k1), &first, &second);
    return first;
}

}  // namespace hxmock
