// hx_ang2pix.h -- (lon, lat) in degrees -> HEALPix RING pixel, device only: what k_ang2pix (hx_mapper.hip) and the prepare kernels of the
// catalogue contexts (hx_catmap.hip, hx_catmap_sel.hip, hx_catalm.hip) inline.
//
// ang2pix follows the published HEALPix algorithm (Gorski et al. 2005; healpix_cxx
// T_Healpix_Base::loc2pix, RING branch), the third-party code healpy calls; it is absent
// from /root/reference, so index parity is pinned on the test-side numpy restatement
// and on the pix2ang round trip of every pixel centre (tests/test_gpu_mapper.py), and at
// pixel edges on the exact pixel and admissible set of tests/pixel_reference.py
// (tests/test_gpu_pixel_edges.py).
#pragma once
#include <hip/hip_runtime.h>

namespace hx {

namespace {

constexpr double kInvHalfPi = 0.6366197723675813430755350534900574;
constexpr double kDeg2Rad = 0.017453292519943295769236907684886;  // numpy: NPY_PI / 180
constexpr double kHalfPi = 1.5707963267948966192313216916398;
constexpr double kTwoThird = 2.0 / 3.0;

// healpix_cxx fmodulo(v, 4.0)
__device__ inline double fmodulo4(double v)
{
#pragma clang fp contract(off)
    if (v >= 0.0) return (v < 4.0) ? v : fmod(v, 4.0);
    double t = fmod(v, 4.0) + 4.0;
    return (t == 4.0) ? 0.0 : t;
}

__device__ inline long long ang2pix_ring_one(long long nside, double lon_deg, double lat_deg)
{
    // every operation rounds on its own, as in numpy / healpix_cxx built without FMA contraction: a fused
    // pi/2 - lat * (pi/180) gives theta = -6e-17 instead of 0 for lat = 90
#pragma clang fp contract(off)
    // healpy lonlat2thetaphi: theta = pi/2 - radians(lat), phi = radians(lon)
    double theta = kHalfPi - lat_deg * kDeg2Rad;
    double phi = lon_deg * kDeg2Rad;
    double z = cos(theta);
    bool have_sth = (theta < 0.01) || (theta > 3.14159 - 0.01);
    // theta in (pi, pi + 1e-5] passes lonlat_valid as it passes healpy's check; its sine is negative, and from nside 2^17 on a negative
    // tmp truncates to negative jp, jm and a pixel hundreds of rings from the pole.  Clamped, such a point falls in the last ring
    // (ir = 1), where the truncation towards zero already put it at every smaller nside.  sin >= 0 for every double theta in [0, pi].
    double sth = have_sth ? fmax(sin(theta), 0.0) : 0.0;
    double za = fabs(z);
    double tt = fmodulo4(phi * kInvHalfPi);
    long long npix = 12 * nside * nside, ncap = 2 * nside * (nside - 1), nl4 = 4 * nside;
    if (za <= kTwoThird) {
        double temp1 = (double)nside * (0.5 + tt);
        double temp2 = (double)nside * z * 0.75;
        long long jp = (long long)(temp1 - temp2);
        long long jm = (long long)(temp1 + temp2);
        long long ir = nside + 1 + jp - jm;
        long long kshift = 1 - (ir & 1);
        long long t1 = jp + jm - nside + kshift + 1 + nl4 + nl4;
        long long ip = (t1 >> 1) % nl4;
        return ncap + (ir - 1) * nl4 + ip;
    }
    double tp = tt - (double)(long long)tt;
    double tmp = ((za < 0.99) || !have_sth) ? (double)nside * sqrt(3.0 * (1.0 - za))
                                           : (double)nside * sth / sqrt((1.0 + za) / 3.0);
    long long jp = (long long)(tp * tmp);
    long long jm = (long long)((1.0 - tp) * tmp);
    long long ir = jp + jm + 1;
    long long ip = (long long)(tt * (double)ir);
    if (ip >= 4 * ir) ip = 4 * ir - 1;  // healpix_cxx asserts this never happens; stay in range
    return (z > 0.0) ? 2 * ir * (ir - 1) + ip : npix - 2 * ir * (ir + 1) + ip;
}

// healpy.ang2pix validates its input (check_theta_valid: 0 <= theta <= pi + 1e-5, which a NaN fails) and
// raises ValueError before any pixel is touched; the formulas above yield negative or out-of-range
// indices for such points.  Invalid points (a non-finite longitude included) get pixel -1 and are counted
// in *nbad; the entry points return HX_ERR_ARG before anything is scattered.  The rule is evaluated on the
// double theta = pi/2 - radians(lat): a latitude an ulp beyond +-90 whose theta rounds to 0 or pi is accepted,
// and an accepted theta in (pi, pi + 1e-5] gets a pixel of the last ring (tests/test_gpu_pixel_edges.py).
__device__ inline bool lonlat_valid(double lon_deg, double lat_deg)
{
#pragma clang fp contract(off)
    const double theta = kHalfPi - lat_deg * kDeg2Rad;
    return isfinite(lon_deg) && theta >= 0.0 && theta <= 3.14159265358979323846 + 1e-5;
}

}  // namespace

}  // namespace hx
