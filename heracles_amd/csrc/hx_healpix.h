// hx_healpix.h -- HEALPix pixel geometry as pure functions, the one place in csrc that knows the cap / belt / cap
// layout of the RING scheme: RING pixel -> (ring, index in ring), RING pixel <-> (face, ix, iy) <-> NEST pixel, (face, ix, iy) and
// sub-pixel offsets -> (lon, lat), and the geometry of a ring with the unit vectors of its pixel centres.  Usable from device code
// and from the host tests (tests/csrc), which run the very code the kernels run.  Compiles with plain g++.
//
// Every floating-point function rounds operation by operation (no contraction into fused multiply-adds), so that the host and the
// device differ only where their sqrt / sin / cos / atan2 do.
//
// Not here: ang2pix (hx_ang2pix.h; its device transcendentals have no host twin) and the plan's ring table (hx_plan.hip; it spells
// the belt z as (2 nside - i) fact1, whose bits every SHT result depends on).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define HX_PIX_HD __host__ __device__ inline
#else
#define HX_PIX_HD inline
#endif

#if defined(__clang__)
#define HX_PIX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HX_PIX_NO_CONTRACT
#endif

namespace hxpix {

constexpr double HALFPI = 1.57079632679489661923;

// ---- integer helpers ----
HX_PIX_HD long long isqrt_ll(long long v)  // floor(sqrt(v)), v < 2^52
{
    long long r = (long long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// a / b for 0 <= a < 2^32, 0 < b < 2^32: every quotient of the pixel arithmetic at nside <= 8192 (12 nside^2 < 2^30), where a 64-bit
// division costs a kernel several times as much
HX_PIX_HD long long div32(long long a, long long b) { return (long long)((uint32_t)a / (uint32_t)b); }

HX_PIX_HD int face_jrll(int face) { return 2 + (face >> 2); }
HX_PIX_HD int face_jpll(int face) { return face < 4 ? 2 * face + 1 : (face < 8 ? 2 * (face - 4) : 2 * (face - 8) + 1); }

// ---- RING pixel -> (ring 1 .. 4 nside - 1, index in the ring 0 .. n - 1), any nside in 1 .. 8192: the cap / belt / cap decode ----
HX_PIX_HD void pix2ring(long long nside, long long pix, long long *ir, long long *j)
{
    const long long npix = 12 * nside * nside, ncap = 2 * nside * (nside - 1), nl4 = 4 * nside;
    if (pix < ncap) {
        const long long iring = (1 + isqrt_ll(1 + 2 * pix)) >> 1;
        *ir = iring;
        *j = pix - 2 * iring * (iring - 1);
    } else if (pix < npix - ncap) {
        const long long ip = pix - ncap, tmp = div32(ip, nl4);
        *ir = tmp + nside;
        *j = ip - tmp * nl4;
    } else {
        const long long ip = npix - pix, irs = (1 + isqrt_ll(2 * ip - 1)) >> 1;
        *ir = nl4 - irs;
        *j = 4 * irs - (ip - 2 * irs * (irs - 1));
    }
}

// ---- face coordinates (healpix_cxx ring2xyf / xyf2ring without the power-of-two shifts), any nside in 1 .. 8192 ----
HX_PIX_HD void ring2xyf(long long nside, long long pix, int *face_out, long long *ix, long long *iy)
{
    long long iring, j, kshift, nr;
    int face;
    pix2ring(nside, pix, &iring, &j);
    const long long iphi = j + 1;
    if (iring < nside) {
        kshift = 0;
        nr = iring;
        face = (int)div32(j, nr);
    } else if (iring <= 3 * nside) {
        const long long tmp = iring - nside;
        kshift = (iring + nside) & 1;
        nr = nside;
        const long long ire = tmp + 1, irm = 2 * nside + 1 - tmp;
        const long long ifm = div32(iphi - (ire >> 1) + nside - 1, nside), ifp = div32(iphi - (irm >> 1) + nside - 1, nside);
        face = (int)((ifp == ifm) ? (ifp | 4) : ((ifp < ifm) ? ifp : (ifm + 8)));
    } else {
        kshift = 0;
        nr = 4 * nside - iring;
        face = (int)(8 + div32(j, nr));
    }
    const long long irt = iring - face_jrll(face) * nside + 1;
    long long ipt = 2 * iphi - face_jpll(face) * nr - kshift - 1;
    if (ipt >= 2 * nside) ipt -= 8 * nside;
    *face_out = face;
    *ix = (ipt - irt) >> 1;
    *iy = (-ipt - irt) >> 1;
}

HX_PIX_HD long long xyf2ring(long long nside, int face, long long ix, long long iy)
{
    const long long npix = 12 * nside * nside, ncap = 2 * nside * (nside - 1), nl4 = 4 * nside;
    const long long jr = (long long)face_jrll(face) * nside - ix - iy - 1;
    long long nr, n_before, kshift;
    if (jr < nside) { nr = jr; n_before = 2 * nr * (nr - 1); kshift = 0; }
    else if (jr > 3 * nside) { nr = nl4 - jr; n_before = npix - 2 * (nr + 1) * nr; kshift = 0; }
    else { nr = nside; n_before = ncap + (jr - nside) * nl4; kshift = (jr - nside) & 1; }
    long long jp = (face_jpll(face) * nr + ix - iy + 1 + kshift) / 2;
    if (jp > nl4) jp -= nl4;
    else if (jp < 1) jp += nl4;
    return n_before + jp - 1;
}

// (face, ix, iy) and offsets (u, v) in (0, 1) -> (lon, lat) in degrees: HEALPix's area-preserving face map (xyf2loc), lon in [0, 360).
HX_PIX_HD void xyf2lonlat(long long nside, int face, long long ix, long long iy, double u, double v, double *lon, double *lat)
{
    HX_PIX_NO_CONTRACT
    const double x = ((double)ix + u) / (double)nside, y = ((double)iy + v) / (double)nside;
    const double jr = ((double)face_jrll(face) - x) - y;
    double nr, z, sth;
    if (jr < 1.0) {
        nr = jr;
        const double t = nr * nr / 3.0;
        z = 1.0 - t;
        sth = sqrt(t * (2.0 - t));
    } else if (jr > 3.0) {
        nr = 4.0 - jr;
        const double t = nr * nr / 3.0;
        z = t - 1.0;
        sth = sqrt(t * (2.0 - t));
    } else {
        nr = 1.0;
        z = (2.0 - jr) * 2.0 / 3.0;
        sth = sqrt((1.0 - z) * (1.0 + z));
    }
    double tmp = ((double)face_jpll(face) * nr + x) - y;
    if (tmp < 0.0) tmp += 8.0;
    if (tmp >= 8.0) tmp -= 8.0;
    const double phi = 0.78539816339744830962 * tmp / nr;
    *lon = phi * 57.295779513082320877;
    *lat = atan2(z, sth) * 57.295779513082320877;
}

// ---- RING <-> NEST (healpix_cxx xyf2nest / nest2xyf around the two above), nside = 2^order <= 8192 ----
HX_PIX_HD long long spread_bits(long long v)  // bit b -> bit 2b (v < 2^16)
{
    v = (v | (v << 8)) & 0x00ff00ffll;
    v = (v | (v << 4)) & 0x0f0f0f0fll;
    v = (v | (v << 2)) & 0x33333333ll;
    v = (v | (v << 1)) & 0x55555555ll;
    return v;
}
HX_PIX_HD long long compress_bits(long long v)  // bit 2b -> bit b
{
    v &= 0x55555555ll;
    v = (v | (v >> 1)) & 0x33333333ll;
    v = (v | (v >> 2)) & 0x0f0f0f0fll;
    v = (v | (v >> 4)) & 0x00ff00ffll;
    v = (v | (v >> 8)) & 0x0000ffffll;
    return v;
}

HX_PIX_HD long long ring2nest(int order, long long pring)
{
    int face;
    long long ix, iy;
    ring2xyf(1ll << order, pring, &face, &ix, &iy);
    return ((long long)face << (2 * order)) + spread_bits(ix) + (spread_bits(iy) << 1);
}

HX_PIX_HD long long nest2ring(int order, long long pnest)
{
    const long long pf = pnest & ((1ll << (2 * order)) - 1);
    return xyf2ring(1ll << order, (int)(pnest >> (2 * order)), compress_bits(pf), compress_bits(pf >> 1));
}

// ---- ring geometry: ring ir in 1 .. 4 nside - 1, its pixels j in 0 .. n - 1 at phi = (j + 1 - shift) (pi / 2) / div (pix2ang of
// the HEALPix paper; sin(theta) of the cap rings from 1 - |z| directly) ----
struct Ring {
    long long first, n;  // first RING pixel, number of pixels
    double z, sth, shift, div;
};

HX_PIX_HD Ring ring_info(long long nside, long long ir)
{
    HX_PIX_NO_CONTRACT
    const long long npix = 12 * nside * nside, ncap = 2 * nside * (nside - 1);
    const double fact2 = 4.0 / (double)npix;
    Ring r;
    if (ir < nside) {
        const double t = (double)(ir * ir) * fact2;
        r.first = 2 * ir * (ir - 1);
        r.n = 4 * ir;
        r.z = 1.0 - t;
        r.sth = sqrt(t * (2.0 - t));
        r.shift = 0.5;
        r.div = (double)ir;
    } else if (ir <= 3 * nside) {
        const double zz = (double)(2 * nside - ir) * (2.0 / (3.0 * (double)nside));
        r.first = ncap + (ir - nside) * 4 * nside;
        r.n = 4 * nside;
        r.z = zz;
        r.sth = sqrt((1.0 - zz) * (1.0 + zz));
        r.shift = ((ir + nside) & 1) ? 1.0 : 0.5;
        r.div = (double)nside;
    } else {
        const long long irs = 4 * nside - ir;
        const double t = (double)(irs * irs) * fact2;
        r.first = npix - 2 * irs * (irs + 1);
        r.n = 4 * irs;
        r.z = t - 1.0;
        r.sth = sqrt(t * (2.0 - t));
        r.shift = 0.5;
        r.div = (double)irs;
    }
    return r;
}

HX_PIX_HD double ring_phi(const Ring &r, long long j)
{
    HX_PIX_NO_CONTRACT
    return ((double)(j + 1) - r.shift) * HALFPI / r.div;
}

HX_PIX_HD void ring_vec(const Ring &r, long long j, double *x, double *y, double *z)
{
    HX_PIX_NO_CONTRACT
    const double phi = ring_phi(r, j);
    *x = r.sth * cos(phi);
    *y = r.sth * sin(phi);
    *z = r.z;
}

// the (fractional) in-ring index at which the ring reaches phi: pixel j sits at j
HX_PIX_HD double ring_index_of_phi(const Ring &r, double phi)
{
    HX_PIX_NO_CONTRACT
    return phi * (r.div / HALFPI) - (1.0 - r.shift);
}

// the ring at or just above z (0 above the first ring), healpix's ring_above for any nside
HX_PIX_HD long long ring_above(long long nside, double z)
{
    HX_PIX_NO_CONTRACT
    const double az = fabs(z);
    if (az <= 2.0 / 3.0) return (long long)((double)nside * (2.0 - 1.5 * z));
    const long long ir = (long long)((double)nside * sqrt(3.0 * (1.0 - az)));
    return z > 0.0 ? ir : 4 * nside - ir - 1;
}

// unit vector of the centre of RING pixel pix, any nside in 1 .. 8192
HX_PIX_HD void pix2vec_ring(long long nside, long long pix, double *x, double *y, double *z)
{
    long long ir, j;
    pix2ring(nside, pix, &ir, &j);
    ring_vec(ring_info(nside, ir), j, x, y, z);
}

}  // namespace hxpix
