// hx_jkregions.h -- the definition of the equal-weight sky segmentation as pure functions: the integer pixel
// weights, the order-preserving key of a projection, the weight target and the clamped count of a split, and the principal axis of a
// 3 x 3 covariance with its sign rule; the unit vector of a pixel centre, pix2vec_ring, is that of hx_healpix.h.  Usable from device
// code and from the host test (tests/csrc/test_jkregions.cpp), which runs the very code hx_jkregions.hip runs.  Compiles with plain g++.
#pragma once
#include <cmath>
#include <cstdint>

#include "hx_healpix.h"  // HX_PIX_HD, HX_PIX_NO_CONTRACT, pix2vec_ring

namespace hxjk {

using hxpix::pix2vec_ring;  // unit vector of the centre of a RING pixel

constexpr int NJK_MAX = 4096;
constexpr int NMOM = 10;  // S0, S1 (x, y, z), S2 (xx, xy, xz, yy, yz, zz)

HX_PIX_HD bool weight_valid(double w) { return w >= 0.0 && w <= 1.7976931348623157e308; }  // (a NaN fails both)

// q = max(1, llrint(w / wmax 2^32)) for 0 < w <= wmax: every later weight sum is an exact 64-bit integer
HX_PIX_HD uint64_t quantise(double w, double wmax)
{
    const long long r = llrint(w / wmax * 4294967296.0);
    return r < 1 ? 1ull : (uint64_t)r;
}

// order-preserving double -> 64-bit key of t + 0.0 (which maps -0 to +0): a < b  <=>  key(a) < key(b)
HX_PIX_HD uint64_t order_key(double t)
{
    const double u = t + 0.0;
    uint64_t b;
    __builtin_memcpy(&b, &u, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// T = floor(Q n1 / n) for Q < 2^63 and 0 < n1 < n <= 4096: long division in base 2^32, no 128-bit type
HX_PIX_HD uint64_t split_target(uint64_t Q, uint32_t n1, uint32_t n)
{
    uint64_t a = (Q >> 32) * n1, b = (Q & 0xffffffffull) * n1;  // Q n1 = a 2^32 + b
    a += b >> 32;
    b &= 0xffffffffull;
    const uint64_t qhi = a / n, r = a % n;
    const uint64_t qlo = ((r << 32) | b) / n;  // r < n <= 2^12: fits, and the quotient is below 2^32
    return (qhi << 32) + qlo;
}

// does the pixel with exclusive prefix E and weight q go left of the target T?  2 E + q <= 2 T
HX_PIX_HD bool goes_left(uint64_t E, uint64_t q, uint64_t T) { return 2ull * E + q <= 2ull * T; }

// the count of left pixels clamped to [n1, m - (n - n1)]: no region is left without a pixel (m >= n)
HX_PIX_HD uint32_t clamp_count(uint32_t c, uint32_t m, uint32_t n1, uint32_t n)
{
    const uint32_t lo = n1, hi = m - (n - n1);
    return c < lo ? lo : (c > hi ? hi : c);
}

// t = a . v, summed x, y, z in that order without fused multiply-adds
HX_PIX_HD double project(const double a[3], double x, double y, double z)
{
    HX_PIX_NO_CONTRACT
    return (a[0] * x + a[1] * y) + a[2] * z;
}

// C (xx, xy, xz, yy, yz, zz) = S2 / S0 - (S1 / S0)(S1 / S0)^T from the ten moments
HX_PIX_HD void covariance(const double mom[NMOM], double C[6])
{
    HX_PIX_NO_CONTRACT
    const double s0 = mom[0], mx = mom[1] / s0, my = mom[2] / s0, mz = mom[3] / s0;
    C[0] = mom[4] / s0 - mx * mx;
    C[1] = mom[5] / s0 - mx * my;
    C[2] = mom[6] / s0 - mx * mz;
    C[3] = mom[7] / s0 - my * my;
    C[4] = mom[8] / s0 - my * mz;
    C[5] = mom[9] / s0 - mz * mz;
}

// Unit eigenvector of the largest eigenvalue of the symmetric C (xx, xy, xz, yy, yz, zz), its component of largest magnitude (the
// first of equals) positive.  Cyclic Jacobi on C scaled to unit size, then one step of inverse iteration at the eigenvalue found,
// y = adj(C - lambda I) a: the adjugate of the (numerically singular) shifted matrix is its inverse without the common factor
// 1 / det, so the step needs no division and cannot overflow; it brings the error of a down to rounding / (relative gap).  With two
// (nearly) equal leading eigenvalues the axis is whatever the sweeps leave.
HX_PIX_HD void principal_axis(const double C[6], double a[3])
{
    HX_PIX_NO_CONTRACT
    double scale = 0.0;
    for (int k = 0; k < 6; ++k) scale = fabs(C[k]) > scale ? fabs(C[k]) : scale;
    if (!(scale > 0.0)) {
        a[0] = 1.0; a[1] = 0.0; a[2] = 0.0;
        return;
    }
    double A[3][3] = {{C[0] / scale, C[1] / scale, C[2] / scale}, {C[1] / scale, C[3] / scale, C[4] / scale}, {C[2] / scale, C[4] / scale, C[5] / scale}};
    const double M0[3][3] = {{A[0][0], A[0][1], A[0][2]}, {A[1][0], A[1][1], A[1][2]}, {A[2][0], A[2][1], A[2][2]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                const double app = A[p][p], aqq = A[q][q], apq = A[p][q];
                A[p][p] = app - t * apq;
                A[q][q] = aqq + t * apq;
                A[p][q] = A[q][p] = 0.0;
                const int r = 3 - p - q;
                const double arp = A[r][p], arq = A[r][q];
                A[r][p] = A[p][r] = c * arp - s * arq;
                A[r][q] = A[q][r] = s * arp + c * arq;
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int best = 0;
    if (A[1][1] > A[best][best]) best = 1;
    if (A[2][2] > A[best][best]) best = 2;
    double v[3] = {V[0][best], V[1][best], V[2][best]};
    // the eigenvalue as the Rayleigh quotient of the untouched matrix, then the inverse-iteration step
    double lam = 0.0;
    for (int i = 0; i < 3; ++i) lam += v[i] * (M0[i][0] * v[0] + M0[i][1] * v[1] + M0[i][2] * v[2]);
    const double m00 = M0[0][0] - lam, m11 = M0[1][1] - lam, m22 = M0[2][2] - lam, m01 = M0[0][1], m02 = M0[0][2], m12 = M0[1][2];
    const double j00 = m11 * m22 - m12 * m12, j01 = m02 * m12 - m01 * m22, j02 = m01 * m12 - m02 * m11;
    const double j11 = m00 * m22 - m02 * m02, j12 = m01 * m02 - m00 * m12, j22 = m00 * m11 - m01 * m01;
    const double y[3] = {j00 * v[0] + j01 * v[1] + j02 * v[2], j01 * v[0] + j11 * v[1] + j12 * v[2], j02 * v[0] + j12 * v[1] + j22 * v[2]};
    const double ny = sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
    if (ny > 1e-30 && ny == ny) {  // (a double leading eigenvalue leaves adj = 0: keep the Jacobi vector)
        v[0] = y[0] / ny; v[1] = y[1] / ny; v[2] = y[2] / ny;
    } else {
        const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        v[0] /= nv; v[1] /= nv; v[2] /= nv;
    }
    int big = 0;
    if (fabs(v[1]) > fabs(v[big])) big = 1;
    if (fabs(v[2]) > fabs(v[big])) big = 2;
    const double sgn = v[big] < 0.0 ? -1.0 : 1.0;
    a[0] = sgn * v[0]; a[1] = sgn * v[1]; a[2] = sgn * v[2];
}

}  // namespace hxjk
