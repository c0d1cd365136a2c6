// hx_masktools.h -- the definition of the mask tools as pure functions: the chord measure
// h = 1 - cos(angle) between two unit vectors, the rings and the conservative phi window of a disc, the same for a convex spherical
// polygon with its orientation, validity and inside test, the per-ring neighbour tables of a
// mask and the pruned search for the nearest masked pixel over them, and the C1 / C2 tapers, all on the ring geometry of hx_healpix.h
// (Ring).  Usable from device code and from the host test (tests/csrc/test_masktools.cpp), which runs the very code
// hx_masktools.hip runs.  Compiles with plain g++.
#pragma once
#include <cmath>
#include <cstdint>

#include "hx_healpix.h"  // the geometry of a ring and of its pixel centres

// tests/csrc/test_masktools.cpp includes this header alone and compares ring_vec with the pixel centre under the name hx_jkregions.h
// gives it; repeated here so that the mask tools need not include the jackknife header for it
namespace hxjk {
using hxpix::pix2vec_ring;
}

namespace hxmask {

using hxpix::HALFPI;
using hxpix::Ring;
using hxpix::pix2ring;
using hxpix::ring_above;
using hxpix::ring_index_of_phi;
using hxpix::ring_info;
using hxpix::ring_phi;
using hxpix::ring_vec;

constexpr uint32_t NONE = 0xffffffffu;  // "no masked pixel" in the neighbour tables
constexpr double DEG = 0.017453292519943295, PI = 3.14159265358979323846, TWOPI = 6.28318530717958647692;
constexpr int KIND_C1 = 1, KIND_C2 = 2;
constexpr double WIDE_MIN = 512.0;  // discs with more pixels than this (estimated) get a work-group of their own

HX_PIX_HD bool finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }  // (a NaN fails both)
HX_PIX_HD bool is_masked(double m) { return m <= 0.0; }

// h(u, v) = 1 - cos(angle between u and v) in the chord form, summed x, y, z in that order
HX_PIX_HD double chord_h(double ux, double uy, double uz, double vx, double vy, double vz)
{
    HX_PIX_NO_CONTRACT
    const double dx = ux - vx, dy = uy - vy, dz = uz - vz;
    return 0.5 * ((dx * dx + dy * dy) + dz * dz);
}

// h of an angle in degrees: 2 sin^2(angle / 2)
HX_PIX_HD double angle_h(double deg)
{
    HX_PIX_NO_CONTRACT
    const double s = sin(0.5 * (deg * DEG));
    return 2.0 * s * s;
}

// ---- discs ----
struct Disc {
    double x, y, z;  // the centre
    double s, phi;   // cos(lat), the longitude of the centre in [0, 2 pi)
    double theta, rad, hr;  // colatitude and radius in radians, h(radius)
};

HX_PIX_HD bool disc_valid(double lon, double lat, double radius)
{
    return finite(lon) && lat >= -90.0 && lat <= 90.0 && radius >= 0.0 && radius <= 180.0;  // (a NaN fails)
}

HX_PIX_HD Disc make_disc(double lon, double lat, double radius)
{
    HX_PIX_NO_CONTRACT
    const double lo = lon * DEG, la = lat * DEG;
    Disc d;
    d.s = cos(la);
    d.z = sin(la);
    d.x = d.s * cos(lo);
    d.y = d.s * sin(lo);
    d.phi = atan2(d.y, d.x);
    if (d.phi < 0.0) d.phi += TWOPI;
    d.theta = (90.0 - lat) * DEG;
    d.rad = radius * DEG;
    d.hr = angle_h(radius);
    return d;
}

// an estimate of the number of pixel centres in the disc: the area of the cap in pixels
HX_PIX_HD double disc_pixels(long long nside, double hr) { return 6.0 * (double)nside * (double)nside * hr; }

HX_PIX_HD bool disc_has_pole(const Disc &d) { return d.theta - d.rad <= 0.0 || d.theta + d.rad >= PI; }

// the rings whose colatitude lies within the radius of the centre's, widened by a ring or two: lo .. hi inclusive
HX_PIX_HD void disc_rings(long long nside, const Disc &d, long long *lo, long long *hi)
{
    const double tlo = d.theta - d.rad, thi = d.theta + d.rad;
    const double zhi = tlo <= 0.0 ? 1.0 : cos(tlo), zlo = thi >= PI ? -1.0 : cos(thi);
    long long a = ring_above(nside, zhi) - 1, b = ring_above(nside, zlo) + 2;
    const long long last = 4 * nside - 1;
    a = a < 1 ? 1 : (a > last ? last : a);
    b = b < 1 ? 1 : (b > last ? last : b);
    *lo = a;
    *hi = b;
}

// The conservative phi window of the disc on ring r: the in-ring indices k0 .. k0 + count - 1, to be taken modulo r.n (k0 may be
// negative); count == r.n is the whole ring.  From the cap formula in its chord form, 2 sin^2(dphi / 2) <= (h(radius) - hlow) /
// (sin(theta_r) sin(theta_c)) with hlow the chord between the two colatitudes: widened by at least one pixel each side; the whole
// ring where the cap holds a pole or the right-hand side reaches 2; a negative right-hand side (no pixel of the ring qualifies, up
// to rounding) leaves the widening alone.  The window only prunes: disc_hit decides every pixel.
struct Window {
    long long k0, count;
};

HX_PIX_HD Window disc_window(const Ring &r, const Disc &d)
{
    HX_PIX_NO_CONTRACT
    Window w = {0, r.n};
    if (disc_has_pole(d)) return w;
    const double ss = r.sth * d.s;
    if (!(ss > 0.0)) return w;
    const double ds = r.sth - d.s, dz = r.z - d.z;
    double B = (d.hr - 0.5 * (ds * ds + dz * dz)) / ss;
    if (B >= 2.0) return w;
    if (!(B > 0.0)) B = 0.0;
    const double scale = r.div / HALFPI, half = 2.0 * asin(sqrt(0.5 * B)) * scale;
    const double tc = ring_index_of_phi(r, d.phi);
    const long long k0 = (long long)floor(tc - half) - 1, k1 = (long long)ceil(tc + half) + 1;
    if (k1 - k0 + 1 >= r.n) return w;
    w.k0 = k0;
    w.count = k1 - k0 + 1;
    return w;
}

HX_PIX_HD long long wrap_index(long long k, long long n)
{
    const long long j = k % n;
    return j < 0 ? j + n : j;
}

// the rule: is the centre of pixel j of ring r inside the disc?
HX_PIX_HD bool disc_hit(const Ring &r, long long j, const Disc &d)
{
    double x, y, z;
    ring_vec(r, j, &x, &y, &z);
    return chord_h(x, y, z, d.x, d.y, d.z) <= d.hr;
}

// ---- convex polygons ----
// A polygon is a cyclic list of POLY_MIN .. POLY_MAX vertices, its edges the minor great-circle arcs between consecutive ones.  The
// vertices travel as v [3 n] (x, y, z of each), the edges as Edge [n]: edge k runs from vertex k to vertex k + 1.
constexpr int POLY_MIN = 3, POLY_MAX = 64;

HX_PIX_HD bool count_valid(long long n) { return n >= POLY_MIN && n <= POLY_MAX; }
HX_PIX_HD bool vertex_valid(double lon, double lat) { return finite(lon) && lat >= -90.0 && lat <= 90.0; }  // (a NaN fails)

// the unit vector of (lon, lat) in degrees, by the operations of make_disc: the bits of a disc's centre
HX_PIX_HD void make_vertex(double lon, double lat, double *v)
{
    HX_PIX_NO_CONTRACT
    const double lo = lon * DEG, la = lat * DEG, s = cos(la);
    v[0] = s * cos(lo);
    v[1] = s * sin(lo);
    v[2] = sin(la);
}

// n = v x w, unnormalised: each component the difference of two products in the written order
HX_PIX_HD void edge_normal(const double *v, const double *w, double *n)
{
    HX_PIX_NO_CONTRACT
    n[0] = v[1] * w[2] - v[2] * w[1];
    n[1] = v[2] * w[0] - v[0] * w[2];
    n[2] = v[0] * w[1] - v[1] * w[0];
}

// d(u, e) = (n_x u_x + n_y u_y) + n_z u_z
HX_PIX_HD double edge_d(double nx, double ny, double nz, double ux, double uy, double uz)
{
    HX_PIX_NO_CONTRACT
    return (nx * ux + ny * uy) + nz * uz;
}

// Orientation and validity: sigma = +1 if d(v_2, e_0) > 0, else -1; valid iff sigma d(v_k, e) > 0 for every edge e and every vertex k
// that is not one of its two endpoints -- no repeated vertex, no collinear triple, no reflex vertex, no antipodal neighbours.
HX_PIX_HD bool poly_valid(int n, const double *v, int *sigma)
{
    double m[3];
    edge_normal(v, v + 3, m);
    const double sg = edge_d(m[0], m[1], m[2], v[6], v[7], v[8]) > 0.0 ? 1.0 : -1.0;
    *sigma = sg > 0.0 ? 1 : -1;
    for (int e = 0; e < n; ++e) {
        const int e1 = e + 1 < n ? e + 1 : 0;
        edge_normal(v + 3 * e, v + 3 * e1, m);
        for (int k = 0; k < n; ++k) {
            if (k == e || k == e1) continue;
            if (!(sg * edge_d(m[0], m[1], m[2], v[3 * k], v[3 * k + 1], v[3 * k + 2]) > 0.0)) return false;
        }
    }
    return true;
}

// An edge as the kernels use it: sigma n_e (a change of sign is exact in every operation of d: d(u, sigma n) = sigma d(u, n) bit for
// bit), and for the phi windows rho = sqrt(n_x^2 + n_y^2) and phi = atan2(sigma n_y, sigma n_x) in [0, 2 pi)
struct Edge {
    double x, y, z, rho, phi;
};

HX_PIX_HD Edge make_edge(const double *v, const double *w, int sigma)
{
    HX_PIX_NO_CONTRACT
    double m[3];
    edge_normal(v, w, m);
    const double sg = sigma > 0 ? 1.0 : -1.0;
    Edge e;
    e.x = sg * m[0];
    e.y = sg * m[1];
    e.z = sg * m[2];
    e.rho = sqrt(e.x * e.x + e.y * e.y);
    e.phi = atan2(e.y, e.x);
    if (e.phi < 0.0) e.phi += TWOPI;
    return e;
}

// the rule: is the centre of pixel j of ring r inside the polygon?  sigma d(v_p, e) >= 0 for every edge
HX_PIX_HD bool poly_hit(const Ring &r, long long j, int n, const Edge *e)
{
    double x, y, z;
    ring_vec(r, j, &x, &y, &z);
    for (int k = 0; k < n; ++k)
        if (!(edge_d(e[k].x, e[k].y, e[k].z, x, y, z) >= 0.0)) return false;
    return true;
}

// a disc from a unit vector and an h instead of degrees; theta from atan2(sin, cos), the radius from the chord
HX_PIX_HD Disc disc_of_vec(double x, double y, double z, double h)
{
    HX_PIX_NO_CONTRACT
    Disc d;
    d.x = x;
    d.y = y;
    d.z = z;
    d.s = sqrt(x * x + y * y);
    d.phi = atan2(y, x);
    if (d.phi < 0.0) d.phi += TWOPI;
    d.theta = atan2(d.s, z);
    d.hr = h;
    d.rad = h >= 2.0 ? PI : 2.0 * asin(sqrt(0.5 * h));
    return d;
}

// The bounding cap: c = sum of the vertices, normalised, h_cap = max_k h(c, v_k).  For h_cap < 1 (a radius below 90 degrees) the cap
// is geodesically convex and holds the vertices, hence the polygon: true, and *cap is that disc.  Else, or where the sum vanishes:
// false, cap->hr = 2 (the whole sphere), and every ring and the whole ring are to be scanned.
HX_PIX_HD bool poly_cap(int n, const double *v, Disc *cap)
{
    HX_PIX_NO_CONTRACT
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = 0; k < n; ++k) {
        sx += v[3 * k];
        sy += v[3 * k + 1];
        sz += v[3 * k + 2];
    }
    const double norm = sqrt((sx * sx + sy * sy) + sz * sz);
    double h = 2.0;
    if (norm > 0.0) {
        sx /= norm;
        sy /= norm;
        sz /= norm;
        h = 0.0;
        for (int k = 0; k < n; ++k) {
            const double hk = chord_h(sx, sy, sz, v[3 * k], v[3 * k + 1], v[3 * k + 2]);
            h = hk > h ? hk : h;
        }
    } else {
        sx = sy = 0.0;
        sz = 1.0;
    }
    if (!(h < 1.0)) {
        *cap = disc_of_vec(sx, sy, sz, 2.0);
        return false;
    }
    *cap = disc_of_vec(sx, sy, sz, h);
    return true;
}

// the rings to scan: those of the bounding cap, or all of them
HX_PIX_HD void poly_rings(long long nside, bool capped, const Disc &cap, long long *lo, long long *hi)
{
    if (capped) {
        disc_rings(nside, cap, lo, hi);
    } else {
        *lo = 1;
        *hi = 4 * nside - 1;
    }
}

// The phi window of the polygon on ring r (z, s = sin theta): the window of the bounding cap, clipped by the edges.  Edge e admits
// cos(phi - phi_e) >= t = -sigma n_z z / (s rho): the whole ring for t <= -1 (and where s rho = 0: no clipping), else the arc of half
// width acos(min(t, 1)) around phi_e, widened here by one pixel each side.  The window is kept as one interval (lo, len) in in-ring
// indices and cut by one arc after the other; where a cut would leave two intervals (possible on rings near a pole, and where the
// long edges of a strip meet a ring twice) their hull within the current interval -- the current interval -- is kept, and the
// edges are gone over once more, since an arc that split the wide window of the cap may cut the narrower one the other edges
// left in one piece (cutting twice by the same arc changes nothing).  An empty intersection gives count 0.  The window only prunes: poly_hit decides every pixel.
HX_PIX_HD Window poly_window(const Ring &r, bool capped, const Disc &cap, int n, const Edge *e)
{
    HX_PIX_NO_CONTRACT
    Window w = {0, r.n};
    if (capped) w = disc_window(r, cap);
    const double nn = (double)r.n, scale = r.div / HALFPI;
    bool whole = w.count >= r.n;
    double lo = (double)w.k0, len = (double)(w.count - 1);
    for (int pass = 0; pass < 2; ++pass) {
        bool again = false;
        for (int k = 0; k < n; ++k) {
            const double sr = r.sth * e[k].rho;
            if (!(sr > 0.0)) continue;
            const double t = -(e[k].z * r.z) / sr;
            if (!(t > -1.0)) continue;
            const double half = (t >= 1.0 ? 0.0 : acos(t)) * scale + 1.0, blen = 2.0 * half;
            if (blen >= nn) continue;
            const double bstart = ring_index_of_phi(r, e[k].phi) - half;
            if (whole) {
                lo = bstart;
                len = blen;
                whole = false;
                continue;
            }
            double delta = fmod(bstart - lo, nn);
            if (delta < 0.0) delta += nn;
            const bool head = delta <= len, tail = delta + blen >= nn;  // the arc from its start on; the part of it that wrapped round
            if (head && tail) {
                again = true;
                continue;
            }
            if (head) {
                const double end = delta + blen < len ? delta + blen : len;
                lo += delta;
                len = end - delta;
            } else if (tail) {
                const double end = delta + blen - nn;
                len = end < len ? end : len;
            } else {
                w.k0 = 0;
                w.count = 0;
                return w;
            }
        }
        if (!again) break;
    }
    w.k0 = 0;
    w.count = r.n;
    if (whole) return w;
    const long long k0 = (long long)floor(lo), k1 = (long long)ceil(lo + len);
    if (k1 - k0 + 1 >= r.n) return w;
    w.k0 = k0;
    w.count = k1 - k0 + 1;
    return w;
}

// ---- the neighbour tables of a mask ----
// left[p]: the in-ring index of the nearest masked pixel at or before p on p's ring, right[p]: at or after p (NONE: there is none on
// that side); first / last [ring]: the first and the last masked index of the ring (NONE: the ring has no masked pixel), for the
// wrap-around.  One ring, in order (the device builds the same tables with a scan per ring):
HX_PIX_HD void ring_neighbours(const double *mask, const Ring &r, uint32_t *left, uint32_t *right, uint32_t *first, uint32_t *last)
{
    uint32_t seen = NONE;
    *first = NONE;
    for (long long j = 0; j < r.n; ++j) {
        if (is_masked(mask[r.first + j])) {
            seen = (uint32_t)j;
            if (*first == NONE) *first = seen;
        }
        left[r.first + j] = seen;
    }
    *last = seen;
    seen = NONE;
    for (long long j = r.n - 1; j >= 0; --j) {
        if (is_masked(mask[r.first + j])) seen = (uint32_t)j;
        right[r.first + j] = seen;
    }
}

struct Neighbours {
    const uint32_t *left, *right;   // [npix]
    const uint32_t *first, *last;   // [4 nside], indexed by ring
};

// H of the unmasked pixel pix: min(cap, min over masked q of h(v_pix, v_q)).  The rings are walked outward from the pixel's own, north
// then south; on a ring the nearest masked pixel is the nearest at or before the pixel nearest in phi or the nearest at or after it
// (h to a fixed point is monotone in |dphi| on either side), each with its wrap-around; a direction stops at the first ring whose
// lower bound -- the chord between the two colatitudes, monotone in the ring offset -- reaches the best value so far (which starts
// at the cap).  evals, unless null, counts the evaluations of h.
HX_PIX_HD double nearest_h(long long nside, long long pix, double cap, const Neighbours &nb, unsigned long long *evals)
{
    HX_PIX_NO_CONTRACT
    long long ir0, j0;
    pix2ring(nside, pix, &ir0, &j0);
    const Ring r0 = ring_info(nside, ir0);
    const double pphi = ring_phi(r0, j0);
    double px, py, pz;
    ring_vec(r0, j0, &px, &py, &pz);
    const long long last = 4 * nside - 1;
    double best = cap;
    for (int dir = 0; dir < 2; ++dir) {
        const long long step = dir == 0 ? -1 : 1;
        for (long long ir = dir == 0 ? ir0 : ir0 + 1; ir >= 1 && ir <= last; ir += step) {
            const Ring r = ring_info(nside, ir);
            const double ds = r0.sth - r.sth, dz = r0.z - r.z;
            if (0.5 * (ds * ds + dz * dz) >= best) break;
            const uint32_t f = nb.first[ir];
            if (f == NONE) continue;
            const long long jn = wrap_index((long long)floor(ring_index_of_phi(r, pphi) + 0.5), r.n);
            uint32_t L = nb.left[r.first + jn], R = nb.right[r.first + jn];
            if (L == NONE) L = nb.last[ir];
            if (R == NONE) R = f;
            double x, y, z;
            ring_vec(r, (long long)L, &x, &y, &z);
            double h = chord_h(px, py, pz, x, y, z);
            best = h < best ? h : best;
            if (evals) ++*evals;
            if (R != L) {
                ring_vec(r, (long long)R, &x, &y, &z);
                h = chord_h(px, py, pz, x, y, z);
                best = h < best ? h : best;
                if (evals) ++*evals;
            }
        }
    }
    return best;
}

// ---- tapers: w(x) on x = sqrt(H / h(aposize)) in [0, 1], w(0) = 0, w(1) = 1 ----
HX_PIX_HD bool kind_valid(int kind) { return kind == KIND_C1 || kind == KIND_C2; }

HX_PIX_HD double taper(int kind, double x)
{
    HX_PIX_NO_CONTRACT
    if (x >= 1.0) return 1.0;
    if (!(x > 0.0)) return 0.0;
    return kind == KIND_C1 ? x - sin(TWOPI * x) / TWOPI : 0.5 * (1.0 - cos(PI * x));
}

HX_PIX_HD double taper_of_h(int kind, double H, double hcap) { return taper(kind, sqrt(H / hcap)); }

}  // namespace hxmask
