// hx_lognormal.h -- the scalar pieces of hx_cl_nearest_psd (hx_lognormal.hip): the Jacobi rotation and the round-robin ordering of a
// sweep.  Pure functions, usable from device code and from the host test (tests/csrc/test_lognormal_host.cpp), which runs the very
// code the kernel runs.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define HX_LOGN_HD __host__ __device__ __forceinline__
#else
#define HX_LOGN_HD inline
#endif
#include <cmath>

namespace hxlogn {

// The rotation that zeroes a_pq of a symmetric matrix: J = [[c, s], [-s, c]] in the (p, q) plane, A' = J^T A J, with
//   tau = (a_qq - a_pp) / (2 a_pq),  t = sgn(tau) / (|tau| + sqrt(1 + tau^2))  (sgn(0) = +1: the smaller root, |t| <= 1),
//   c = 1 / sqrt(1 + t^2),  s = t c,  a'_pp = a_pp - t a_pq,  a'_qq = a_qq + t a_pq,
//   a'_rp = c a_rp - s a_rq,  a'_rq = s a_rp + c a_rq  (r != p, q); the columns p, q of the eigenvector matrix turn like a_rp, a_rq.
// a_pq = 0 gives the identity (c = 1, s = t = 0).  A tau that overflows gives t = 0, which is then the rounded answer.
struct Rotation {
    double c, s, t;
};

HX_LOGN_HD Rotation jacobi_rotation(double app, double aqq, double apq)
{
    Rotation r = {1.0, 0.0, 0.0};
    if (apq == 0.0) return r;
    const double tau = (aqq - app) / (2.0 * apq);
    const double at = fabs(tau);
    const double t = 1.0 / (at + sqrt(1.0 + at * at));
    r.t = tau < 0.0 ? -t : t;
    r.c = 1.0 / sqrt(1.0 + r.t * r.t);
    r.s = r.t * r.c;
    return r;
}

// Round-robin ordering of the pairs of n indices (the circle method): with m = n rounded up to even, a sweep has m - 1 steps of m / 2
// disjoint pairs each; index m - 1 stays put and the others turn by one place per step.  Pair k of step r is
//   k = 0: (r, m - 1);   k >= 1: ((r + k) mod (m - 1), (r - k) mod (m - 1)),
// returned with p < q.  For odd n the pair that holds the phantom index n is not a pair: the function returns false.  Every pair
// (p, q), p < q < n, is met exactly once per sweep.
HX_LOGN_HD int rr_steps(int n) { return ((n + 1) & ~1) - 1; }
HX_LOGN_HD int rr_pairs(int n) { return (n + 1) >> 1; }

HX_LOGN_HD bool rr_pair(int n, int step, int k, int *p, int *q)
{
    const int m1 = rr_steps(n);  // m - 1
    int a, b;
    if (k == 0) {
        a = step;
        b = m1;
    } else {
        a = step + k;
        if (a >= m1) a -= m1;
        b = step - k;
        if (b < 0) b += m1;
    }
    if (a > b) {
        const int x = a;
        a = b;
        b = x;
    }
    *p = a;
    *q = b;
    return b < n && a != b;
}

}  // namespace hxlogn
