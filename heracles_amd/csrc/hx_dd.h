// hx_dd.h -- double-double arithmetic on the device: a value is h + l, |l| <= ulp(h) / 2.  Error-free transformations: every product and
// sum rounds on its own, so each function switches contraction off for itself.  Used by the Wigner-d recursion (hx_wigner.hip) and
// the node weights of the mixing matrices (hx_mixmat.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace hx {

struct DD {
    double h, l;
};
__device__ __forceinline__ DD dd_quick(double a, double b)
{
#pragma clang fp contract(off)
    const double s = a + b;
    return DD{s, b - (s - a)};
}
__device__ __forceinline__ DD dd_add(DD a, DD b)
{
#pragma clang fp contract(off)
    const double s = a.h + b.h, bb = s - a.h;
    const double e = ((a.h - (s - bb)) + (b.h - bb)) + (a.l + b.l);
    return dd_quick(s, e);
}
__device__ __forceinline__ DD dd_mul(DD a, DD b)
{
#pragma clang fp contract(off)
    const double p = a.h * b.h;
    const double e = fma(a.h, b.h, -p) + (a.h * b.l + a.l * b.h);
    return dd_quick(p, e);
}
__device__ __forceinline__ DD dd_neg(DD a) { return DD{-a.h, -a.l}; }
// sqrt of a positive double-double: one Newton step on the square root of the high part (r + (q - r^2) / (2 r), r^2 formed exactly)
__device__ __forceinline__ DD dd_sqrt(DD q)
{
#pragma clang fp contract(off)
    if (!(q.h > 0.0)) return DD{0.0, 0.0};
    const double r = sqrt(q.h), rr = r * r, re = fma(r, r, -rr);
    const double diff = ((q.h - rr) - re) + q.l;
    return dd_quick(r, diff / (2.0 * r));
}

}  // namespace hx
