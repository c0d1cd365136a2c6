// hx_wigner.hip -- Gauss-Legendre nodes and Wigner-d tables d^l_{ab}(x_k) in double-double, and what is kept of them between calls
// (hx_wigner.h).  The tables feed the mixing matrices (hx_mixmat.hip), the Cl <-> xi columns of any spin weight (hx_transforms.hip,
// hx_xi_cols.hip) and the polar tables of the point transform (hx_nufft.hip).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hx_dd.h"
#include "hx_wigner.h"

namespace hx {

// ---- Gauss-Legendre nodes: Newton on P_n, one thread per node pair ---------------------
// xlo (may be null): the part of every node that a double cannot hold -- node = x + xlo, xlo = -P_n(x) / P_n'(x) at the converged
// double, accurate to ~1 % (P_n(x) ~ P_n' * 1e-16 stands well above the rounding noise of its recurrence).  The mixing-matrix tables
// need it: next to the poles d^l(x)' ~ l^2 / 2, so rounding a node to a double shifts d^l there by l^2 / 2 * 5e-17 ~ 1e-9 for l = 6000,
// coherently over all l of a table -- 2.7e-10 on the diagonal of the L = 4096 matrix of a mask whose correlation function peaks at
// theta = 0 (found by tests/test_gpu_mixmat.py::test_mixmat_blocks_at_high_l_vs_3j; the weights are good to 1e-16 as they are).
__global__ void k_gauss_legendre(int n, double *__restrict__ x, double *__restrict__ w, double *__restrict__ xlo)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (n + 1) / 2) return;
    double t = cospi((i + 0.75) / (n + 0.5));
    double dp = 1.0, tl = 0.0, pn = 0.0, om = 1.0;
    for (int it = 0; it < 10; ++it) {
        double p0 = 1.0, p1 = t;
        for (int k = 2; k <= n; ++k) {
            double p2 = ((2.0 * k - 1.0) * t * p1 - (k - 1.0) * p0) / k;
            p0 = p1;
            p1 = p2;
        }
        dp = n * (t * p1 - p0) / (t * t - 1.0);
        double dt = p1 / dp;
        t -= dt;
        // (|t| <= 1: an absolute threshold.  Relative to |t| the nodes next to 0 never met it and every thread ran all ten O(n) sweeps:
        // 7.7 ms of the L = 6144 build; converged Newton steps do not move the node any more)
        if (fabs(dt) <= 4e-16) break;
    }
    {
        // P_n at the converged node in double-double: in plain doubles the value (~ P_n' x 1e-16) drowns in the rounding noise of the
        // recurrence (~ n x 1e-16) everywhere but next to the poles, and a correction made of noise is worse than none
#pragma clang fp contract(off)  // (error-free transformations: every product and sum below rounds on its own)
        double ph0 = 1.0, pl0 = 0.0, ph1 = t, pl1 = 0.0;
        for (int k = 2; k <= n; ++k) {
            const double a = 2.0 * k - 1.0, b = k - 1.0;
            // u = t * p1 (dd x double), v = a * u, w = b * p0, d = v - w, p2 = d / k
            double uh = ph1 * t, ul = fma(ph1, t, -uh) + pl1 * t;
            double vh = uh * a, vl = fma(uh, a, -vh) + ul * a;
            double wh = ph0 * b, wl = fma(ph0, b, -wh) + pl0 * b;
            double sh = vh - wh, bb = sh - vh, sl = (vh - (sh - bb)) + (-wh - bb);  // two_sum(vh, -wh)
            sl += vl - wl;
            double dh = sh + sl, dl = sl - (dh - sh);                              // quick_two_sum
            const double q1 = dh / k, r = fma(-q1, (double)k, dh), q2 = (r + dl) / k;
            ph0 = ph1; pl0 = pl1;
            ph1 = q1 + q2; pl1 = q2 - (ph1 - q1);
        }
        // (1 - t^2 as (1 - t)(1 + t): t * t - 1 loses 7e-10 of its value next to the poles, and the weights with it)
        om = (1.0 - t) * (1.0 + t);
        dp = -n * (t * ph1 - ph0) / om;
        pn = ph1 + pl1;
        tl = -pn / dp;
    }
    // the weight belongs to the node t + tl: evaluated at the rounded t it is off by up to 6e-10 next to the poles
    // (d ln w / dx = -2 x / (1 - x^2)); P_n'(t + tl) = P_n' + tl P_n'' with (1 - t^2) P_n'' = 2 t P_n' - n (n + 1) P_n
    const double dps = dp + tl * (2.0 * t * dp - (double)n * (n + 1.0) * pn) / om;
    const double ww = 2.0 / ((om - 2.0 * t * tl) * dps * dps);
    if ((n & 1) && i == n / 2) { t = 0.0; tl = 0.0; }
    x[i] = -t; x[n - 1 - i] = t;
    w[i] = ww; w[n - 1 - i] = ww;
    if (xlo) { xlo[i] = -tl; xlo[n - 1 - i] = tl; }
}

// ---- Wigner-d tables: out[l * sl + k * sk] = d^l_{ab}(x_k), l = 0 .. lmax, in double-double arithmetic -------------------------------
// coef[l]: d^{l+1} = (c1x x + c1c) d^l - c2 d^{l-1}
// At l ~ 4000-6000 a table value next to the poles carries ~l^1.5 x 1e-16 of rounding noise from the upward recurrence (every
// step's rounding error is carried on by a solution that grows like l there), and the noise is alike for the ~100 polar nodes,
// which carry the whole integrand when the mask's correlation function peaks at theta = 0: 5e-11 on a diagonal element of 10.8 at
// L = 4096 (with exact nodes and weights; tests/test_gpu_mixmat.py::test_mixmat_blocks_at_high_l_vs_3j).  In double-double the noise is
// ~1e-32 l^1.5; the coefficients come as (hi, lo) pairs from the host's long doubles, the node as x + xlo.  One thread per node, a
// dependent chain of ~16 operations per step: ~0.4 ms per table at L = 6144, once per context (measured: 2.1 ms per table under rocprofv3, profiles/r06_kernel_stats.csv).
struct WigCoefDD {
    double c1xh, c1xl, c1ch, c1cl, c2h, c2l;
};
// The seed d^{l0}_{ab} of the recursion for any (a, b), from the host (wigner_seed): with (A, B) the pair brought to A >= |B| by
// d_{ab} = (-1)^{a-b} d_{ba} = d_{-b,-a} and sg the sign that took it there,
//   d^A_{AB}(x) = sqrt((2A)! / ((A+B)! (A-B)!)) ((1+x)/2)^{(A+B)/2} ((1-x)/2)^{(A-B)/2},
// pp = A + B, pm = A - B (both even or both odd), c = the square root of the binomial as (hi, lo).
struct WigSeed {
    int pp, pm;
    double ch, cl, sg;
    int general;  // 1: take the general seed also for the pairs that have a branch of their own (test hook)
};
__device__ __forceinline__ DD wigner_seed_dd(const WigSeed sd, DD op, DD om)
{
    const DD hp = DD{0.5 * op.h, 0.5 * op.l}, hm = DD{0.5 * om.h, 0.5 * om.l};
    DD v = DD{1.0, 0.0};
    for (int i = 0; i < sd.pp / 2; ++i) v = dd_mul(v, hp);
    for (int i = 0; i < sd.pm / 2; ++i) v = dd_mul(v, hm);
    if (sd.pp & 1) v = dd_mul(v, dd_sqrt(dd_mul(hp, hm)));  // (pp and pm are odd together: one factor sqrt((1 - x^2) / 4))
    v = dd_mul(DD{sd.ch, sd.cl}, v);
    return DD{sd.sg * v.h, sd.sg * v.l};
}
// out[l * sl + k * sk] = d^l_{ab}(x_k + xlo_k), l = 0..lmax; s6: sqrt(6) / 4 as (hi, lo)
__global__ void k_wigner_table_dd(int lmax, int a, int b, int n, const double *__restrict__ x, const double *__restrict__ xlo,
                                  const WigCoefDD *__restrict__ coef, double *__restrict__ out, long long sl, long long sk, double s6h,
                                  double s6l, WigSeed sd)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const DD xx = dd_quick(x[k], xlo[k]);
    const DD one = DD{1.0, 0.0};
    const DD om = dd_add(one, dd_neg(xx)), op = dd_add(one, xx);
    const int l0 = max(abs(a), abs(b));
    DD d0;
    if (sd.general) d0 = wigner_seed_dd(sd, op, om);
    else if (a == 0 && b == 0) d0 = one;
    else if (a == 2 && b == 0) d0 = dd_mul(DD{s6h, s6l}, dd_mul(om, op));
    else if (a == 2 && b == 2) { d0 = dd_mul(op, op); d0.h *= 0.25; d0.l *= 0.25; }
    else if (a == 1 && b == 1) { d0 = op; d0.h *= 0.5; d0.l *= 0.5; }     // d^1_{11}   (heracles/transforms.py:68-73)
    else if (a * b == -1) { d0 = om; d0.h *= 0.5; d0.l *= 0.5; }          // d^1_{-1,1} = d^1_{1,-1}
    else if (a == 2 && b == -2) { d0 = dd_mul(om, om); d0.h *= 0.25; d0.l *= 0.25; }
    else d0 = wigner_seed_dd(sd, op, om);
    for (int l = 0; l < l0 && l <= lmax; ++l) out[l * sl + k * sk] = 0.0;
    if (l0 > lmax) return;
    DD dp = DD{0.0, 0.0}, dc = d0;
    out[l0 * sl + k * sk] = dc.h + dc.l;
    for (int l = l0; l < lmax; ++l) {
        const WigCoefDD c = coef[l];
        const DD t = dd_add(dd_mul(DD{c.c1xh, c.c1xl}, xx), DD{c.c1ch, c.c1cl});
        const DD dn = dd_add(dd_mul(t, dc), dd_neg(dd_mul(DD{c.c2h, c.c2l}, dp)));
        dp = dc;
        dc = dn;
        out[(l + 1) * sl + k * sk] = dc.h + dc.l;
    }
}

// ---- host helpers --------------------------------------------------------------------
static void wigner_coefs_dd(int lmax, int a, int b, std::vector<WigCoefDD> &c)
{
    c.assign(lmax + 1, WigCoefDD{0, 0, 0, 0, 0, 0});
    auto split = [](long double v, double &h, double &l) {
        h = (double)v;
        l = (double)(v - (long double)h);
    };
    for (int l = 0; l <= lmax; ++l) {
        if (l == 0) { c[l].c1xh = 1.0; continue; }
        long double dl = l, lp = l + 1.0L;
        long double den = dl * sqrtl((lp * lp - (long double)a * a) * (lp * lp - (long double)b * b));
        if (den == 0.0L) continue;
        split((2 * dl + 1) * dl * lp / den, c[l].c1xh, c[l].c1xl);
        split(-(2 * dl + 1) * (long double)a * b / den, c[l].c1ch, c[l].c1cl);
        split(lp * sqrtl((dl * dl - (long double)a * a) * (dl * dl - (long double)b * b)) / den, c[l].c2h, c[l].c2l);
    }
}

// (a, b) brought to A >= |B|, A >= 0 by d_{ab} = (-1)^{a-b} d_{ba} = d_{-b,-a}; returns the sign that took it there
static double wigner_normal_pair(int a, int b, int &A, int &B)
{
    const double flip = ((a - b) & 1) ? -1.0 : 1.0;
    if (abs(a) >= abs(b)) {
        if (a >= 0) { A = a; B = b; return 1.0; }
        A = -a; B = -b;
        return flip;
    }
    if (b > 0) { A = b; B = a; return flip; }
    A = -b; B = -a;
    return 1.0;
}
// the seed of k_wigner_table_dd for any (a, b), max(|a|, |b|) <= HX_MAX_MIX_SPIN: the binomial (2A over A+B) <= (64 over 32) < 2^63 is
// formed in integers, its root in the host's long double and handed over as (hi, lo), like sqrt(6) / 4 of the (2,0) branch
static WigSeed wigner_seed(int a, int b)
{
    WigSeed sd;
    int A, B;
    sd.sg = wigner_normal_pair(a, b, A, B);
    sd.pp = A + B;
    sd.pm = A - B;
    unsigned __int128 bin = 1;
    for (int i = 1; i <= sd.pm; ++i) bin = bin * (unsigned)(sd.pp + i) / (unsigned)i;
    const long double c = sqrtl((long double)bin);  // (not through 64 bits: C(2A, A) passes 2^64 at A = 34, the polar tables of hx_nufft.hip go to 56)
    sd.ch = (double)c;
    sd.cl = (double)(c - (long double)sd.ch);
    const char *e = getenv("HX_WIGNER_SEED");
    sd.general = e && !strcmp(e, "general");
    return sd;
}
// out[l * sl + k * sk] = d^l_{ab}(x_k + xlo_k), l = 0 .. lmax, on the stream of the library
static int launch_wigner_table(int lmax, int a, int b, int n, const double *d_x, const double *d_xlo, const WigCoefDD *d_coef, double *d_out,
                               long long sl, long long sk)
{
    ProfScope ps("wigner_tables");
    const long double s6 = sqrtl(6.0L) / 4.0L;
    const double s6h = (double)s6, s6l = (double)(s6 - (long double)s6h);
    hipLaunchKernelGGL(k_wigner_table_dd, dim3((n + 63) / 64), dim3(64), 0, rt().stream, lmax, a, b, n, d_x, d_xlo, d_coef, d_out, sl, sk, s6h, s6l,
                       wigner_seed(a, b));
    HX_HIP(hipGetLastError());
    return HX_OK;
}

int launch_gauss_legendre(int n, double *d_x, double *d_w, double *d_xlo)
{
    const int half = (n + 1) / 2;
    hipLaunchKernelGGL(k_gauss_legendre, dim3((half + 63) / 64), dim3(64), 0, rt().stream, n, d_x, d_w, d_xlo);
    HX_HIP(hipGetLastError());
    return HX_OK;
}

// The normalisation under which pairs share a table, and one table by the kernel above in the caller's layout (hx_wigner.h).
double wigner_pair_normalise(int a, int b, int *A, int *B) { return wigner_normal_pair(a, b, *A, *B); }
int wigner_table_build(int lmax, int a, int b, int n, const double *d_x, const double *d_xlo, double *d_out, long long sl, long long sk)
{
    std::vector<WigCoefDD> coef;
    wigner_coefs_dd(lmax, a, b, coef);
    DevBuf d_coef;
    HX_TRY(upload_vec(d_coef, coef));
    HX_TRY(launch_wigner_table(lmax, a, b, n, d_x, d_xlo, d_coef.as<WigCoefDD>(), d_out, sl, sk));
    HX_HIP(hipStreamSynchronize(rt().stream));  // d_coef dies with this scope
    return HX_OK;
}

// ---- what is kept between calls: nodes, and tables by normalised pair (hx_wigner.h) ------------------------------------------------
int GLNodes::ensure(int n_new, bool want_xlo)
{
    if (n == n_new && x.p && (xlo.p || !want_xlo)) return HX_OK;
    n = 0;  // (a build that fails half-way leaves no size behind that the buffers no longer hold)
    HX_TRY(x.alloc(sizeof(double) * n_new));
    HX_TRY(w.alloc(sizeof(double) * n_new));
    if (want_xlo) HX_TRY(xlo.alloc(sizeof(double) * n_new));
    else xlo.release();  // (xlo.p != null means: the low parts of the n nodes held)
    HX_TRY(launch_gauss_legendre(n_new, x.as<double>(), w.as<double>(), want_xlo ? xlo.as<double>() : nullptr));
    n = n_new;
    return HX_OK;
}
void GLNodes::release()
{
    x.release();
    w.release();
    xlo.release();
    n = 0;
}

int WigTableSet::get(const GLNodes &gl, int A, int B, WigTable **out)
{
    const bool pin = A == pin_a && B == pin_b;
    WigTable *t = pin ? &pinned : nullptr;
    for (size_t i = 0; !t && i < tabs.size(); ++i)
        if (tabs[i]->a == A && tabs[i]->b == B) t = tabs[i].get();
    if (!t) {
        if ((int)tabs.size() >= max_tabs) {
            size_t old = 0;
            for (size_t i = 1; i < tabs.size(); ++i)
                if (tabs[i]->used < tabs[old]->used) old = i;
            HX_HIP(hipStreamSynchronize(rt().stream));  // (a launch may still be reading it)
            tabs.erase(tabs.begin() + old);
        }
        tabs.emplace_back(new WigTable);
        t = tabs.back().get();
        t->a = A;
        t->b = B;
    }
    t->used = ++tick;
    *out = t;
    if (t->have) return HX_OK;
    const size_t bytes = sizeof(double) * (size_t)(pin ? pin_rows : rows) * kpad;
    HX_TRY(t->T.alloc(bytes));
    HX_HIP(hipMemsetAsync(t->T.p, 0, bytes, rt().stream));
    HX_TRY(wigner_table_build(pin ? pin_lmax : lmax, A, B, gl.n, gl.x.as<double>(), gl.xlo.as<double>(), t->T.as<double>(), (long long)kpad, 1LL));
    t->have = true;
    return HX_OK;
}

}  // namespace hx

using namespace hx;

// nodes, weights and (where xlo is not null) low parts of the n-point rule into host or device arrays
static int gauss_legendre_out(int n, double *x, double *w, double *xlo)
{
    GLNodes c;
    HX_TRY(c.ensure(n, true));
    double *dst[3] = {x, w, xlo};
    const DevBuf *src[3] = {&c.x, &c.w, &c.xlo};
    OutView v[3];
    const int nout = xlo ? 3 : 2;
    for (int i = 0; i < nout; ++i) {
        HX_TRY(v[i].bind(dst[i], sizeof(double) * n));
        HX_HIP(hipMemcpyAsync(v[i].dev, src[i]->p, sizeof(double) * n, hipMemcpyDeviceToDevice, rt().stream));
    }
    for (int i = 0; i < nout; ++i) HX_TRY(v[i].finish());
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}

extern "C" int hx_gauss_legendre(int n, double *x, double *w)
{
    HX_TRY(ensure_ready());
    if (n < 1 || !x || !w) return fail(HX_ERR_ARG, "hx_gauss_legendre: bad argument");
    return gauss_legendre_out(n, x, w, nullptr);
}

// The same with the part of every node that a double cannot hold: node k = x[k] + xlo[k] (|xlo| <~ 1e-16; see k_gauss_legendre).
extern "C" int hx_gauss_legendre_dd(int n, double *x, double *w, double *xlo)
{
    HX_TRY(ensure_ready());
    if (n < 1 || !x || !w || !xlo) return fail(HX_ERR_ARG, "hx_gauss_legendre_dd: bad argument");
    return gauss_legendre_out(n, x, w, xlo);
}

extern "C" int hx_wigner_d_table(int lmax, int a, int b, int n, const double *x, double *out)
{
    HX_TRY(ensure_ready());
    if (lmax < 0 || n < 1 || !x || !out) return fail(HX_ERR_ARG, "hx_wigner_d_table: bad argument");
    if (std::max(abs(a), abs(b)) > HX_MAX_MIX_SPIN)
        return fail(HX_ERR_UNSUPPORTED, "hx_wigner_d_table: (a,b)=(%d,%d) beyond the supported max(|a|,|b|) <= %d", a, b, HX_MAX_MIX_SPIN);
    InView vx;
    OutView vo;
    HX_TRY(vx.bind(x, sizeof(double) * n));
    HX_TRY(vo.bind(out, sizeof(double) * (size_t)n * (lmax + 1)));
    // the double-double kernel of the mixing-matrix tables at the caller's nodes (no low part: xlo = 0)
    DevBuf d_zero;
    HX_TRY(d_zero.alloc(sizeof(double) * n));
    HX_HIP(hipMemsetAsync(d_zero.p, 0, sizeof(double) * n, rt().stream));
    HX_TRY(wigner_table_build(lmax, a, b, n, vx.as<double>(), d_zero.as<double>(), vo.as<double>(), 1LL, (long long)(lmax + 1)));
    HX_TRY(vo.finish());
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}
