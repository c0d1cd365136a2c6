// hx_weights.hip -- healpy's pixel quadrature weights (heracles/healpy.py:183-189, use_pixel_weights=True): the expansion of the
// compressed values of `healpix_full_weights_nside_NNNN.fits` to the full sky (hx_pixel_weights_expand), and the values themselves,
// computed from first principles (hx_pixel_weights_solve).
//
// Layout.  The file holds (nside + 1)(3 nside + 1) / 4 values: for every ring of the northern hemisphere (equator included) the
// weights of the pixels of half a quadrant -- the quadrature weights have the 8-fold symmetry of the pixelisation (4 quadrants x mirror
// inside a quadrant) plus north/south.  The expansion is the published algorithm of healpix_cxx's apply_fullweights (third-party, not in
// /root/reference; restated):  ring i < 2 nside has q = min(nside, i + 1) pixels per quadrant; it is "shifted" (pixel centres off the
// quadrant boundary) for i < nside - 1 or i + nside odd; it stores w = (q + 1) / 2 values, + 1 if q is even and the ring is not shifted;
// pixel j of the ring uses value min(j4, q - shifted - j4), j4 = j mod q; the map value is multiplied by 1 + value.
//
// Solve.  Unknown: x, the compressed values.  E x is its expansion to
// the full sky (without the `1 +`), A = map2alm with unit weights at the band limit L = 2 lmax of the products Y_lm Y_l'm' of a
// transform at lmax.  The weights 1 + E x integrate every Y_LM, L <= 2 lmax, exactly:
//     A (1 + E x) = sqrt(4 pi) e_00.
// A map with the symmetries of the pixelisation (4 quadrants x mirror inside a quadrant x north/south) has real alms, and only those
// with L even and M = 0 (mod 4); P projects onto them, so that the rounding noise of the other modes never enters the iteration.
//     S = P A E,   r = sqrt(4 pi) e_00 - P A 1,   S x = r
// is solved by conjugate gradients on the normal equations (CGLS) from x = 0, which gives the solution of minimum norm.  With the
// inner product on alms that counts the orders m > 0 twice, A^T = (4 pi / npix) alm2map, hence S^T a = (4 pi / npix) E^T alm2map(P a),
// E^T being the sum over the pixels that share a compressed value (the fold).
//
// One iteration, all in HBM:
//     q = S p            k_expand_pixel_weights, analysis sweep of the orders 0, 4, 8, .. (m_step = 4), k_wt_project (+ <q, q> per order)
//     alpha = gamma / <q, q>                                                     k_wt_alpha (ordered sum of the per-order sums)
//     x += alpha p,  res -= alpha q                                              k_wt_axpy2
//     g = S^T res        synthesis sweep (all orders: it takes no stride), k_wt_fold (+ <g, g> per ring)
//     gamma' = <g, g>,  beta = gamma' / gamma                                    k_wt_beta (ordered sum of the per-ring sums)
//     p = g + beta p                                                             k_wt_xpby
// and the host reads one scalar, gamma', for the stopping test sqrt(gamma' / gamma_0) <= epsilon.  Every sum is formed in a fixed
// order (threads: strided partial sums, then a tree through LDS; blocks: one value each, added by one work-group in the same way):
// two solves give the same bits.
#include <algorithm>
#include <cmath>
#include <vector>

#include "hx_sht_common.h"

namespace hx {

namespace {

enum { WT_GAMMA = 0, WT_GAMMA0, WT_ALPHA, WT_BETA, WT_QQ, WT_MAXRES, WT_NSCALAR };

// sum over the 256 threads of a work-group, the same association every time; every thread must call
__device__ inline double wt_block_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__device__ inline double wt_block_max(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// geometry of northern ring i (0 = next to the pole, 2 nside - 1 = the equator): pixels per quadrant, shifted or not, values stored,
// first pixel of the ring and of its southern twin
struct WtRing {
    int q, shifted, nval;
    long long pix, psouth;
};
__device__ inline WtRing wt_ring(int nside, int i)
{
    WtRing r;
    const long long ns = nside, npix = 12 * ns * ns;
    r.q = i + 1 < nside ? i + 1 : nside;
    r.shifted = ((i < nside - 1) || ((i + nside) & 1)) ? 1 : 0;
    r.nval = ((r.q + 1) >> 1) + (((r.q & 1) || r.shifted) ? 0 : 1);
    r.pix = i < nside ? 2ll * i * (i + 1) : 2 * ns * (ns - 1) + (long long)(i - nside + 1) * 4 * ns;
    r.psouth = npix - r.pix - 4ll * r.q;
    return r;
}

// out = base + E x: base = 1 gives the multiplicative weights, base = 0 the expansion without the `1 +`.  One work-group per northern ring.
__global__ __launch_bounds__(256) void k_expand_pixel_weights(int nside, const long long *__restrict__ voff, const double *__restrict__ x, double base,
                                                              double *__restrict__ out)
{
    const int i = blockIdx.x;
    const WtRing r = wt_ring(nside, i);
    const double *w = x + voff[i];
    for (int j = threadIdx.x; j < 4 * r.q; j += blockDim.x) {
        const int j4 = j % r.q, mir = r.q - r.shifted - j4;
        const double v = base + w[j4 < mir ? j4 : mir];
        out[r.pix + j] = v;
        if (i != 2 * nside - 1) out[r.psouth + j] = v;
    }
}

// g = scale E^T map: the sum over the orbit of every compressed value -- per quadrant the pixel j4 = v and its mirror image
// q - shifted - v (where that is another pixel of the quadrant), north then south (the equator ring has no southern twin) -- in that
// order.  gg[i] = sum over the ring's values of g^2.  One work-group per northern ring.
__global__ __launch_bounds__(256) void k_wt_fold(int nside, const long long *__restrict__ voff, const double *__restrict__ map, double scale,
                                                 double *__restrict__ g, double *__restrict__ gg)
{
    __shared__ double sh[256];
    const int i = blockIdx.x;
    const WtRing r = wt_ring(nside, i);
    const bool south = i != 2 * nside - 1;
    double acc = 0.0;
    for (int v = threadIdx.x; v < r.nval; v += blockDim.x) {
        const int ja = v, jb = r.q - r.shifted - v;
        const bool two = jb != ja && jb < r.q;
        double s = 0.0;
        for (int k = 0; k < 4; ++k) {
            s += map[r.pix + k * r.q + ja];
            if (two) s += map[r.pix + k * r.q + jb];
        }
        if (south)
            for (int k = 0; k < 4; ++k) {
                s += map[r.psouth + k * r.q + ja];
                if (two) s += map[r.psouth + k * r.q + jb];
            }
        s *= scale;
        g[voff[i] + v] = s;
        acc += s * s;
    }
    const double t = wt_block_sum(acc, sh);
    if (threadIdx.x == 0) gg[i] = t;
}

// alm <- P alm: the real part of the modes with l even and m = 0 (mod 4), zero elsewhere (the orders the strided analysis sweep did
// not write included).  qq[m] = the order's share of <alm, alm>, orders m > 0 counted twice.  One work-group per order.
__global__ __launch_bounds__(256) void k_wt_project(int lmax, double2 *__restrict__ alm, double *__restrict__ qq)
{
    __shared__ double sh[256];
    const int m = blockIdx.x;
    const bool keep = (m & 3) == 0;
    double2 *a = alm + almidx(lmax, 0, m);
    double acc = 0.0;
    for (int l = m + threadIdx.x; l <= lmax; l += blockDim.x) {
        const double v = (keep && !(l & 1)) ? a[l].x : 0.0;
        a[l] = make_double2(v, 0.0);
        acc += v * v;
    }
    const double t = wt_block_sum(acc, sh);
    if (threadIdx.x == 0) qq[m] = m ? 2.0 * t : t;
}

// res = sqrt(4 pi) e_00 - a
__global__ __launch_bounds__(256) void k_wt_residual(long long nlm, const double2 *__restrict__ a, double2 *__restrict__ res)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nlm) return;
    const double2 v = a[i];
    res[i] = make_double2((i == 0 ? 3.5449077018110320546 : 0.0) - v.x, -v.y);
}

// per order the largest |res| over its modes; one work-group per order
__global__ __launch_bounds__(256) void k_wt_absmax(int lmax, const double2 *__restrict__ res, double *__restrict__ mx)
{
    __shared__ double sh[256];
    const int m = blockIdx.x;
    const double2 *a = res + almidx(lmax, 0, m);
    double acc = 0.0;
    for (int l = m + threadIdx.x; l <= lmax; l += blockDim.x) acc = fmax(acc, fmax(fabs(a[l].x), fabs(a[l].y)));
    const double t = wt_block_max(acc, sh);
    if (threadIdx.x == 0) mx[m] = t;
}

// the n per-block values added by one work-group: thread t adds part[t], part[t + 256], .. in that order, then the tree
__device__ inline double wt_ordered_sum(const double *__restrict__ part, int n, double *sh)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += part[i];
    return wt_block_sum(acc, sh);
}

__global__ __launch_bounds__(256) void k_wt_alpha(const double *__restrict__ part, int n, double *__restrict__ sc)
{
    __shared__ double sh[256];
    const double qq = wt_ordered_sum(part, n, sh);
    if (threadIdx.x == 0) {
        sc[WT_QQ] = qq;
        sc[WT_ALPHA] = qq > 0.0 ? sc[WT_GAMMA] / qq : 0.0;
    }
}

// first: the gradient at x = 0 -- gamma_0, and beta = 0 so that p = g
__global__ __launch_bounds__(256) void k_wt_beta(const double *__restrict__ part, int n, int first, double *__restrict__ sc)
{
    __shared__ double sh[256];
    const double gn = wt_ordered_sum(part, n, sh);
    if (threadIdx.x == 0) {
        if (first) sc[WT_GAMMA0] = gn;
        sc[WT_BETA] = (first || !(sc[WT_GAMMA] > 0.0)) ? 0.0 : gn / sc[WT_GAMMA];
        sc[WT_GAMMA] = gn;
    }
}

__global__ __launch_bounds__(256) void k_wt_max(const double *__restrict__ part, int n, double *__restrict__ sc)
{
    __shared__ double sh[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc = fmax(acc, part[i]);
    const double t = wt_block_max(acc, sh);
    if (threadIdx.x == 0) sc[WT_MAXRES] = t;
}

// y1 += alpha x1 (n1 values), y2 -= alpha x2 (n2 values): the two updates of a step that need alpha
__global__ __launch_bounds__(256) void k_wt_axpy2(const double *__restrict__ sc, long long n1, double *__restrict__ y1, const double *__restrict__ x1,
                                                  long long n2, double *__restrict__ y2, const double *__restrict__ x2)
{
    const double alpha = sc[WT_ALPHA];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n1) y1[i] += alpha * x1[i];
    else if (i - n1 < n2) y2[i - n1] -= alpha * x2[i - n1];
}

// p = g + beta p
__global__ __launch_bounds__(256) void k_wt_xpby(const double *__restrict__ sc, long long n, const double *__restrict__ g, double *__restrict__ p)
{
    const double beta = sc[WT_BETA];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = g[i] + beta * p[i];
}

__global__ __launch_bounds__(256) void k_wt_fill(long long n, double v, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v;
}

inline unsigned wt_blocks(long long n) { return (unsigned)((n + 255) / 256); }

// the analysis sweeps of the plan cover the orders 0, 4, 8, .. while one of these lives
struct StrideGuard {
    hx_plan *pl;
    explicit StrideGuard(hx_plan *p) : pl(p) { pl->m_lo = 0; pl->m_hi = -1; pl->m_step = 4; }
    ~StrideGuard() { pl->m_lo = 0; pl->m_hi = -1; pl->m_step = 1; }
};

// first compressed value of every northern ring, on the device; HX_ERR_ARG if they do not add up to hx_pixel_weights_size
int ring_value_offsets(int nside, DevBuf &d_off, const char *who)
{
    std::vector<long long> voff(2 * nside);
    long long v = 0;
    for (int i = 0; i < 2 * nside; ++i) {
        voff[i] = v;
        const int q = std::min(nside, i + 1);
        const bool shifted = (i < nside - 1) || ((i + nside) & 1);
        v += ((q + 1) >> 1) + (((q & 1) || shifted) ? 0 : 1);
    }
    if (v != hx_pixel_weights_size(nside)) return fail(HX_ERR_ARG, "%s: internal size mismatch", who);
    return upload(d_off, voff);
}

}  // namespace

}  // namespace hx

using namespace hx;

extern "C" int64_t hx_pixel_weights_size(int nside) { return nside < 1 ? 0 : ((int64_t)(nside + 1) * (3 * (int64_t)nside + 1)) / 4; }

extern "C" int hx_pixel_weights_expand(int nside, int64_t ncompressed, const double *compressed, double *weights)
{
    HX_TRY(ensure_ready());
    if (nside < 1 || nside > 8192 || !compressed || !weights) return fail(HX_ERR_ARG, "hx_pixel_weights_expand: bad arguments");
    if (ncompressed != hx_pixel_weights_size(nside))
        return fail(HX_ERR_ARG, "hx_pixel_weights_expand: %lld compressed weights, NSIDE=%d needs %lld", (long long)ncompressed, nside,
                    (long long)hx_pixel_weights_size(nside));
    DevBuf d_off;
    HX_TRY(ring_value_offsets(nside, d_off, "hx_pixel_weights_expand"));
    InView vin;
    OutView vout;
    HX_TRY(vin.bind(compressed, sizeof(double) * ncompressed));
    HX_TRY(vout.bind(weights, sizeof(double) * 12ll * nside * nside));
    hipLaunchKernelGGL(k_expand_pixel_weights, dim3(2 * nside), dim3(256), 0, rt().stream, nside, d_off.as<long long>(), vin.as<double>(), 1.0,
                       vout.as<double>());
    HX_HIP(hipGetLastError());
    HX_TRY(vout.finish());
    HX_HIP(hipStreamSynchronize(rt().stream));  // d_off dies with this scope
    return HX_OK;
}

extern "C" int hx_pixel_weights_solve(hx_plan *pl, int lmax, double epsilon, int itmax, double *compressed_out, int *iterations,
                                      double *rel_gradient, double *max_residual)
{
    HX_TRY(ensure_ready());
    if (!pl || pl->nside < 1 || pl->nside > 8192 || !compressed_out) return fail(HX_ERR_ARG, "hx_pixel_weights_solve: bad arguments");
    if (lmax < 0 || lmax > 3 * pl->nside / 2)
        return fail(HX_ERR_ARG, "hx_pixel_weights_solve: lmax %d: the weights of NSIDE=%d are exact up to lmax = %d only and make the quadrature worse beyond",
                    lmax, pl->nside, 3 * pl->nside / 2);
    if (pl->lmax != 2 * lmax) return fail(HX_ERR_ARG, "hx_pixel_weights_solve: the plan must have the band limit 2 lmax = %d, it has %d", 2 * lmax, pl->lmax);
    if (!(epsilon >= 0.0) || itmax < 0) return fail(HX_ERR_ARG, "hx_pixel_weights_solve: epsilon %g, itmax %d", epsilon, itmax);
    if (pl->nssrc || pl->hsrc) return fail(HX_ERR_ARG, "hx_pixel_weights_solve: the plan is in use by another route");
    const int nside = pl->nside, L = pl->lmax, nring = 2 * nside;
    const long long npix = pl->npix, nlm = pl->nlm, nx = hx_pixel_weights_size(nside);
    DevBuf d_off, d_map, d_res, d_q, d_vec, d_part, d_sc;
    HX_TRY(ring_value_offsets(nside, d_off, "hx_pixel_weights_solve"));
    HX_TRY(d_map.alloc(sizeof(double) * (size_t)npix));
    HX_TRY(d_res.alloc(sizeof(double2) * (size_t)nlm));
    HX_TRY(d_q.alloc(sizeof(double2) * (size_t)nlm));
    HX_TRY(d_vec.alloc(sizeof(double) * (size_t)nx * 3));  // x, p, g
    const int npart = std::max(nring, L + 1);
    HX_TRY(d_part.alloc(sizeof(double) * (size_t)npart));
    HX_TRY(d_sc.alloc(sizeof(double) * WT_NSCALAR));
    OutView vout;
    HX_TRY(vout.bind(compressed_out, sizeof(double) * (size_t)nx));
    hipStream_t st = rt().stream;
    const long long *off = d_off.as<long long>();
    double *map = d_map.as<double>(), *x = d_vec.as<double>(), *p = x + nx, *g = p + nx, *part = d_part.as<double>(), *sc = d_sc.as<double>();
    double2 *res = d_res.as<double2>(), *q = d_q.as<double2>();
    const double wnorm = 4.0 * M_PI / (double)npix;
    HX_HIP(hipMemsetAsync(d_vec.p, 0, sizeof(double) * (size_t)nx * 3, st));
    HX_HIP(hipMemsetAsync(d_q.p, 0, sizeof(double2) * (size_t)nlm, st));
    HX_HIP(hipMemsetAsync(d_sc.p, 0, sizeof(double) * WT_NSCALAR, st));
    StrideGuard stride(pl);

    // q <- P A map
    auto analyse = [&]() -> int {
        HX_TRY(analysis_batch(pl, 0, 1, map, q, nullptr, nullptr, nullptr, 0));
        ProfScope ps("pixel_weights");
        hipLaunchKernelGGL(k_wt_project, dim3(L + 1), dim3(256), 0, st, L, q, part);
        HX_HIP(hipGetLastError());
        return HX_OK;
    };
    // g <- S^T res, gamma <- <g, g>, beta
    auto gradient = [&](int first) -> int {
        HX_TRY(synthesis_batch(pl, 0, 1, res, map, nullptr));
        ProfScope ps("pixel_weights");
        hipLaunchKernelGGL(k_wt_fold, dim3(nring), dim3(256), 0, st, nside, off, map, wnorm, g, part);
        hipLaunchKernelGGL(k_wt_beta, dim3(1), dim3(256), 0, st, part, nring, first, sc);
        hipLaunchKernelGGL(k_wt_xpby, dim3(wt_blocks(nx)), dim3(256), 0, st, sc, nx, g, p);
        HX_HIP(hipGetLastError());
        return HX_OK;
    };
    // the one scalar per iteration the host looks at
    auto read_gamma = [&](double *gamma) -> int {
        HX_HIP(hipMemcpyAsync(gamma, sc + WT_GAMMA, sizeof(double), hipMemcpyDeviceToHost, st));
        HX_HIP(hipStreamSynchronize(st));
        return HX_OK;
    };

    // r = sqrt(4 pi) e_00 - P A 1
    {
        ProfScope ps("pixel_weights");
        hipLaunchKernelGGL(k_wt_fill, dim3(wt_blocks(npix)), dim3(256), 0, st, npix, 1.0, map);
        HX_HIP(hipGetLastError());
    }
    HX_TRY(analyse());
    {
        ProfScope ps("pixel_weights");
        hipLaunchKernelGGL(k_wt_residual, dim3(wt_blocks(nlm)), dim3(256), 0, st, nlm, q, res);
        HX_HIP(hipGetLastError());
    }
    HX_TRY(gradient(1));
    double gamma0 = 0.0, gamma = 0.0;
    HX_TRY(read_gamma(&gamma0));
    gamma = gamma0;
    int it = 0;
    while (it < itmax && gamma0 > 0.0 && !(std::sqrt(gamma / gamma0) <= epsilon)) {
        {
            ProfScope ps("pixel_weights");
            hipLaunchKernelGGL(k_expand_pixel_weights,dim3(nring), dim3(256), 0, st, nside, off, p, 0.0, map);
            HX_HIP(hipGetLastError());
        }
        HX_TRY(analyse());
        {
            ProfScope ps("pixel_weights");
            hipLaunchKernelGGL(k_wt_alpha, dim3(1), dim3(256), 0, st, part, L + 1, sc);
            hipLaunchKernelGGL(k_wt_axpy2, dim3(wt_blocks(nx + 2 * nlm)), dim3(256), 0, st, sc, nx, x, p, 2 * nlm, reinterpret_cast<double *>(res),
                               reinterpret_cast<const double *>(q));
            HX_HIP(hipGetLastError());
        }
        HX_TRY(gradient(0));
        HX_TRY(read_gamma(&gamma));
        ++it;
        if (!std::isfinite(gamma)) return fail(HX_ERR_HIP, "hx_pixel_weights_solve: the iteration broke down at step %d", it);
    }
    // the constraint residual of the weights as they are handed out, formed anew: sqrt(4 pi) e_00 - P A (1 + E x)
    double maxres = 0.0;
    {
        ProfScope ps("pixel_weights");
        hipLaunchKernelGGL(k_expand_pixel_weights,dim3(nring), dim3(256), 0, st, nside, off, x, 1.0, map);
        HX_HIP(hipGetLastError());
    }
    HX_TRY(analyse());
    {
        ProfScope ps("pixel_weights");
        hipLaunchKernelGGL(k_wt_residual, dim3(wt_blocks(nlm)), dim3(256), 0, st, nlm, q, res);
        hipLaunchKernelGGL(k_wt_absmax, dim3(L + 1), dim3(256), 0, st, L, res, part);
        hipLaunchKernelGGL(k_wt_max, dim3(1), dim3(256), 0, st, part, L + 1, sc);
        HX_HIP(hipGetLastError());
    }
    HX_HIP(hipMemcpyAsync(&maxres, sc + WT_MAXRES, sizeof(double), hipMemcpyDeviceToHost, st));
    HX_HIP(hipMemcpyAsync(vout.as<double>(), x, sizeof(double) * (size_t)nx, hipMemcpyDeviceToDevice, st));
    HX_TRY(vout.finish());
    HX_HIP(hipStreamSynchronize(st));  // the work buffers die with this scope
    if (iterations) *iterations = it;
    if (rel_gradient) *rel_gradient = gamma0 > 0.0 ? std::sqrt(gamma / gamma0) : 0.0;
    if (max_residual) *max_residual = maxres;
    return HX_OK;
}
