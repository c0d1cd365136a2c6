// hx_mapper.hip -- the one-call pixel operations: ang2pix (RING), the ordered scatter-add of HealpixMapper.map_values
// (heracles/healpy.py:58-66, :144-160), ud_grade and NESTED <-> RING reordering.  The catalogue contexts live in hx_catmap.hip,
// hx_catmap_sel.hip and hx_catalm.hip (shared core: hx_catalog.h); the pixel formulas in hx_ang2pix.h and hx_healpix.h.
//
// Reference semantics: ipix = hp.ang2pix(nside, lon, lat, lonlat=True), then the compiled
// loop `for j, i in enumerate(ipix): maps[..., i] += values[..., j]` -- each pixel receives
// its points in catalogue order.  Floating-point addition does not commute with that order,
// so the default path here reproduces it exactly: a stable radix sort of the point indices
// by pixel (hx_sort.h), then one thread per occupied pixel adds its run of points front to
// back.  HX_MAP_ATOMIC trades that guarantee for a single pass of hardware f64 atomics.
#include "hx_common.h"

#include "hx_ang2pix.h"
#include "hx_healpix.h"
#include "hx_sort.h"

namespace hx {

namespace {

__global__ __launch_bounds__(256) void k_ang2pix(long long nside, long long n, const double *__restrict__ lon,
                                                 const double *__restrict__ lat, long long *__restrict__ ipix,
                                                 unsigned *__restrict__ order, unsigned long long *__restrict__ nbad)
{
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double lo = lon[j], la = lat[j];
    const bool ok = lonlat_valid(lo, la);
    const long long npix = 12 * nside * nside;
    long long p = ok ? ang2pix_ring_one(nside, lo, la) : -1;
    if (ok && (p < 0 || p >= npix)) p = -1;  // never scatter outside the map
    if (p < 0) atomicAdd(nbad, 1ULL);
    ipix[j] = p;
    if (order) order[j] = (unsigned)j;
}

// one thread per sorted position; the first position of each run of equal pixels owns it
template <class PIX>
__global__ __launch_bounds__(256) void k_run_add(long long n, const PIX *__restrict__ pix_sorted,
                                                 const unsigned *__restrict__ idx_sorted, int nval,
                                                 const double *__restrict__ values, long long vstride,
                                                 double *__restrict__ maps, long long npix)
{
    long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const PIX p = pix_sorted[s];
    if (s > 0 && pix_sorted[s - 1] == p) return;
    long long e = s + 1;
    while (e < n && pix_sorted[e] == p) ++e;
    for (int v = 0; v < nval; ++v) {
        double acc = maps[(long long)v * npix + p];
        const double *val = values + (long long)v * vstride;
        for (long long t = s; t < e; ++t) acc += val[idx_sorted[t]];
        maps[(long long)v * npix + p] = acc;
    }
}

__global__ __launch_bounds__(256) void k_scatter_atomic(long long n, const long long *__restrict__ ipix, int nval,
                                                        const double *__restrict__ values, long long vstride,
                                                        double *__restrict__ maps, long long npix)
{
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    long long p = ipix[j];
    for (int v = 0; v < nval; ++v)
        unsafeAtomicAdd(&maps[(long long)v * npix + p], values[(long long)v * vstride + j]);
}

// numpy's pairwise summation (the arithmetic behind healpy's np.sum(axis=1) in _ud_grade_core):
// n < 8 sequential from 0; n <= 128 eight strided accumulators; else split at n/2 rounded to 8.
// numpy hands a reduction to this routine in pieces of its ufunc buffer (8192 elements) and adds the
// pieces' sums in order: numpy_sum below.  For ud_grade the two differ from 65536 children on (nside ratio 256).
template <class Load>
__device__ double numpy_pairwise_sum(long long i0, long long n, Load load)
{
    if (n < 8) {
        double res = 0.0;
        for (long long i = 0; i < n; ++i) res += load(i0 + i);
        return res;
    }
    if (n <= 128) {
        double r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = load(i0 + k);
        long long i = 8;
        for (; i < n - (n % 8); i += 8)
#pragma unroll
            for (int k = 0; k < 8; ++k) r[k] += load(i0 + i + k);
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += load(i0 + i);
        return res;
    }
    long long n2 = n / 2;
    n2 -= n2 % 8;
    return numpy_pairwise_sum(i0, n2, load) + numpy_pairwise_sum(i0 + n2, n - n2, load);
}

constexpr long long kNumpyBufsize = 8192;

template <class Load>
__device__ double numpy_sum(long long n, Load load)
{
#pragma clang fp contract(off)
    double res = numpy_pairwise_sum(0, n < kNumpyBufsize ? n : kNumpyBufsize, load);
    for (long long i0 = kNumpyBufsize; i0 < n; i0 += kNumpyBufsize)
        res += numpy_pairwise_sum(i0, (n - i0 < kNumpyBufsize) ? n - i0 : kNumpyBufsize, load);
    return res;
}

constexpr double kUnseen = -1.6375e30;

// healpy.ud_grade, RING -> RING, pess=False, power=None.  One thread per output pixel.
__global__ __launch_bounds__(256) void k_ud_grade(int order_in, int order_out, const double *__restrict__ in,
                                                  double *__restrict__ out)
{
    const long long npix_out = 12ll << (2 * order_out), npix_in = 12ll << (2 * order_in);
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix_out) return;
    const double *src = in + (long long)blockIdx.y * npix_in;
    double *dst = out + (long long)blockIdx.y * npix_out;
    const long long q = hxpix::ring2nest(order_out, p);
    if (order_out >= order_in) {
        dst[p] = src[hxpix::nest2ring(order_in, q >> (2 * (order_out - order_in)))];
        return;
    }
    const long long rat2 = 1ll << (2 * (order_in - order_out));
    long long nhit = 0;
    // mask_bad(rtol=1e-5, atol=1e-15) | ~isfinite; a masked value enters the sum as value * 0
    auto load = [&](long long c) {
        const double v = src[hxpix::nest2ring(order_in, q * rat2 + c)];
        const bool good = !(fabs(v - kUnseen) <= 1e-15 + 1e-5 * fabs(kUnseen)) && isfinite(v);
        nhit += good;
        return good ? v : v * 0.0;
    };
    const double s = numpy_sum(rat2, load);
    dst[p] = nhit ? s / (double)nhit : kUnseen;
}

bool nside_ok(int nside) { return nside >= 1 && nside <= (1 << 24); }
bool nside_pow2(int nside) { return nside >= 1 && nside <= 8192 && (nside & (nside - 1)) == 0; }

// Pixel indices of n points; fails with HX_ERR_ARG (the reference: ValueError from healpy) if any point is
// outside 0 <= theta <= pi or not finite.  Synchronises the stream (the count is read back).
int launch_ang2pix(int nside, long long n, const double *lon, const double *lat, long long *ipix, unsigned *order,
                   const char *who)
{
    if (n == 0) return HX_OK;
    static DevBuf d_bad;  // 8 bytes, lives with the process
    HX_TRY(d_bad.alloc(sizeof(unsigned long long)));
    hipStream_t st = rt().stream;
    HX_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(unsigned long long), st));
    unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_ang2pix, dim3(blocks), dim3(256), 0, st, (long long)nside, n, lon, lat, ipix, order,
                       d_bad.as<unsigned long long>());
    HX_HIP(hipGetLastError());
    unsigned long long nbad = 0;
    HX_HIP(hipMemcpyAsync(&nbad, d_bad.p, sizeof(nbad), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (nbad)
        return fail(HX_ERR_ARG, "%s: %llu of %lld points have a latitude outside [-90, 90] or a non-finite coordinate "
                    "(healpy: THETA is out of range [0,pi])", who, nbad, n);
    return HX_OK;
}

}  // namespace

}  // namespace hx

using namespace hx;

extern "C" int hx_ang2pix_ring(int nside, int64_t n, const double *lon, const double *lat, int64_t *ipix)
{
    HX_TRY(ensure_ready());
    if (!nside_ok(nside) || n < 0 || (n > 0 && (!lon || !lat || !ipix)))
        return fail(HX_ERR_ARG, "hx_ang2pix_ring: bad arguments (nside=%d n=%lld)", nside, (long long)n);
    if (n == 0) return HX_OK;
    InView vlon, vlat;
    OutView vout;
    HX_TRY(vlon.bind(lon, sizeof(double) * n));
    HX_TRY(vlat.bind(lat, sizeof(double) * n));
    HX_TRY(vout.bind(ipix, sizeof(int64_t) * n));
    {
        ProfScope ps("ang2pix");
        HX_TRY(launch_ang2pix(nside, n, vlon.as<double>(), vlat.as<double>(), (long long *)vout.as<int64_t>(), nullptr, "hx_ang2pix_ring"));
    }
    HX_TRY(vout.finish());
    return finish_call();
}

extern "C" int hx_map_values(int nside, int64_t n, const double *lon, const double *lat, int nval,
                             const double *values, double *maps, int flags)
{
    HX_TRY(ensure_ready());
    if (!nside_ok(nside) || n < 0 || nval < 0 || (n > 0 && nval > 0 && (!lon || !lat || !values || !maps)))
        return fail(HX_ERR_ARG, "hx_map_values: bad arguments (nside=%d n=%lld nval=%d)", nside, (long long)n, nval);
    if (n > 0xfffffff0ll)
        return fail(HX_ERR_UNSUPPORTED, "hx_map_values: at most 2^32-16 points per call (got %lld); page the catalogue",
                    (long long)n);
    if (n == 0 || nval == 0) return HX_OK;
    const long long npix = 12ll * nside * nside;
    hipStream_t st = rt().stream;
    InView vlon, vlat, vval;
    HX_TRY(vlon.bind(lon, sizeof(double) * n));
    HX_TRY(vlat.bind(lat, sizeof(double) * n));
    HX_TRY(vval.bind(values, sizeof(double) * n * nval));
    // maps are read-modify-write: a host array makes the round trip through a device copy
    DevBuf mtmp;
    double *dmaps = maps;
    const bool host_maps = !is_device_ptr(maps);
    if (host_maps) {
        HX_TRY(mtmp.alloc(sizeof(double) * npix * nval));
        HX_TRY(copy_h2d(mtmp.p, maps, sizeof(double) * npix * nval));
        dmaps = mtmp.as<double>();
    }
    DevBuf bpix, bord, bpix2, bord2, btmp;
    rsort::SortedPairs sp;  // the sorted (pixel, point index) pairs: whichever buffers the last pass wrote (keys narrowed to 32 bits when they fit)
    HX_TRY(bpix.alloc(sizeof(long long) * n));
    const bool ordered = !(flags & HX_MAP_ATOMIC);
    unsigned blocks = (unsigned)((n + 255) / 256);
    if (ordered) HX_TRY(bord.alloc(sizeof(unsigned) * n));
    {
        ProfScope ps("ang2pix");
        HX_TRY(launch_ang2pix(nside, n, vlon.as<double>(), vlat.as<double>(), bpix.as<long long>(),
                              ordered ? bord.as<unsigned>() : nullptr, "hx_map_values"));
    }
    if (ordered) {
        ProfScope ps("map_sort");
        // HX_SORT_WIDE=1 (tests): the 64-bit path that nside > 16384 takes, at any size
        static const bool force_wide = getenv("HX_SORT_WIDE") && getenv("HX_SORT_WIDE")[0] == '1';
        // the largest key is the last pixel (nside <= 16384: 32-bit keys, bpix2 then holds the two 32-bit key buffers of the later passes)
        HX_TRY(rsort::sort_pairs_by_key(bpix.as<long long>(), bord.as<unsigned>(), (unsigned long long)n, (unsigned long long)(npix - 1), force_wide,
                                        bpix2, bord2, btmp, st, &sp));
    }
    {
        ProfScope ps("map_add");
        if (ordered && sp.k64)
            hipLaunchKernelGGL(k_run_add<long long>, dim3(blocks), dim3(256), 0, st, (long long)n, sp.k64, sp.idx, nval, vval.as<double>(), (long long)n, dmaps, npix);
        else if (ordered)
            hipLaunchKernelGGL(k_run_add<unsigned>, dim3(blocks), dim3(256), 0, st, (long long)n, sp.k32, sp.idx, nval, vval.as<double>(), (long long)n, dmaps, npix);
        else
            hipLaunchKernelGGL(k_scatter_atomic, dim3(blocks), dim3(256), 0, st, (long long)n, bpix.as<long long>(), nval,
                               vval.as<double>(), (long long)n, dmaps, npix);
        HX_HIP(hipGetLastError());
    }
    if (host_maps) {
        return copy_d2h(maps, dmaps, sizeof(double) * npix * nval);
    }
    // temporaries die with this scope: the stream must have drained them
    HX_HIP(hipStreamSynchronize(st));
    return HX_OK;
}

extern "C" int hx_ud_grade(int nside_in, int nside_out, int nmaps, const double *in, double *out)
{
    HX_TRY(ensure_ready());
    if (!nside_pow2(nside_in) || !nside_pow2(nside_out))
        return fail(HX_ERR_ARG, "hx_ud_grade: %d -> %d: nside must be a power of 2 (<= 8192)", nside_in, nside_out);
    if (nmaps < 0 || (nmaps > 0 && (!in || !out))) return fail(HX_ERR_ARG, "hx_ud_grade: bad arguments");
    if (nmaps == 0) return HX_OK;
    const long long npix_in = 12ll * nside_in * nside_in, npix_out = 12ll * nside_out * nside_out;
    InView vin;
    OutView vout;
    HX_TRY(vin.bind(in, sizeof(double) * npix_in * nmaps));
    HX_TRY(vout.bind(out, sizeof(double) * npix_out * nmaps));
    int oi = 0, oo = 0;
    while ((1 << oi) < nside_in) ++oi;
    while ((1 << oo) < nside_out) ++oo;
    {
        ProfScope ps("ud_grade");
        hipLaunchKernelGGL(k_ud_grade, dim3((unsigned)((npix_out + 255) / 256), nmaps), dim3(256), 0, rt().stream, oi, oo,
                           vin.as<double>(), vout.as<double>());
        HX_HIP(hipGetLastError());
    }
    HX_TRY(vout.finish());
    return finish_call();
}

// NESTED <-> RING reordering of full-sky maps (healpy.read_map converts a NESTED file to RING: heracles/io.py:365 reads visibility maps
// through it).  One thread per output pixel: out[p] = in[other index of p].
__global__ __launch_bounds__(256) void k_reorder(int order, int to_ring, const double *__restrict__ in, double *__restrict__ out)
{
    const long long npix = 12ll << (2 * order);
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const long long q = to_ring ? hxpix::ring2nest(order, p) : hxpix::nest2ring(order, p);
    out[(long long)blockIdx.y * npix + p] = in[(long long)blockIdx.y * npix + q];
}

extern "C" int hx_reorder(int nside, int to_ring, int nmaps, const double *in, double *out)
{
    HX_TRY(ensure_ready());
    if (!nside_pow2(nside)) return fail(HX_ERR_ARG, "hx_reorder: nside %d must be a power of 2 (<= 8192)", nside);
    if (nmaps < 0 || (nmaps > 0 && (!in || !out)) || in == out) return fail(HX_ERR_ARG, "hx_reorder: bad arguments (in place is not supported)");
    if (nmaps == 0) return HX_OK;
    const long long npix = 12ll * nside * nside;
    InView vin;
    OutView vout;
    HX_TRY(vin.bind(in, sizeof(double) * npix * nmaps));
    HX_TRY(vout.bind(out, sizeof(double) * npix * nmaps));
    int o = 0;
    while ((1 << o) < nside) ++o;
    hipLaunchKernelGGL(k_reorder, dim3((unsigned)((npix + 255) / 256), nmaps), dim3(256), 0, rt().stream, o, to_ring ? 1 : 0, vin.as<double>(), vout.as<double>());
    HX_HIP(hipGetLastError());
    HX_TRY(vout.finish());
    return finish_call();
}

// (healpy's pixel weights -- hx_pixel_weights_size / _expand / _solve -- live in hx_weights.hip)
