// hx_mapper.hip -- catalogue -> HEALPix map accumulation on the GPU: ang2pix (RING) and the
// ordered scatter-add of HealpixMapper.map_values (heracles/healpy.py:58-66, :144-160).
//
// Reference semantics: ipix = hp.ang2pix(nside, lon, lat, lonlat=True), then the compiled
// loop `for j, i in enumerate(ipix): maps[..., i] += values[..., j]` -- each pixel receives
// its points in catalogue order.  Floating-point addition does not commute with that order,
// so the default path here reproduces it exactly: a stable radix sort of the point indices
// by pixel (rocPRIM), then one thread per occupied pixel adds its run of points front to
// back.  HX_MAP_ATOMIC trades that guarantee for a single pass of hardware f64 atomics.
//
// ang2pix follows the published HEALPix algorithm (Gorski et al. 2005; healpix_cxx
// T_Healpix_Base::loc2pix, RING branch), the third-party code healpy calls; it is absent
// from /root/reference, so index parity is pinned on the test-side numpy restatement
// and on the pix2ang round trip of every pixel centre (tests/test_gpu_mapper.py), and at
// pixel edges on the exact pixel and admissible set of tests/pixel_reference.py
// (tests/test_gpu_pixel_edges.py).
#include "hx_common.h"

#include "hx_healpix.h"
#include "hx_sort.h"

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
    long long *spix64 = nullptr;
    unsigned *spix = nullptr;    // the sorted (pixel, point index) pairs: whichever buffers the last pass wrote (keys narrowed to 32 bits)
    unsigned *sord = nullptr;
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
        HX_TRY(bpix2.alloc(sizeof(long long) * n));
        HX_TRY(bord2.alloc(sizeof(unsigned) * n));
        unsigned end_bit = 1;
        while ((1ll << end_bit) < npix) ++end_bit;
        ProfScope ps("map_sort");
        // HX_SORT_WIDE=1 (tests): the 64-bit path that nside > 16384 takes, at any size
        static const bool force_wide = getenv("HX_SORT_WIDE") && getenv("HX_SORT_WIDE")[0] == '1';
        if (end_bit <= 32 && !force_wide) {
            // pixel indices fit 32 bits (nside <= 16384): the first pass narrows the keys, bpix2 holds the two 32-bit key buffers of the later passes
            HX_TRY(rsort::radix_sort_pairs_narrow(bpix.as<long long>(), bord.as<unsigned>(), bpix2.as<unsigned>(), bpix2.as<unsigned>() + n, bord2.as<unsigned>(),
                                                  (unsigned long long)n, (int)end_bit, btmp, st, &spix, &sord));
        } else {
            HX_TRY(rsort::radix_sort_pairs<long long>(bpix.as<long long>(), bord.as<unsigned>(), bpix2.as<long long>(), bord2.as<unsigned>(),
                                                      (unsigned long long)n, (int)end_bit, btmp, st, &spix64, &sord));
        }
    }
    {
        ProfScope ps("map_add");
        if (ordered && spix64)
            hipLaunchKernelGGL(k_run_add<long long>, dim3(blocks), dim3(256), 0, st, (long long)n, spix64, sord, nval, vval.as<double>(), (long long)n, dmaps, npix);
        else if (ordered)
            hipLaunchKernelGGL(k_run_add<unsigned>, dim3(blocks), dim3(256), 0, st, (long long)n, spix, sord, nval, vval.as<double>(), (long long)n, dmaps, npix);
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

// =====================================================================================
// catalogues -> field maps (heracles.map_catalogs, heracles/fields.py:197-559): one pass over each page for every field of a catalogue
// =====================================================================================
// Two contexts share one core.  hx_catmap maps one catalogue; hx_catmap_sel maps the views of one base catalogue
// (heracles/catalog/base.py:204-310) in one pass over the base's pages.  The rules of the reference's fields are stated once, in
// field_step (keep rule, value rows w v with every product rounded on its own, as numpy's `v * w`; 0 on a dropped row, which adds
// nothing to a sum that starts at +0; the moment contributions {1, w, w^2, |w v|^2}; which columns count their NaNs) and group_step
// (the pixel of a row in an (nside, lon, lat) group; the sentinel npix for rows no field of the group keeps and for invalid positions,
// which are counted).  Moments are summed per block into a slab and over blocks in a fixed order (k_cat_reduce); no float atomics.
//
// k_cat_prepare reads the page's columns once, writes value rows, pixel keys and row indices, and sums the moments in registers.  Each
// group is then stably sorted once (hx_sort.h) and k_cat_run_add adds every map row of its fields in catalogue order, one pass per row,
// stopping at the sentinel.
//
// Nothing in a page's mapping depends on the selection but the sort key: the value rows and the pixel of a row are the same for every
// view.  k_sel_prepare therefore reads the page once: it forms each row's membership word (bit s: the base's filters keep the row, its
// mask word has bit s, and every predicate term of selection s holds), writes the value rows and the pixels of every group, and sums
// the moments of every (selection, field): a ballot loop over the selections present in the wave, the wave sums kept per wave in LDS
// (one writer each), the four waves and then the blocks added in a fixed order.  k_sel_keys turns (membership, pixel) into the key
// s (npix + 1) + pixel, npix being the sentinel of the selection's unkept rows and nsel (npix + 1) that of rows in no selection; a row
// in k > 1 selections gets k keys at offsets from an exclusive scan of the per-row key counts (only when some row of the page has
// k > 1: disjoint selections sort n keys).  One stable sort per group orders them, and k_sel_run_add adds each run into the map of its
// key's selection, in catalogue order.
namespace hx {
namespace {

constexpr int kCatF = HX_CAT_MAX_FIELDS, kCatG = HX_CAT_MAX_GROUPS, kCatC = HX_CAT_MAX_COLUMNS;
constexpr int kSelS = HX_CAT_MAX_SELECTIONS, kSelP = HX_CAT_MAX_PREDICATES, kSelFl = HX_CAT_MAX_FILTERS;
constexpr int kCatBlocks = 2048;  // most blocks of a prepare kernel: rows per thread grow beyond 2048 x 256 rows

// what both prepare kernels read about the page, the fields and their (nside, lon, lat) groups (the scalars before the pointers: with the
// pointers first the compiler reserves a scratch slot for the prepare kernels that it never uses)
struct CatCore {
    long long cap;
    int nfield, ngroup;
    int kind[kCatF], grp[kCatF], cv[kCatF], ci[kCatF], cw[kCatF];
    int gnside[kCatG], glon[kCatG], glat[kCatG];
    const double *col[kCatC];
    double *val[kCatF];  // row r of field f at val[f] + r * cap
};

struct CatArgs {
    CatCore c;
    long long *key[kCatG];
    unsigned *ord[kCatG];
    unsigned long long *nan;   // [nfield][5]
    unsigned long long *nbad;  // [ngroup]
    double *slab;              // [gridDim.x][nfield * 4]
};

struct SelArgs {
    CatCore c;
    const unsigned *mask;  // per row, or null (every bit set)
    unsigned *pix[kCatG];  // per group: the row's pixel, npix for a row no field of the group keeps or an invalid position
    int nsel, npred, nfilt;
    int pmeta[kSelP];  // selection | column << 8 | op << 16
    double pval[kSelP];
    int ftype[kSelFl], fa[kSelFl], fb[kSelFl], fnside[kSelFl];
    const double *fp[kSelFl];
    unsigned *mem;                // [n] membership words
    unsigned *cnt;                // [n] keys per row: max(1, popcount)
    unsigned long long *nan;      // [nsel][nfield][5]
    unsigned long long *nbad;     // [nsel][ngroup]
    unsigned long long *fcount;   // [nsel][nfilt + 1]
    unsigned long long *extra;    // sum over rows of popcount - 1
    double *slab;                 // [gridDim.x][nsel nfield 4]
};

__device__ inline double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// One field on one row: whether the field keeps the row, what the row adds to the moments {n, w, w^2, |w v|^2} (all 0 on a dropped row)
// and which of the columns read on a kept row hold a NaN (bit 0 lon, 1 lat, 2 value, 3 imaginary part, 4 weight).
struct FieldStep {
    bool keep;
    double n, w, w2, v2;
    unsigned nan;
};

// stores the value rows of field f on row j
__device__ __forceinline__ FieldStep field_step(const CatCore &a, int f, long long j)
{
#pragma clang fp contract(off)
    const int kind = a.kind[f];
    const double w = a.cw[f] >= 0 ? a.col[a.cw[f]][j] : 1.0;
    FieldStep s{kind == HX_CAT_POSITIONS || w != 0.0, 0.0, 0.0, 0.0, 0.0, 0u};
    double r0 = 0.0, r1 = 0.0;
    if (s.keep) {
        const int g = a.grp[f];
        s.nan = (isnan(a.col[a.glon[g]][j]) ? 1u : 0u) | (isnan(a.col[a.glat[g]][j]) ? 2u : 0u) | (isnan(w) ? 16u : 0u);
        if (kind == HX_CAT_SCALAR || kind == HX_CAT_COMPLEX) {
            const double v = a.col[a.cv[f]][j];
            if (isnan(v)) s.nan |= 4u;
            r0 = v * w;
            if (kind == HX_CAT_COMPLEX) {
                const double im = a.col[a.ci[f]][j];
                if (isnan(im)) s.nan |= 8u;
                r1 = im * w;
            }
            s.v2 = r0 * r0 + r1 * r1;  // |w v|^2: (w re)^2 + (w im)^2, r1 = 0 for a scalar
        } else {
            r0 = w;
        }
        s.n = 1.0;
        s.w = w;
        s.w2 = w * w;
    }
    a.val[f][j] = r0;
    if (kind == HX_CAT_COMPLEX) a.val[f][a.cap + j] = r1;
    return s;
}

// One (nside, lon, lat) group on one row: the pixel, or the sentinel npix when the row is not wanted or its position is invalid (bad)
struct GroupStep {
    long long pix;
    bool bad;
};

__device__ __forceinline__ GroupStep group_step(const CatCore &a, int g, long long j, bool wanted)
{
    const long long nside = a.gnside[g], npix = 12 * nside * nside;
    GroupStep s{npix, false};
    if (wanted) {
        const double lo = a.col[a.glon[g]][j], la = a.col[a.glat[g]][j];
        const long long q = lonlat_valid(lo, la) ? ang2pix_ring_one(nside, lo, la) : -1;
        if (q < 0 || q >= npix) s.bad = true;
        else s.pix = q;
    }
    return s;
}

// Every field on row j, for the prepare kernels of hx_catmap and hx_catalm: field_step, the NaN counters (nan [nfield][5]), the
// thread's moment sums m and which groups have a field that keeps the row.
template <int NF>
__device__ __forceinline__ void fields_step(const CatCore &a, long long j, double (&m)[NF][4], bool (&kept)[kCatG], unsigned long long *nan)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int g = 0; g < kCatG; ++g) kept[g] = false;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const FieldStep s = field_step(a, f, j);
        if (s.keep) {
#pragma unroll
            for (int g = 0; g < kCatG; ++g)
                if (g == a.grp[f]) kept[g] = true;
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if ((s.nan >> k) & 1u) atomicAdd(nan + 5 * f + k, 1ULL);
            // (a dropped row's contributions are +0.0 and adding them would leave the sums as they are, bit for bit: the sums start at
            // +0.0 and never become -0.0.  Adding under the branch keeps the kernel at 8 VGPRs per field instead of 16.)
            m[f][0] += s.n;
            m[f][1] += s.w;
            m[f][2] += s.w2;
            m[f][3] += s.v2;
        }
    }
}

// per-block partial moments: fixed-shape wave and block reductions into slab[blockIdx.x][NF * 4]
template <int NF>
__device__ __forceinline__ void block_moments(const double (&m)[NF][4], double *slab)
{
#pragma clang fp contract(off)
    __shared__ double part[4][kCatF * 4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double s = wave_sum(m[f][k]);
            if (lane == 0) part[wv][f * 4 + k] = s;
        }
    __syncthreads();
    if (threadIdx.x < NF * 4) {
        const int t = threadIdx.x;
        slab[(long long)blockIdx.x * NF * 4 + t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    }
}

// NF = the number of fields, a template argument so that only their moments occupy registers
template <int NF>
__global__ __launch_bounds__(256) void k_cat_prepare(long long n, CatArgs a)
{
#pragma clang fp contract(off)
    double m[NF][4];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int k = 0; k < 4; ++k) m[f][k] = 0.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        bool kept[kCatG];
        fields_step<NF>(a.c, j, m, kept, a.nan);
#pragma unroll
        for (int g = 0; g < kCatG; ++g) {
            if (g >= a.c.ngroup) break;
            const GroupStep s = group_step(a.c, g, j, kept[g]);
            if (s.bad) atomicAdd(a.nbad + g, 1ULL);
            a.key[g][j] = s.pix;
            a.ord[g][j] = (unsigned)j;
        }
    }
    block_moments<NF>(m, a.slab);
}

// acc[t] += sum over blocks of slab[b][t], b in order: the moments of the page added to the context's
__global__ __launch_bounds__(256) void k_cat_reduce(int nblocks, int width, const double *__restrict__ slab, double *__restrict__ acc)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= width) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += slab[(long long)b * width + t];
    acc[t] += s;
}

// ---- hx_catalm: the same page, prepared for the point transform (no pixels, no sort key) -----------------------------------------
struct AlmArgs {
    CatCore c;             // gnside[g]: the band limit of group g
    double2 *loc[kCatG];   // per group: (theta, phi) of every row
    unsigned long long *nan;   // [nfield][5]
    unsigned long long *nbad;  // [ngroup]
    double *slab;              // [gridDim.x][nfield * 4]
};

// One (lmax, lon, lat) group on one row: the point (theta, phi) = (radians(90 - lat), radians(lon % 360)) of
// heracles/ducc.py:117-119, every operation rounded on its own (lat = -90 gives exactly M_PI, the largest colatitude the spread
// takes).  Validity is group_step's rule without its 1e-5 of slack beyond the south pole, which the (theta, phi) grid has no cell
// for: a latitude outside [-90, 90] or a non-finite coordinate is bad on a wanted row.  A row that adds nothing -- no field of the
// group keeps it, or its position is invalid -- gets a ZERO VALUE (field_step writes 0 on a dropped row; k_catalm_prepare clears the
// value rows of a bad one) at a harmless location: its own position when that is valid, else the equator.  The spread kernels skip a
// zero value before any atomic, and a finite zero at a valid location is never counted as a bad point.
struct PointStep {
    double2 loc;
    bool bad;
};

__device__ __forceinline__ PointStep point_step(const CatCore &a, int g, long long j, bool wanted)
{
#pragma clang fp contract(off)
    const double lo = a.col[a.glon[g]][j], la = a.col[a.glat[g]][j];
    const bool ok = isfinite(lo) && la >= -90.0 && la <= 90.0;
    PointStep s{{kHalfPi, 0.0}, wanted && !ok};
    if (ok) {
        double r = fmod(lo, 360.0);  // numpy's %: the sign of the divisor
        if (r < 0.0) r += 360.0;
        s.loc.x = (90.0 - la) * kDeg2Rad;
        s.loc.y = r * kDeg2Rad;
    }
    return s;
}

// k_cat_prepare for the point transform: field_step and the moment reduction as they are there (8 VGPRs of sums per field, NF a
// template argument for the same reason); per group one double2 store instead of the key and the row index.
template <int NF>
__global__ __launch_bounds__(256) void k_catalm_prepare(long long n, AlmArgs a)
{
#pragma clang fp contract(off)
    double m[NF][4];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int k = 0; k < 4; ++k) m[f][k] = 0.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        bool kept[kCatG];
        fields_step<NF>(a.c, j, m, kept, a.nan);
#pragma unroll
        for (int g = 0; g < kCatG; ++g) {
            if (g >= a.c.ngroup) break;
            const PointStep s = point_step(a.c, g, j, kept[g]);
            a.loc[g][j] = s.loc;
            if (s.bad) {  // (rare, and an error for the caller: the row must still add nothing)
                atomicAdd(a.nbad + g, 1ULL);
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    if (a.c.grp[f] == g) {
                        a.c.val[f][j] = 0.0;
                        if (a.c.kind[f] == HX_CAT_COMPLEX) a.c.val[f][a.c.cap + j] = 0.0;
                    }
            }
        }
    }
    block_moments<NF>(m, a.slab);
}

// k_run_add for one value row and one map row, ending at the sentinel key npix: a pixel's run is added in catalogue order, starting
// from the map's value
__global__ __launch_bounds__(256) void k_cat_run_add(long long n, const unsigned *__restrict__ pix_sorted, const unsigned *__restrict__ idx_sorted,
                                                     const double *__restrict__ vrow, double *__restrict__ mrow, unsigned npix)
{
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const unsigned p = pix_sorted[s];
    if (p >= npix) return;
    if (s > 0 && pix_sorted[s - 1] == p) return;
    long long e = s + 1;
    while (e < n && pix_sorted[e] == p) ++e;
    double acc = mrow[p];
    for (long long t = s; t < e; ++t) acc += vrow[idx_sorted[t]];
    mrow[p] = acc;
}

__global__ __launch_bounds__(256) void k_cat_finish(long long npix, int nrow, double *__restrict__ map, double norm,
                                                    const double *__restrict__ vis)
{
#pragma clang fp contract(off)
    const long long total = npix * nrow, stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        double v = map[i] / norm;
        if (vis) v = v - vis[i % npix];
        map[i] = v;
    }
}

__device__ inline bool sel_compare(double x, int op, double c)
{
    switch (op) {
    case HX_CAT_EQ: return x == c;
    case HX_CAT_NE: return x != c;
    case HX_CAT_LT: return x < c;
    case HX_CAT_LE: return x <= c;
    case HX_CAT_GT: return x > c;
    default: return x >= c;
    }
}

// add 1 to cnt[s * stride + k] for every bit s of m (rare events: NaNs, invalid positions, filtered rows)
__device__ inline void count_bits(unsigned m, unsigned long long *cnt, int stride, int k)
{
    while (m) {
        const int s = __ffs(m) - 1;
        m &= m - 1;
        atomicAdd(cnt + (long long)s * stride + k, 1ULL);
    }
}

template <int NF>
__global__ __launch_bounds__(256) void k_sel_prepare(long long n, SelArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ double wpart[];  // [4 waves][nsel NF 4]
    const int W = a.nsel * NF * 4, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int t = threadIdx.x; t < 4 * W; t += blockDim.x) wpart[t] = 0.0;
    __syncthreads();
    double *mine = wpart + wv * W;
    const unsigned all = a.nsel == 32 ? ~0u : (1u << a.nsel) - 1u;
    const long long stride = (long long)gridDim.x * blockDim.x;
    // the loop bound is uniform over the block: the ballots below need every lane of the wave
    for (long long base = (long long)blockIdx.x * blockDim.x; base < n; base += stride) {
        const long long j = base + threadIdx.x;
        unsigned m = 0;
        double c[NF][4];
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int k = 0; k < 4; ++k) c[f][k] = 0.0;
        if (j < n) {
            m = (a.mask ? a.mask[j] : ~0u) & all;
            for (int p = 0; p < a.npred; ++p) {
                const int meta = a.pmeta[p];
                if (!sel_compare(a.c.col[(meta >> 8) & 255][j], meta >> 16, a.pval[p])) m &= ~(1u << (meta & 255));
            }
            // the base's filters, in order, on the rows some selection holds (a view selects before it filters)
            for (int k = 0; m && k < a.nfilt; ++k) {
                bool drop = false;
                if (a.ftype[k] == HX_CAT_FILTER_INVALID) {
                    for (int cc = 0; cc < kCatC; ++cc)
                        if ((a.fa[k] >> cc) & 1) drop = drop || isnan(a.c.col[cc][j]);
                    if (drop && a.fb[k] >= 0) drop = a.c.col[a.fb[k]][j] != 0.0;
                } else {
                    const double lo = a.c.col[a.fa[k]][j], la = a.c.col[a.fb[k]][j];
                    const long long ns = a.fnside[k], np = 12 * ns * ns;
                    const long long q = lonlat_valid(lo, la) ? ang2pix_ring_one(ns, lo, la) : -1;
                    if (q < 0 || q >= np) {
                        count_bits(m, a.fcount, a.nfilt + 1, a.nfilt);
                        drop = true;
                    } else {
                        drop = a.fp[k][q] == 0.0;
                    }
                }
                if (drop) {
                    count_bits(m, a.fcount, a.nfilt + 1, k);
                    m = 0;
                }
            }
            bool kept[kCatG];
#pragma unroll
            for (int g = 0; g < kCatG; ++g) kept[g] = false;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const FieldStep s = field_step(a.c, f, j);
                if (s.keep) {
#pragma unroll
                    for (int g = 0; g < kCatG; ++g)
                        if (g == a.c.grp[f]) kept[g] = true;
#pragma unroll
                    for (int k = 0; k < 5; ++k)
                        if ((s.nan >> k) & 1u) count_bits(m, a.nan + 5 * f, 5 * a.c.nfield, k);
                    c[f][0] = s.n;
                    c[f][1] = s.w;
                    c[f][2] = s.w2;
                    c[f][3] = s.v2;
                }
            }
#pragma unroll
            for (int g = 0; g < kCatG; ++g) {
                if (g >= a.c.ngroup) break;
                const GroupStep s = group_step(a.c, g, j, m && kept[g]);
                if (s.bad) count_bits(m, a.nbad, a.c.ngroup, g);
                a.pix[g][j] = (unsigned)s.pix;
            }
            const int pc = __popc(m);
            a.mem[j] = m;
            a.cnt[j] = pc > 1 ? (unsigned)pc : 1u;
        }
        // rows in more than one selection: one atomic per wave
        unsigned ex = __popc(m) > 1 ? (unsigned)__popc(m) - 1u : 0u;
        unsigned orm = m;
        for (int off = 32; off > 0; off >>= 1) {
            ex += __shfl_xor(ex, off, 64);
            orm |= __shfl_xor(orm, off, 64);
        }
        if (lane == 0 && ex) atomicAdd(a.extra, (unsigned long long)ex);
        // moments: for every selection present in the wave, the wave sums of its rows' contributions (fixed shape, one writer)
        while (orm) {
            const int s = __ffs(orm) - 1;
            orm &= orm - 1;
            const bool in = (m >> s) & 1u;
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double t = wave_sum(in ? c[f][k] : 0.0);
                    if (lane == 0) mine[(s * NF + f) * 4 + k] += t;
                }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < W; t += blockDim.x)
        a.slab[(long long)blockIdx.x * W + t] = ((wpart[t] + wpart[W + t]) + wpart[2 * W + t]) + wpart[3 * W + t];
}

// the keys of row j at off[j] (or j when no row has more than one): s (npix + 1) + pixel for every bit s, in ascending s
__global__ __launch_bounds__(256) void k_sel_keys(long long n, const unsigned *__restrict__ mem, const unsigned *__restrict__ off,
                                                  const unsigned *__restrict__ pix, long long npix1, int nsel, long long *__restrict__ key,
                                                  unsigned *__restrict__ ord)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    unsigned m = mem[j];
    long long o = off ? (long long)off[j] : j;
    if (!m) {
        key[o] = (long long)nsel * npix1;
        ord[o] = (unsigned)j;
        return;
    }
    const long long p = pix[j];
    while (m) {
        const int s = __ffs(m) - 1;
        m &= m - 1;
        key[o] = (long long)s * npix1 + p;
        ord[o] = (unsigned)j;
        ++o;
    }
}

// k_cat_run_add for one value row and the map rows of every selection: the run's key names its selection and pixel
template <class K>
__global__ __launch_bounds__(256) void k_sel_run_add(long long n, const K *__restrict__ keys, const unsigned *__restrict__ idx_sorted,
                                                     long long npix1, int nsel, const double *__restrict__ vrow,
                                                     double *const *__restrict__ mrows)
{
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const K k = keys[s];
    if (s > 0 && keys[s - 1] == k) return;
    const long long sel = (long long)k / npix1, p = (long long)k - sel * npix1;
    if (sel >= nsel || p == npix1 - 1) return;
    long long e = s + 1;
    while (e < n && keys[e] == k) ++e;
    double *map = mrows[sel];
    double acc = map[p];
    for (long long t = s; t < e; ++t) acc += vrow[idx_sorted[t]];
    map[p] = acc;
}

// What both contexts hold: the fields, their value rows and maps ([nsel][nfield]; one selection for hx_catmap), the sort's buffers, the
// moments and counters, and the two staging sets of the page protocol.
struct CatBase {
    long long cap = 0;
    int ncols = 0, nfield = 0, ngroup = 0, nsel = 1;
    int kind[kCatF] = {}, grp[kCatF] = {}, nside[kCatF] = {}, nrow[kCatF] = {};
    double *map[kSelS * kCatF] = {};
    DevBuf val[kCatF], ka, kb, v1, sort_tmp;
    DevBuf stage[2][kCatC + 1];  // the columns, then the mask words
    DevBuf slab, acc, counters;
    hipEvent_t ev_up[2] = {}, ev_done[2] = {};
    long long page_no = 0;
    // a context's destructor calls this first: its own buffers are released before ~CatBase runs, and no kernel may still use them
    void wait() { (void)hipStreamSynchronize(rt().stream); }
    ~CatBase()
    {
        for (int s = 0; s < 2; ++s) {
            if (ev_up[s]) (void)hipEventDestroy(ev_up[s]);
            if (ev_done[s]) (void)hipEventDestroy(ev_done[s]);
        }
    }
};

inline bool col_ok(int i, int ncols, bool need) { return i >= (need ? 0 : -1) && i < ncols; }

// Validates the field descriptors, forms the (resolution, lon, lat) groups and allocates the value rows; `who`: the entry point, for
// messages.  The resolution (desc[1], kept in nside[] / gnside[]) is an nside in [1, 16384] for the map contexts, which pass their device
// maps; hx_catalm passes maps = NULL (it owns its outputs) and res_lo / res_hi = the range of its lmax.
int cat_fields_init(CatBase *c, CatCore &a, const char *who, int64_t page_size, int ncols, int nfields, const int *desc, int nsel,
                    double *const *maps, int res_lo = 1, int res_hi = 16384)
{
    c->cap = a.cap = page_size;
    c->ncols = ncols;
    c->nfield = a.nfield = nfields;
    c->nsel = nsel;
    for (int f = 0; f < nfields; ++f) {
        const int *d = desc + 7 * f;
        const int kind = d[0], ns = d[1];
        const bool need_v = kind == HX_CAT_SCALAR || kind == HX_CAT_COMPLEX;
        bool maps_ok = true;
        for (int s = 0; maps && s < nsel; ++s) {
            c->map[s * nfields + f] = maps[s * nfields + f];
            maps_ok = maps_ok && maps[s * nfields + f] && is_device_ptr(maps[s * nfields + f]);
        }
        if (kind < HX_CAT_POSITIONS || kind > HX_CAT_WEIGHTS || ns < res_lo || ns > res_hi || !col_ok(d[2], ncols, true) ||
            !col_ok(d[3], ncols, true) || !col_ok(d[4], ncols, need_v) || !col_ok(d[5], ncols, kind == HX_CAT_COMPLEX) ||
            !col_ok(d[6], ncols, false) || !maps_ok)
            return fail(HX_ERR_ARG, "%s: bad descriptor of field %d (kind %d, resolution %d; maps must be device memory)", who, f, kind, ns);
        int g = 0;
        for (; g < c->ngroup; ++g)
            if (a.gnside[g] == ns && a.glon[g] == d[2] && a.glat[g] == d[3]) break;
        if (g == c->ngroup) {
            if (g == kCatG) return fail(HX_ERR_UNSUPPORTED, "%s: more than %d (resolution, lon, lat) groups", who, kCatG);
            a.gnside[g] = ns;
            a.glon[g] = d[2];
            a.glat[g] = d[3];
            ++c->ngroup;
        }
        c->kind[f] = a.kind[f] = kind;
        c->grp[f] = a.grp[f] = g;
        c->nside[f] = ns;
        c->nrow[f] = kind == HX_CAT_COMPLEX ? 2 : 1;
        a.cv[f] = d[4];
        a.ci[f] = d[5];
        a.cw[f] = d[6];
        HX_TRY(c->val[f].alloc(sizeof(double) * page_size * c->nrow[f]));
        a.val[f] = c->val[f].as<double>();
    }
    a.ngroup = c->ngroup;
    return HX_OK;
}

// The zeroed moments (`width` sums, and their slab) and `ncount` counters, and the events of the page protocol
int cat_sums_init(CatBase *c, int width, size_t ncount)
{
    HX_TRY(c->slab.alloc(sizeof(double) * kCatBlocks * width));
    HX_TRY(c->acc.alloc(sizeof(double) * width));
    HX_TRY(c->counters.alloc(sizeof(unsigned long long) * ncount));
    hipStream_t st = rt().stream;
    HX_HIP(hipMemsetAsync(c->acc.p, 0, c->acc.bytes, st));
    HX_HIP(hipMemsetAsync(c->counters.p, 0, c->counters.bytes, st));
    for (int s = 0; s < 2; ++s) {
        HX_HIP(hipEventCreateWithFlags(&c->ev_up[s], hipEventDisableTiming));
        HX_HIP(hipEventCreateWithFlags(&c->ev_done[s], hipEventDisableTiming));
        HX_HIP(hipEventRecord(c->ev_done[s], st));
    }
    return HX_OK;
}

// The page protocol.  Pages alternate between two staging sets, so that the upload of page k + 1 (copy stream) overlaps the kernels of
// page k (compute stream).  page_open checks the arguments (n == 0: nothing to do, nothing opened), waits until the previous user of the
// staging set (page k - 2) has finished reading it, uploads what is host memory, and makes the compute stream wait for the upload; it
// gives the device addresses of the columns and of the optional mask words.  page_close, after the page's last kernel, releases the
// staging set and waits for what reads the caller's memory.
struct PageIO {
    int set = 0;
    bool any_dev = false, any_pinned = false;
    const double *col[kCatC] = {};  // the columns on the device
    const unsigned *mask = nullptr;
};

int page_open(CatBase *c, const char *who, int64_t n, const double *const *cols, const uint32_t *mask, PageIO *io)
{
    if (!c || n < 0 || n > c->cap || (n > 0 && !cols))
        return fail(HX_ERR_ARG, "%s: bad arguments (n=%lld, page size %lld)", who, (long long)n, c ? c->cap : 0ll);
    if (n == 0) return HX_OK;
    for (int i = 0; i < c->ncols; ++i)
        if (!cols[i]) return fail(HX_ERR_ARG, "%s: column %d is NULL", who, i);
    hipStream_t st = rt().stream, cs = copy_stream();
    if (!cs) cs = st;
    const int s = io->set = (int)(c->page_no++ & 1);
    bool uploaded = false;
    HX_HIP(hipStreamWaitEvent(cs, c->ev_done[s], 0));
    for (int i = 0; i <= c->ncols; ++i) {
        const void *src = i < c->ncols ? (const void *)cols[i] : (const void *)mask;
        const size_t elem = i < c->ncols ? sizeof(double) : sizeof(unsigned);
        if (!src) continue;  // (no mask)
        const void *dev = src;
        if (is_device_ptr(src)) {
            io->any_dev = true;
        } else {
            HX_TRY(c->stage[s][i].alloc(elem * c->cap));
            io->any_pinned = io->any_pinned || is_pinned_host(src);
            HX_TRY(copy_h2d(c->stage[s][i].p, src, elem * n, cs));
            dev = c->stage[s][i].p;
            uploaded = true;
        }
        if (i < c->ncols) io->col[i] = static_cast<const double *>(dev);
        else io->mask = static_cast<const unsigned *>(dev);
    }
    if (uploaded && cs != st) {
        HX_HIP(hipEventRecord(c->ev_up[s], cs));
        HX_HIP(hipStreamWaitEvent(st, c->ev_up[s], 0));
    }
    return HX_OK;
}

int page_close(CatBase *c, const PageIO &io)
{
    hipStream_t st = rt().stream, cs = copy_stream();
    HX_HIP(hipEventRecord(c->ev_done[io.set], st));
    // the caller may free its columns on return: device columns are read by the kernels, pinned ones by a DMA that nothing waited for
    if (io.any_dev) HX_HIP(hipStreamSynchronize(st));
    else if (io.any_pinned) HX_HIP(hipStreamSynchronize(cs ? cs : st));
    return HX_OK;
}

// Waits for the pages; the moments and counters of a context with one selection (counters: nan [nfield][5] at 0, nbad [ngroup] at 5 kCatF)
int cat_moments(CatBase *c, const char *who, double *out, int64_t *bad)
{
    HX_TRY(ensure_ready());
    if (!c || !out || !bad) return fail(HX_ERR_ARG, "%s: bad arguments", who);
    hipStream_t st = rt().stream;
    double acc[kCatF * 4];
    unsigned long long cnt[5 * kCatF + kCatG];
    HX_HIP(hipMemcpyAsync(acc, c->acc.p, sizeof(double) * 4 * c->nfield, hipMemcpyDeviceToHost, st));
    HX_HIP(hipMemcpyAsync(cnt, c->counters.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    for (int f = 0; f < c->nfield; ++f) {
        for (int k = 0; k < 4; ++k) out[4 * f + k] = acc[4 * f + k];
        for (int k = 0; k < 5; ++k) bad[6 * f + k] = (int64_t)cnt[5 * f + k];
        bad[6 * f + 5] = (int64_t)cnt[5 * kCatF + c->grp[f]];
    }
    return HX_OK;
}

// map <- map / norm - vis for the map of (sel, field)
int cat_finish(CatBase *c, const char *who, int sel, int field, double norm, const double *vis)
{
    HX_TRY(ensure_ready());
    if (!c || sel < 0 || sel >= c->nsel || field < 0 || field >= c->nfield) return fail(HX_ERR_ARG, "%s: bad arguments", who);
    const long long npix = 12ll * c->nside[field] * c->nside[field];
    InView vv;
    HX_TRY(vv.bind(vis, sizeof(double) * npix));
    {
        ProfScope ps("catmap_finish");
        const long long total = npix * c->nrow[field];
        const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 65536);
        hipLaunchKernelGGL(k_cat_finish, dim3(blocks), dim3(256), 0, rt().stream, npix, c->nrow[field], c->map[sel * c->nfield + field], norm,
                           vv.as<double>());
        HX_HIP(hipGetLastError());
    }
    HX_HIP(hipStreamSynchronize(rt().stream));  // (a staged visibility dies with this scope)
    return HX_OK;
}

}  // namespace
}  // namespace hx

struct hx_catmap : CatBase {
    CatArgs args{};
    DevBuf key[kCatG], ord[kCatG];
    // counters: nan [nfield][5] at 0, nbad [ngroup] at 5 kCatF
    ~hx_catmap() { wait(); }
};

static int catmap_init(hx_catmap *c, int64_t page_size, int ncols, int nfields, const int *desc, double *const *maps)
{
    if (page_size < 1 || page_size > 0xfffffff0ll || ncols < 2 || ncols > kCatC || nfields < 1 || nfields > kCatF || !desc || !maps)
        return fail(HX_ERR_ARG, "hx_catmap_create: bad arguments (page_size=%lld ncols=%d nfields=%d; at most %d columns and %d fields)",
                    (long long)page_size, ncols, nfields, kCatC, kCatF);
    CatArgs &a = c->args;
    HX_TRY(cat_fields_init(c, a.c, "hx_catmap_create", page_size, ncols, nfields, desc, 1, maps));
    for (int g = 0; g < c->ngroup; ++g) {
        HX_TRY(c->key[g].alloc(sizeof(long long) * page_size));
        HX_TRY(c->ord[g].alloc(sizeof(unsigned) * page_size));
        a.key[g] = c->key[g].as<long long>();
        a.ord[g] = c->ord[g].as<unsigned>();
    }
    HX_TRY(c->ka.alloc(sizeof(unsigned) * page_size));
    HX_TRY(c->kb.alloc(sizeof(unsigned) * page_size));
    HX_TRY(c->v1.alloc(sizeof(unsigned) * page_size));
    HX_TRY(cat_sums_init(c, nfields * 4, 5 * kCatF + kCatG));
    a.slab = c->slab.as<double>();
    a.nan = c->counters.as<unsigned long long>();
    a.nbad = a.nan + 5 * kCatF;
    return HX_OK;
}

extern "C" hx_catmap *hx_catmap_create(int64_t page_size, int ncols, int nfields, const int *desc, double *const *maps)
{
    if (ensure_ready() != HX_OK) return nullptr;
    hx_catmap *c = new hx_catmap;
    if (catmap_init(c, page_size, ncols, nfields, desc, maps) != HX_OK) {
        delete c;
        return nullptr;
    }
    return c;
}

extern "C" void hx_catmap_destroy(hx_catmap *c) { delete c; }

extern "C" int hx_catmap_page(hx_catmap *c, int64_t n, const double *const *cols)
{
    HX_TRY(ensure_ready());
    PageIO io;
    HX_TRY(page_open(c, "hx_catmap_page", n, cols, nullptr, &io));
    if (n == 0) return HX_OK;
    CatArgs a = c->args;
    std::copy(io.col, io.col + kCatC, a.c.col);
    hipStream_t st = rt().stream;
    const unsigned nblocks = (unsigned)std::min<long long>((n + 255) / 256, kCatBlocks);
    {
        ProfScope ps("catmap_prepare");
        switch (c->nfield) {
#define HX_CAT_PREP(NF) case NF: hipLaunchKernelGGL(k_cat_prepare<NF>, dim3(nblocks), dim3(256), 0, st, (long long)n, a); break;
            HX_CAT_PREP(1) HX_CAT_PREP(2) HX_CAT_PREP(3) HX_CAT_PREP(4) HX_CAT_PREP(5) HX_CAT_PREP(6) HX_CAT_PREP(7) HX_CAT_PREP(8)
#undef HX_CAT_PREP
        }
        hipLaunchKernelGGL(k_cat_reduce, dim3(1), dim3(256), 0, st, (int)nblocks, c->nfield * 4, c->slab.as<double>(), c->acc.as<double>());
        HX_HIP(hipGetLastError());
    }
    for (int g = 0; g < c->ngroup; ++g) {
        const long long npix = 12ll * a.c.gnside[g] * a.c.gnside[g];
        unsigned end_bit = 1;
        while ((1ll << end_bit) <= npix) ++end_bit;  // the sentinel npix sorts after every pixel
        unsigned *ks = nullptr, *vs = nullptr;
        {
            ProfScope ps("catmap_sort");
            HX_TRY(rsort::radix_sort_pairs_narrow(c->key[g].as<long long>(), c->ord[g].as<unsigned>(), c->ka.as<unsigned>(), c->kb.as<unsigned>(),
                                                  c->v1.as<unsigned>(), (unsigned long long)n, (int)end_bit, c->sort_tmp, st, &ks, &vs));
        }
        {
            ProfScope ps("catmap_add");
            // one pass per map row: the live set of a pass (one value row, one map) stays small enough for the cache (all rows of the
            // group in one pass: 21 instead of 17 ms per 10^8 rows for four rows at nside 4096)
            for (int f = 0; f < c->nfield; ++f) {
                if (c->grp[f] != g) continue;
                for (int r = 0; r < c->nrow[f]; ++r)
                    hipLaunchKernelGGL(k_cat_run_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n, ks, vs,
                                       c->val[f].as<double>() + r * c->cap, c->map[f] + r * npix, (unsigned)npix);
            }
            HX_HIP(hipGetLastError());
        }
    }
    return page_close(c, io);
}

extern "C" int hx_catmap_moments(hx_catmap *c, double *out, int64_t *bad) { return cat_moments(c, "hx_catmap_moments", out, bad); }

extern "C" int hx_catmap_finish(hx_catmap *c, int field, double norm, const double *vis)
{
    return cat_finish(c, "hx_catmap_finish", 0, field, norm, vis);
}

struct hx_catmap_sel : CatBase {
    int nfilt = 0;
    SelArgs args{};
    DevBuf mrows[kCatF];  // per field: for each of its rows, the nsel map-row pointers
    DevBuf pix[kCatG], mem, cnt, scan_sums, key, key2, ord;
    // counters: nan [nsel][nfield][5], nbad [nsel][ngroup], fcount [nsel][nfilt + 1], extra
    size_t n_nan() const { return (size_t)nsel * nfield * 5; }
    size_t n_bad() const { return (size_t)nsel * ngroup; }
    size_t n_fcount() const { return (size_t)nsel * (nfilt + 1); }
    ~hx_catmap_sel() { wait(); }
};

static int catmap_sel_init(hx_catmap_sel *c, int64_t page_size, int ncols, int nfields, const int *desc, int nsel, int npred,
                           const int *preds, const double *pval, int nfilt, const int *filters, const double *const *footprints,
                           double *const *maps)
{
    if (page_size < 1 || page_size > 0xfffffff0ll || ncols < 2 || ncols > kCatC || nfields < 1 || nfields > kCatF || !desc || !maps ||
        nsel < 1 || nsel > kSelS || npred < 0 || npred > kSelP || (npred && (!preds || !pval)) || nfilt < 0 || nfilt > kSelFl ||
        (nfilt && !filters))
        return fail(HX_ERR_ARG, "hx_catmap_create_sel: bad arguments (page_size=%lld ncols=%d nfields=%d nsel=%d npred=%d nfilt=%d; at most "
                    "%d columns, %d fields, %d selections, %d predicates and %d filters)", (long long)page_size, ncols, nfields, nsel,
                    npred, nfilt, kCatC, kCatF, kSelS, kSelP, kSelFl);
    c->nfilt = nfilt;
    SelArgs &a = c->args;
    a.nsel = nsel;
    a.npred = npred;
    a.nfilt = nfilt;
    for (int p = 0; p < npred; ++p) {
        const int s = preds[3 * p], col = preds[3 * p + 1], op = preds[3 * p + 2];
        if (s < 0 || s >= nsel || !col_ok(col, ncols, true) || op < HX_CAT_EQ || op > HX_CAT_GE)
            return fail(HX_ERR_ARG, "hx_catmap_create_sel: bad predicate %d (selection %d, column %d, op %d)", p, s, col, op);
        a.pmeta[p] = s | col << 8 | op << 16;
        a.pval[p] = pval[p];
    }
    for (int k = 0; k < nfilt; ++k) {
        const int *d = filters + 4 * k;
        bool ok;
        if (d[0] == HX_CAT_FILTER_INVALID) {
            ok = d[1] != 0 && (unsigned)d[1] < (1u << ncols) && col_ok(d[2], ncols, false);
        } else {
            ok = d[0] == HX_CAT_FILTER_FOOTPRINT && col_ok(d[1], ncols, true) && col_ok(d[2], ncols, true) && nside_ok(d[3]) &&
                 d[3] <= 16384 && footprints && footprints[k] && is_device_ptr(footprints[k]);
            if (ok) a.fp[k] = footprints[k];
        }
        if (!ok)
            return fail(HX_ERR_ARG, "hx_catmap_create_sel: bad filter %d (type %d; footprints must be device memory)", k, d[0]);
        a.ftype[k] = d[0];
        a.fa[k] = d[1];
        a.fb[k] = d[2];
        a.fnside[k] = d[3];
    }
    HX_TRY(cat_fields_init(c, a.c, "hx_catmap_create_sel", page_size, ncols, nfields, desc, nsel, maps));
    for (int f = 0; f < nfields; ++f) {
        const long long npix = 12ll * c->nside[f] * c->nside[f];
        std::vector<double *> rows;
        for (int r = 0; r < c->nrow[f]; ++r)
            for (int s = 0; s < nsel; ++s) rows.push_back(maps[s * nfields + f] + r * npix);
        HX_TRY(c->mrows[f].alloc(sizeof(double *) * rows.size()));
        HX_HIP(hipMemcpy(c->mrows[f].p, rows.data(), sizeof(double *) * rows.size(), hipMemcpyHostToDevice));
    }
    for (int g = 0; g < c->ngroup; ++g) {
        HX_TRY(c->pix[g].alloc(sizeof(unsigned) * page_size));
        a.pix[g] = c->pix[g].as<unsigned>();
    }
    HX_TRY(c->mem.alloc(sizeof(unsigned) * page_size));
    HX_TRY(c->cnt.alloc(sizeof(unsigned) * page_size));
    a.mem = c->mem.as<unsigned>();
    a.cnt = c->cnt.as<unsigned>();
    HX_TRY(cat_sums_init(c, nsel * nfields * 4, c->n_nan() + c->n_bad() + c->n_fcount() + 1));
    a.slab = c->slab.as<double>();
    a.nan = c->counters.as<unsigned long long>();
    a.nbad = a.nan + c->n_nan();
    a.fcount = a.nbad + c->n_bad();
    a.extra = a.fcount + c->n_fcount();
    return HX_OK;
}

extern "C" hx_catmap_sel *hx_catmap_create_sel(int64_t page_size, int ncols, int nfields, const int *desc, int nsel, int npred,
                                               const int *preds, const double *pval, int nfilt, const int *filters,
                                               const double *const *footprints, double *const *maps)
{
    if (ensure_ready() != HX_OK) return nullptr;
    hx_catmap_sel *c = new hx_catmap_sel;
    if (catmap_sel_init(c, page_size, ncols, nfields, desc, nsel, npred, preds, pval, nfilt, filters, footprints, maps) != HX_OK) {
        delete c;
        return nullptr;
    }
    return c;
}

extern "C" void hx_catmap_destroy_sel(hx_catmap_sel *c) { delete c; }

extern "C" int hx_catmap_page_sel(hx_catmap_sel *c, int64_t n, const double *const *cols, const uint32_t *mask)
{
    HX_TRY(ensure_ready());
    PageIO io;
    HX_TRY(page_open(c, "hx_catmap_page_sel", n, cols, mask, &io));
    if (n == 0) return HX_OK;
    SelArgs a = c->args;
    std::copy(io.col, io.col + kCatC, a.c.col);
    a.mask = io.mask;
    hipStream_t st = rt().stream;
    const unsigned nblocks = (unsigned)std::min<long long>((n + 255) / 256, kCatBlocks);
    const int width = c->nsel * c->nfield * 4;
    unsigned long long extra = 0;
    {
        ProfScope ps("catmap_prepare");
        const size_t lds = sizeof(double) * 4 * width;
        HX_HIP(hipMemsetAsync(a.extra, 0, sizeof(unsigned long long), st));
        switch (c->nfield) {
#define HX_SEL_PREP(NF) case NF: hipLaunchKernelGGL(k_sel_prepare<NF>, dim3(nblocks), dim3(256), lds, st, (long long)n, a); break;
            HX_SEL_PREP(1) HX_SEL_PREP(2) HX_SEL_PREP(3) HX_SEL_PREP(4) HX_SEL_PREP(5) HX_SEL_PREP(6) HX_SEL_PREP(7) HX_SEL_PREP(8)
#undef HX_SEL_PREP
        }
        hipLaunchKernelGGL(k_cat_reduce, dim3((width + 255) / 256), dim3(256), 0, st, (int)nblocks, width, c->slab.as<double>(),
                           c->acc.as<double>());
        HX_HIP(hipGetLastError());
        // the number of keys decides the sort's size: rows in several selections enter it once per selection
        HX_HIP(hipMemcpyAsync(&extra, a.extra, sizeof(extra), hipMemcpyDeviceToHost, st));
        HX_HIP(hipStreamSynchronize(st));
    }
    const unsigned long long nkeys = (unsigned long long)n + extra;
    if (nkeys > 0xfffffff0ull)
        return fail(HX_ERR_UNSUPPORTED, "hx_catmap_page_sel: %llu (row, selection) pairs in one page (at most 2^32 - 16): use smaller pages",
                    nkeys);
    const unsigned *off = nullptr;
    if (extra) {
        // exclusive scan of the per-row key counts, in place
        ProfScope ps("catmap_sort");
        const unsigned long long e = (unsigned long long)n;
        const unsigned nsb = (unsigned)((e + rsort::SCAN_TILE - 1) / rsort::SCAN_TILE);
        HX_TRY(c->scan_sums.alloc(sizeof(unsigned) * (nsb + 16)));
        hipLaunchKernelGGL(rsort::k_scan_sums, dim3(nsb), dim3(rsort::SCAN_T), 0, st, c->cnt.as<unsigned>(), e, c->scan_sums.as<unsigned>());
        hipLaunchKernelGGL(rsort::k_scan_top, dim3(1), dim3(1024), 0, st, c->scan_sums.as<unsigned>(), nsb);
        hipLaunchKernelGGL(rsort::k_scan_apply, dim3(nsb), dim3(rsort::SCAN_T), 0, st, c->cnt.as<unsigned>(), e, c->scan_sums.as<unsigned>());
        HX_HIP(hipGetLastError());
        off = c->cnt.as<unsigned>();
    }
    HX_TRY(c->key.alloc(sizeof(long long) * nkeys));
    HX_TRY(c->ord.alloc(sizeof(unsigned) * nkeys));
    HX_TRY(c->v1.alloc(sizeof(unsigned) * nkeys));
    for (int g = 0; g < c->ngroup; ++g) {
        const long long npix = 12ll * a.c.gnside[g] * a.c.gnside[g], npix1 = npix + 1;
        const unsigned long long top = (unsigned long long)c->nsel * (unsigned long long)npix1;  // the largest key
        int end_bit = 1;
        while (end_bit < 64 && (1ull << end_bit) <= top) ++end_bit;
        const unsigned *ks32 = nullptr;
        const long long *ks64 = nullptr;
        unsigned *vs = nullptr;
        {
            ProfScope ps("catmap_sort");
            hipLaunchKernelGGL(k_sel_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n, c->mem.as<unsigned>(), off,
                               c->pix[g].as<unsigned>(), npix1, c->nsel, c->key.as<long long>(), c->ord.as<unsigned>());
            HX_HIP(hipGetLastError());
            if (end_bit <= 32) {
                HX_TRY(c->ka.alloc(sizeof(unsigned) * nkeys));
                HX_TRY(c->kb.alloc(sizeof(unsigned) * nkeys));
                unsigned *k = nullptr;
                HX_TRY(rsort::radix_sort_pairs_narrow(c->key.as<long long>(), c->ord.as<unsigned>(), c->ka.as<unsigned>(), c->kb.as<unsigned>(),
                                                      c->v1.as<unsigned>(), nkeys, end_bit, c->sort_tmp, st, &k, &vs));
                ks32 = k;
            } else {
                HX_TRY(c->key2.alloc(sizeof(long long) * nkeys));
                long long *k = nullptr;
                HX_TRY(rsort::radix_sort_pairs<long long>(c->key.as<long long>(), c->ord.as<unsigned>(), c->key2.as<long long>(),
                                                          c->v1.as<unsigned>(), nkeys, end_bit, c->sort_tmp, st, &k, &vs));
                ks64 = k;
            }
        }
        {
            ProfScope ps("catmap_add");
            const unsigned blocks = (unsigned)((nkeys + 255) / 256);
            // one launch per value row for every selection (the row's map rows are those of all selections)
            for (int f = 0; f < c->nfield; ++f) {
                if (c->grp[f] != g) continue;
                for (int r = 0; r < c->nrow[f]; ++r) {
                    const double *vrow = c->val[f].as<double>() + r * c->cap;
                    double *const *mrows = c->mrows[f].as<double *>() + r * c->nsel;
                    if (ks32)
                        hipLaunchKernelGGL(k_sel_run_add<unsigned>, dim3(blocks), dim3(256), 0, st, (long long)nkeys, ks32, vs, npix1, c->nsel,
                                           vrow, mrows);
                    else
                        hipLaunchKernelGGL(k_sel_run_add<long long>, dim3(blocks), dim3(256), 0, st, (long long)nkeys, ks64, vs, npix1,
                                           c->nsel, vrow, mrows);
                }
            }
            HX_HIP(hipGetLastError());
        }
    }
    return page_close(c, io);
}


extern "C" int hx_catmap_moments_sel(hx_catmap_sel *c, double *out, int64_t *bad, int64_t *fcount)
{
    HX_TRY(ensure_ready());
    if (!c || !out || !bad || !fcount) return fail(HX_ERR_ARG, "hx_catmap_moments_sel: bad arguments");
    hipStream_t st = rt().stream;
    const int nf = c->nfield, width = c->nsel * nf * 4;
    std::vector<double> acc(width);
    std::vector<unsigned long long> cnt(c->n_nan() + c->n_bad() + c->n_fcount() + 1);
    HX_HIP(hipMemcpyAsync(acc.data(), c->acc.p, sizeof(double) * width, hipMemcpyDeviceToHost, st));
    HX_HIP(hipMemcpyAsync(cnt.data(), c->counters.p, sizeof(unsigned long long) * cnt.size(), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    const unsigned long long *nan = cnt.data(), *nbad = nan + c->n_nan(), *fc = nbad + c->n_bad();
    for (int s = 0; s < c->nsel; ++s) {
        for (int f = 0; f < nf; ++f) {
            const int sf = s * nf + f;
            for (int k = 0; k < 4; ++k) out[4 * sf + k] = acc[4 * sf + k];
            for (int k = 0; k < 5; ++k) bad[6 * sf + k] = (int64_t)nan[5 * sf + k];
            bad[6 * sf + 5] = (int64_t)nbad[s * c->ngroup + c->grp[f]];
        }
        for (int k = 0; k <= c->nfilt; ++k) fcount[(c->nfilt + 1) * s + k] = (int64_t)fc[(c->nfilt + 1) * s + k];
    }
    return HX_OK;
}

extern "C" int hx_catmap_finish_sel(hx_catmap_sel *c, int sel, int field, double norm, const double *vis)
{
    return cat_finish(c, "hx_catmap_finish_sel", sel, field, norm, vis);
}

// =====================================================================================
// catalogues -> alms through the point transform (heracles.map_catalogs with a DiscreteMapper: heracles/fields.py:197-559 over
// heracles/ducc.py:92-133)
// =====================================================================================
// The third context on the shared core: the field rules, the moments and the page protocol are those of hx_catmap; what a page adds to is
// not a map but the oversampled (theta, phi) grid of the point transform (hx_nufft.hip), one per component, owned by the context and
// resident from the first page to hx_catalm_finish.  Spreading is additive in the points, so the grid after the last page is the grid of
// the whole catalogue, and the FFT stages and the Legendre analysis run once per field instead of once per page.  Per page and
// (lmax, lon, lat) group: at most one tile sort, shared by every component of the group, then one spread per component.
// The spread adds with hardware float64 atomics: alms are NOT bit-repeatable between runs (unlike the maps of hx_catmap); the moments are.
struct hx_catalm : CatBase {
    AlmArgs args{};
    hx_pointsht *ps[kCatF] = {};   // borrowed: tables, sort buffers, FFT scratch and the equiangular plan of each field's band limit
    long long n1[kCatF] = {}, nlm[kCatF] = {};
    DevBuf grid[kCatF];            // per field: nrow grids [n1][n1]
    DevBuf loc[kCatG];
    ~hx_catalm() { wait(); }
};

static int catalm_init(hx_catalm *c, int64_t page_size, int ncols, int nfields, const int *desc, hx_pointsht *const *ps)
{
    if (page_size < 1 || page_size > 0xfffffff0ll || ncols < 2 || ncols > kCatC || nfields < 1 || nfields > kCatF || !desc || !ps)
        return fail(HX_ERR_ARG, "hx_catalm_create: bad arguments (page_size=%lld ncols=%d nfields=%d; at most %d columns and %d fields)",
                    (long long)page_size, ncols, nfields, kCatC, kCatF);
    AlmArgs &a = c->args;
    HX_TRY(cat_fields_init(c, a.c, "hx_catalm_create", page_size, ncols, nfields, desc, 1, nullptr, 0, 8191));
    hipStream_t st = rt().stream;
    for (int f = 0; f < nfields; ++f) {
        int info[4];
        if (!ps[f] || hx_pointsht_info(ps[f], info) != HX_OK || info[0] != c->nside[f])
            return fail(HX_ERR_ARG, "hx_catalm_create: field %d needs a point transform of lmax %d", f, c->nside[f]);
        c->ps[f] = ps[f];
        c->n1[f] = info[2];
        c->nlm[f] = (long long)(info[0] + 1) * (info[0] + 2) / 2;
        HX_TRY(c->grid[f].alloc(sizeof(double) * (size_t)c->n1[f] * c->n1[f] * c->nrow[f]));
        HX_HIP(hipMemsetAsync(c->grid[f].p, 0, c->grid[f].bytes, st));
    }
    for (int g = 0; g < c->ngroup; ++g) {
        HX_TRY(c->loc[g].alloc(sizeof(double2) * page_size));
        a.loc[g] = c->loc[g].as<double2>();
    }
    HX_TRY(cat_sums_init(c, nfields * 4, 5 * kCatF + kCatG));
    a.slab = c->slab.as<double>();
    a.nan = c->counters.as<unsigned long long>();
    a.nbad = a.nan + 5 * kCatF;
    return HX_OK;
}

extern "C" hx_catalm *hx_catalm_create(int64_t page_size, int ncols, int nfields, const int *desc, hx_pointsht *const *ps)
{
    if (ensure_ready() != HX_OK) return nullptr;
    hx_catalm *c = new hx_catalm;
    if (catalm_init(c, page_size, ncols, nfields, desc, ps) != HX_OK) {
        delete c;
        return nullptr;
    }
    return c;
}

extern "C" void hx_catalm_destroy(hx_catalm *c) { delete c; }

extern "C" int hx_catalm_page(hx_catalm *c, int64_t n, const double *const *cols)
{
    HX_TRY(ensure_ready());
    PageIO io;
    HX_TRY(page_open(c, "hx_catalm_page", n, cols, nullptr, &io));
    if (n == 0) return HX_OK;
    AlmArgs a = c->args;
    std::copy(io.col, io.col + kCatC, a.c.col);
    hipStream_t st = rt().stream;
    const unsigned nblocks = (unsigned)std::min<long long>((n + 255) / 256, kCatBlocks);
    {
        ProfScope ps("catalm_prepare");
        switch (c->nfield) {
#define HX_CAT_PREP(NF) case NF: hipLaunchKernelGGL(k_catalm_prepare<NF>, dim3(nblocks), dim3(256), 0, st, (long long)n, a); break;
            HX_CAT_PREP(1) HX_CAT_PREP(2) HX_CAT_PREP(3) HX_CAT_PREP(4) HX_CAT_PREP(5) HX_CAT_PREP(6) HX_CAT_PREP(7) HX_CAT_PREP(8)
#undef HX_CAT_PREP
        }
        hipLaunchKernelGGL(k_cat_reduce, dim3(1), dim3(256), 0, st, (int)nblocks, c->nfield * 4, c->slab.as<double>(), c->acc.as<double>());
        HX_HIP(hipGetLastError());
    }
    // The spread kernels count the points they reject (a colatitude outside [0, pi], a non-finite value) in ps->nbad.  That counter is
    // deliberately not read here: k_catalm_prepare wrote only valid locations, and a NaN value on a kept row is in the NaN counters,
    // from which the caller raises.  hx_pointsht_adjoint clears the counter before its own use.
    for (int g = 0; g < c->ngroup; ++g) {
        ProfScope pf("catalm_spread");
        hx_pointsht *ps = nullptr;
        PointOrder order;
        for (int f = 0; f < c->nfield; ++f) {
            if (c->grp[f] != g) continue;
            if (!ps) {  // (the fields of a group share the band limit, hence the transform: one order for all their components)
                ps = c->ps[f];
                HX_TRY(pointsht_order(ps, n, a.loc[g], &order));
            }
            for (int r = 0; r < c->nrow[f]; ++r)
                HX_TRY(pointsht_spread_one(ps, order, n, a.loc[g], c->val[f].as<double>() + r * c->cap,
                                           c->grid[f].as<double>() + (size_t)r * c->n1[f] * c->n1[f]));
        }
    }
    return page_close(c, io);
}

extern "C" int hx_catalm_moments(hx_catalm *c, double *out, int64_t *bad) { return cat_moments(c, "hx_catalm_moments", out, bad); }

extern "C" int hx_catalm_finish(hx_catalm *c, int field, int spin, double norm, const double *vis_alm, double *alm)
{
    HX_TRY(ensure_ready());
    if (!c || field < 0 || field >= c->nfield || !alm) return fail(HX_ERR_ARG, "hx_catalm_finish: bad arguments");
    if (spin < 0) return fail(HX_ERR_ARG, "hx_catalm_finish: negative spin weight %d", spin);
    const int nrow = c->nrow[field];
    if (spin > 0 && nrow != 2) return fail(HX_ERR_ARG, "hx_catalm_finish: a spin-%d field has two components (field %d has one)", spin, field);
    const long long nlm = c->nlm[field];
    const size_t gsz = (size_t)c->n1[field] * c->n1[field];
    InView vv;
    OutView va;
    HX_TRY(vv.bind(vis_alm, sizeof(double) * 2 * nlm));
    HX_TRY(va.bind(alm, sizeof(double) * 2 * nlm * nrow));
    {
        ProfScope ps("catalm_finish");
        const double *grids = c->grid[field].as<double>();
        const GridOf resident = [&](int r, const double **grid) -> int {
            *grid = grids + (size_t)r * gsz;
            return HX_OK;
        };
        HX_TRY(pointsht_grids_to_alm(c->ps[field], spin, nrow, resident, va.as<double2>()));
        // alm <- alm / norm - vis_alm on the real and imaginary parts: k_cat_finish over rows of 2 nlm doubles
        const long long total = 2 * nlm * nrow;
        const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 65536);
        hipLaunchKernelGGL(k_cat_finish, dim3(blocks), dim3(256), 0, rt().stream, 2 * nlm, nrow, va.as<double>(), norm, vv.as<double>());
        HX_HIP(hipGetLastError());
    }
    HX_TRY(va.finish());
    HX_HIP(hipStreamSynchronize(rt().stream));  // (a staged visibility dies with this scope)
    return HX_OK;
}
