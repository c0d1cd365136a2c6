// hx_masktools.hip -- disc and convex-polygon holes, the distance to the nearest masked pixel and the C1 / C2 apodisation of a HEALPix
// mask.  The definition lives in hx_masktools.h; this file is launch shape only.  gfx950 only.
//
//   k_mt_validate     one work item per pixel (work-groups stride over the map): the first pixel whose value is NaN or infinite
//                     (atomicMin), the number of masked pixels (integer atomicAdd per work-group).
//   k_mt_disc_check   one work item per disc: the first invalid disc (atomicMin); the discs whose estimated pixel count exceeds WIDE_MIN
//                     (all of them with HX_MASK_WIDE=1) are appended to a list -- in any order: every writer below stores the same 0.0.
//   k_mt_disc_small   one work item per remaining disc: its rings, on each the pixels of the phi window, the rule on every one.
//   k_mt_disc_wide    one work-group per listed disc: waves over the rings, lanes over the window.
//   k_mt_neighbours   one work-group per ring: the left / right tables as two inclusive max-scans (forward, and over the reversed
//                     ring), 256 pixels per step with the running value carried; the ring's first and last masked index.
//   k_mt_distance     one work item per pixel: hxmask::nearest_h over the tables; writes H, or mask x taper(H) (the fused epilogue).
//                     Each work item reads mask[p] before it writes out[p] and the search reads the tables only: out may alias mask.
//   k_mp_offsets      (polygons) one work item per polygon: the first vertex count outside 3 .. 64 (atomicMin).
//   k_mp_check        one work item per polygon: its vertices and its signed edge normals (with rho and phi_e of each for the windows)
//                     into two buffers, the first invalid polygon (atomicMin), the wide list by the pixel estimate of the bounding cap.
//   k_mp_small        one work item per remaining polygon: the rings of its cap, the clipped window, the rule.
//   k_mp_wide         one work-group per listed polygon: its edges staged in LDS once, waves over the rings, lanes over the window.
// No floating-point atomics; vector stores only.
#include <cstdlib>

#include "hx_common.h"
#include "hx_masktools.h"

namespace hx {

namespace {

constexpr int MT_BLOCK = 256, MT_NW = MT_BLOCK / 64;
constexpr unsigned long long MT_CLEAR = ~0ull;

struct MtWords {
    unsigned long long bad, count;
};

__global__ __launch_bounds__(MT_BLOCK) void k_mt_validate(long long npix, const double *mask, MtWords *__restrict__ words)
{
    __shared__ unsigned lds[MT_NW];
    unsigned c = 0;
    for (long long p = (long long)blockIdx.x * MT_BLOCK + threadIdx.x; p < npix; p += (long long)gridDim.x * MT_BLOCK) {
        const double m = mask[p];
        if (!hxmask::finite(m)) atomicMin(&words->bad, (unsigned long long)p);
        else if (hxmask::is_masked(m)) ++c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < MT_NW; ++w) s += lds[w];
        if (s) atomicAdd(&words->count, s);
    }
}

__device__ __forceinline__ double radius_of(const double *__restrict__ radius, double radius_all, long long k) { return radius ? radius[k] : radius_all; }

__global__ __launch_bounds__(MT_BLOCK) void k_mt_disc_check(long long nside, long long ndisc, const double *__restrict__ lon, const double *__restrict__ lat,
                                                           const double *__restrict__ radius, double radius_all, int force_wide,
                                                           MtWords *__restrict__ words, unsigned *__restrict__ wide)
{
    const long long k = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (k >= ndisc) return;
    const double r = radius_of(radius, radius_all, k);
    if (!hxmask::disc_valid(lon[k], lat[k], r)) {
        atomicMin(&words->bad, (unsigned long long)k);
        return;
    }
    if (force_wide || hxmask::disc_pixels(nside, hxmask::angle_h(r)) > hxmask::WIDE_MIN) {
        const unsigned long long i = atomicAdd(&words->count, 1ull);
        if (i < (unsigned long long)ndisc) wide[i] = (unsigned)k;
    }
}

// the pixels k0 + lane0, k0 + lane0 + stride, ... of the window of disc d on ring ir
__device__ __forceinline__ void disc_ring(long long nside, long long npix, long long ir, const hxmask::Disc &d, int lane0, int stride, double *mask)
{
    const hxmask::Ring r = hxmask::ring_info(nside, ir);
    const hxmask::Window w = hxmask::disc_window(r, d);
    for (long long i = lane0; i < w.count; i += stride) {
        const long long j = hxmask::wrap_index(w.k0 + i, r.n), p = r.first + j;
        if (p >= 0 && p < npix && hxmask::disc_hit(r, j, d)) mask[p] = 0.0;
    }
}

__global__ __launch_bounds__(MT_BLOCK) void k_mt_disc_small(long long nside, long long npix, long long ndisc, const double *__restrict__ lon,
                                                           const double *__restrict__ lat, const double *__restrict__ radius, double radius_all,
                                                           double *mask)
{
    const long long k = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (k >= ndisc) return;
    const double rad = radius_of(radius, radius_all, k);
    if (hxmask::disc_pixels(nside, hxmask::angle_h(rad)) > hxmask::WIDE_MIN) return;
    const hxmask::Disc d = hxmask::make_disc(lon[k], lat[k], rad);
    long long lo, hi;
    hxmask::disc_rings(nside, d, &lo, &hi);
    for (long long ir = lo; ir <= hi; ++ir) disc_ring(nside, npix, ir, d, 0, 1, mask);
}

__global__ __launch_bounds__(MT_BLOCK) void k_mt_disc_wide(long long nside, long long npix, const unsigned *__restrict__ wide, const double *__restrict__ lon,
                                                          const double *__restrict__ lat, const double *__restrict__ radius, double radius_all, double *mask)
{
    const long long k = (long long)wide[blockIdx.x];
    const hxmask::Disc d = hxmask::make_disc(lon[k], lat[k], radius_of(radius, radius_all, k));
    long long lo, hi;
    hxmask::disc_rings(nside, d, &lo, &hi);
    for (long long ir = lo + (threadIdx.x >> 6); ir <= hi; ir += MT_NW) disc_ring(nside, npix, ir, d, (int)(threadIdx.x & 63), 64, mask);
}

// ---- convex polygons ----
// the first polygon whose vertex count lies outside POLY_MIN .. POLY_MAX (offsets[0] != 0 counts against polygon 0): no other kernel
// reads offsets, lon or lat before this one has passed
__global__ __launch_bounds__(MT_BLOCK) void k_mp_offsets(long long npoly, const long long *__restrict__ offsets, MtWords *__restrict__ words)
{
    const long long k = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (k >= npoly) return;
    const long long a = offsets[k], n = offsets[k + 1] - a;
    if ((k == 0 && a != 0) || !hxmask::count_valid(n)) atomicMin(&words->bad, (unsigned long long)k);
}

// one work item per polygon: its vertices into verts, validity (the first invalid polygon as 2 k + reason by atomicMin; reason 0: a
// coordinate, 1: the shape), its edges into edges, and the wide list as for discs, by the estimated pixel count of the bounding cap
__global__ __launch_bounds__(MT_BLOCK) void k_mp_check(long long nside, long long npoly, const long long *__restrict__ offsets, const double *__restrict__ lon,
                                                      const double *__restrict__ lat, int force_wide, double *verts, hxmask::Edge *__restrict__ edges,
                                                      MtWords *__restrict__ words, unsigned *__restrict__ wide)
{
    const long long k = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (k >= npoly) return;
    const long long o = offsets[k];
    const int n = (int)(offsets[k + 1] - o);
    double *v = verts + 3 * o;
    for (int i = 0; i < n; ++i) {
        const double lo = lon[o + i], la = lat[o + i];
        if (!hxmask::vertex_valid(lo, la)) {
            atomicMin(&words->bad, 2ull * (unsigned long long)k);
            return;
        }
        hxmask::make_vertex(lo, la, v + 3 * i);
    }
    int sigma;
    if (!hxmask::poly_valid(n, v, &sigma)) {
        atomicMin(&words->bad, 2ull * (unsigned long long)k + 1ull);
        return;
    }
    for (int i = 0; i < n; ++i) edges[o + i] = hxmask::make_edge(v + 3 * i, v + 3 * (i + 1 < n ? i + 1 : 0), sigma);
    hxmask::Disc cap;
    const bool capped = hxmask::poly_cap(n, v, &cap);
    if (force_wide || !capped || hxmask::disc_pixels(nside, cap.hr) > hxmask::WIDE_MIN) {
        const unsigned long long i = atomicAdd(&words->count, 1ull);
        if (i < (unsigned long long)npoly) wide[i] = (unsigned)k;
    }
}

// the pixels k0 + lane0, k0 + lane0 + stride, ... of the window of the polygon on ring ir
__device__ __forceinline__ void poly_ring(long long nside, long long npix, long long ir, bool capped, const hxmask::Disc &cap, int n, const hxmask::Edge *e,
                                          int lane0, int stride, double value, double *mask)
{
    const hxmask::Ring r = hxmask::ring_info(nside, ir);
    const hxmask::Window w = hxmask::poly_window(r, capped, cap, n, e);
    for (long long i = lane0; i < w.count; i += stride) {
        const long long j = hxmask::wrap_index(w.k0 + i, r.n), p = r.first + j;
        if (p >= 0 && p < npix && hxmask::poly_hit(r, j, n, e)) mask[p] = value;
    }
}

__global__ __launch_bounds__(MT_BLOCK) void k_mp_small(long long nside, long long npix, long long npoly, const long long *__restrict__ offsets,
                                                      const double *__restrict__ verts, const hxmask::Edge *__restrict__ edges, double value, double *mask)
{
    const long long k = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (k >= npoly) return;
    const long long o = offsets[k];
    const int n = (int)(offsets[k + 1] - o);
    hxmask::Disc cap;
    if (!hxmask::poly_cap(n, verts + 3 * o, &cap) || hxmask::disc_pixels(nside, cap.hr) > hxmask::WIDE_MIN) return;
    long long lo, hi;
    hxmask::poly_rings(nside, true, cap, &lo, &hi);
    for (long long ir = lo; ir <= hi; ++ir) poly_ring(nside, npix, ir, true, cap, n, edges + o, 0, 1, value, mask);
}

__global__ __launch_bounds__(MT_BLOCK) void k_mp_wide(long long nside, long long npix, const unsigned *__restrict__ wide, const long long *__restrict__ offsets,
                                                     const double *__restrict__ verts, const hxmask::Edge *__restrict__ edges, double value, double *mask)
{
    __shared__ hxmask::Edge lds[hxmask::POLY_MAX];
    const long long k = (long long)wide[blockIdx.x], o = offsets[k];
    const int n = (int)(offsets[k + 1] - o);
    if ((int)threadIdx.x < n) lds[threadIdx.x] = edges[o + threadIdx.x];
    hxmask::Disc cap;
    const bool capped = hxmask::poly_cap(n, verts + 3 * o, &cap);
    long long lo, hi;
    hxmask::poly_rings(nside, capped, cap, &lo, &hi);
    __syncthreads();
    for (long long ir = lo + (threadIdx.x >> 6); ir <= hi; ir += MT_NW) poly_ring(nside, npix, ir, capped, cap, n, lds, (int)(threadIdx.x & 63), 64, value, mask);
}

// inclusive running maximum of v over the work-group in thread order; total: the maximum of all
__device__ __forceinline__ int block_inclusive_max(int v, int *lds /* [MT_NW] */, int &total)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(v, o, 64);
        if ((int)(threadIdx.x & 63) >= o) v = y > v ? y : v;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) lds[w] = v;
    __syncthreads();
    int before = -1, all = -1;
#pragma unroll
    for (int k = 0; k < MT_NW; ++k) {
        const int s = lds[k];
        if (k < w) before = s > before ? s : before;
        all = s > all ? s : all;
    }
    __syncthreads();
    total = all;
    return before > v ? before : v;
}

__global__ __launch_bounds__(MT_BLOCK) void k_mt_neighbours(long long nside, long long npix, const double *__restrict__ mask, unsigned *__restrict__ left,
                                                           unsigned *__restrict__ right, unsigned *__restrict__ first, unsigned *__restrict__ last)
{
    __shared__ int lds[MT_NW];
    const long long ir = (long long)blockIdx.x + 1;
    const hxmask::Ring r = hxmask::ring_info(nside, ir);
    const int n = (int)r.n;
    int carry_l = -1, carry_r = -1;  // forward: the last masked index so far; reversed: the same in reversed indices
    for (int base = 0; base < n; base += MT_BLOCK) {
        const int j = base + (int)threadIdx.x, jr = n - 1 - j;
        const long long pl = r.first + j, pr = r.first + jr;
        const bool in = j < n && pl >= 0 && pr >= 0 && pl < npix && pr < npix;
        int total;
        int v = (in && hxmask::is_masked(mask[pl])) ? j : -1;
        v = block_inclusive_max(v, lds, total);
        v = carry_l > v ? carry_l : v;
        carry_l = total > carry_l ? total : carry_l;
        if (in) left[pl] = v < 0 ? hxmask::NONE : (unsigned)v;
        v = (in && hxmask::is_masked(mask[pr])) ? j : -1;
        v = block_inclusive_max(v, lds, total);
        v = carry_r > v ? carry_r : v;
        carry_r = total > carry_r ? total : carry_r;
        if (in) right[pr] = v < 0 ? hxmask::NONE : (unsigned)(n - 1 - v);
    }
    if (threadIdx.x == 0) {
        last[ir] = carry_l < 0 ? hxmask::NONE : (unsigned)carry_l;
        first[ir] = carry_r < 0 ? hxmask::NONE : (unsigned)(n - 1 - carry_r);
        if (ir == 1) first[0] = last[0] = hxmask::NONE;
    }
}

// KIND 0: out = H; else out = mask x taper(H).  empty: the mask has no masked pixel, H is the cap everywhere.
__global__ __launch_bounds__(MT_BLOCK) void k_mt_distance(long long nside, long long npix, const double *mask, hxmask::Neighbours nb, double cap, int kind,
                                                         int empty, double *out)
{
    for (long long p = (long long)blockIdx.x * MT_BLOCK + threadIdx.x; p < npix; p += (long long)gridDim.x * MT_BLOCK) {
        const double m = mask[p];
        const bool masked = hxmask::is_masked(m);
        const double H = masked ? 0.0 : (empty ? cap : hxmask::nearest_h(nside, p, cap, nb, nullptr));
        out[p] = kind == 0 ? H : (masked ? 0.0 : m * hxmask::taper_of_h(kind, H, cap));
    }
}

unsigned stride_grid(long long items, int per_cu)
{
    const long long need = (items + MT_BLOCK - 1) / MT_BLOCK, cap = (long long)rt().cus * per_cu;
    return (unsigned)(need < 1 ? 1 : (need < cap ? need : cap));
}

// the first NaN or infinite pixel and the number of masked pixels of mask [npix] on the device; complete on return
int validate_mask(const char *who, long long npix, const double *mask, DevBuf &words, unsigned long long *nmasked)
{
    hipStream_t st = rt().stream;
    HX_TRY(words.alloc(sizeof(MtWords)));
    const MtWords init = {MT_CLEAR, 0ull};
    MtWords got;
    HX_HIP(hipMemcpyAsync(words.p, &init, sizeof(init), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_mt_validate, dim3(stride_grid(npix, 16)), dim3(MT_BLOCK), 0, st, npix, mask, words.as<MtWords>());
    HX_HIP(hipGetLastError());
    HX_HIP(hipMemcpyAsync(&got, words.p, sizeof(got), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (got.bad != MT_CLEAR) return fail(HX_ERR_ARG, "%s: the mask value of pixel %llu is NaN or infinite", who, got.bad);
    *nmasked = got.count;
    return HX_OK;
}

bool overlap(const void *a, const void *b, size_t bytes)
{
    const char *x = (const char *)a, *y = (const char *)b;
    return x < y + bytes && y < x + bytes;
}

// hx_mask_distance (kind 0) and hx_mask_taper (a kind it has validated)
int distance_call(const char *who, int nside, const double *mask, double degrees, int kind, double *out)
{
    HX_TRY(ensure_ready());
    if (nside < 1 || nside > 8192) return fail(HX_ERR_ARG, "%s: nside = %d, 1 .. 8192 are supported", who, nside);
    if (!mask || !out) return fail(HX_ERR_ARG, "%s: null pointer", who);
    if (!(degrees > 0.0 && degrees <= 180.0)) return fail(HX_ERR_ARG, "%s: an angle of %g degrees, (0, 180] is supported", who, degrees);
    const long long npix = 12ll * nside * nside;
    const size_t bytes = sizeof(double) * (size_t)npix;
    if ((const void *)mask != (const void *)out && overlap(mask, out, bytes)) return fail(HX_ERR_ARG, "%s: the output overlaps the mask without being the mask", who);
    hipStream_t st = rt().stream;
    InView vm;
    HX_TRY(vm.bind(mask, bytes));
    DevBuf words, left, right, rings;
    unsigned long long nmasked = 0;
    HX_TRY(validate_mask(who, npix, vm.as<double>(), words, &nmasked));
    hxmask::Neighbours nb = {nullptr, nullptr, nullptr, nullptr};
    if (nmasked) {
        HX_TRY(left.alloc(sizeof(unsigned) * (size_t)npix));
        HX_TRY(right.alloc(sizeof(unsigned) * (size_t)npix));
        HX_TRY(rings.alloc(sizeof(unsigned) * 8 * (size_t)nside));
        nb.left = left.as<unsigned>();
        nb.right = right.as<unsigned>();
        nb.first = rings.as<unsigned>();
        nb.last = rings.as<unsigned>() + 4 * (size_t)nside;
        ProfScope prof("mask_neighbours");
        hipLaunchKernelGGL(k_mt_neighbours, dim3((unsigned)(4 * nside - 1)), dim3(MT_BLOCK), 0, st, (long long)nside, npix, vm.as<double>(), left.as<unsigned>(),
                           right.as<unsigned>(), rings.as<unsigned>(), rings.as<unsigned>() + 4 * (size_t)nside);
        HX_HIP(hipGetLastError());
    }
    OutView vo;
    HX_TRY(vo.bind(out, bytes));
    {
        ProfScope prof("mask_distance");
        hipLaunchKernelGGL(k_mt_distance, dim3(stride_grid(npix, 64)), dim3(MT_BLOCK), 0, st, (long long)nside, npix, vm.as<double>(), nb, hxmask::angle_h(degrees), kind,
                           nmasked ? 0 : 1, vo.as<double>());
    }
    HX_HIP(hipGetLastError());
    HX_TRY(vo.finish());
    HX_HIP(hipStreamSynchronize(st));  // (the buffers are freed on return)
    return HX_OK;
}

}  // namespace

}  // namespace hx

using namespace hx;

extern "C" int hx_mask_discs(int nside, double *mask, int64_t ndisc, const double *lon, const double *lat, const double *radius, double radius_all)
{
    HX_TRY(ensure_ready());
    if (nside < 1 || nside > 8192) return fail(HX_ERR_ARG, "hx_mask_discs: nside = %d, 1 .. 8192 are supported", nside);
    if (ndisc < 0 || ndisc > 0xffffffffll) return fail(HX_ERR_ARG, "hx_mask_discs: ndisc = %lld, 0 .. 2^32 - 1 are supported", (long long)ndisc);
    if (!mask || (ndisc > 0 && (!lon || !lat))) return fail(HX_ERR_ARG, "hx_mask_discs: null pointer");
    const long long npix = 12ll * nside * nside;
    const size_t bytes = sizeof(double) * (size_t)npix;
    hipStream_t st = rt().stream;
    OutView vm;  // in and out: a host map is uploaded here and copied back by finish()
    HX_TRY(vm.bind(mask, bytes));
    if (vm.host) HX_TRY(copy_h2d(vm.dev, mask, bytes));
    DevBuf words, wide;
    unsigned long long nmasked = 0;
    HX_TRY(validate_mask("hx_mask_discs", npix, vm.as<double>(), words, &nmasked));
    if (ndisc == 0) return HX_OK;
    const char *hook = getenv("HX_MASK_WIDE");  // (tests) 1: every disc down the wide path; read at every call
    const bool force_wide = hook && hook[0] == '1';
    InView vlon, vlat, vrad;
    HX_TRY(vlon.bind(lon, sizeof(double) * (size_t)ndisc));
    HX_TRY(vlat.bind(lat, sizeof(double) * (size_t)ndisc));
    HX_TRY(vrad.bind(radius, sizeof(double) * (size_t)ndisc));
    HX_TRY(wide.alloc(sizeof(unsigned) * (size_t)ndisc));
    const MtWords init = {MT_CLEAR, 0ull};
    MtWords got;
    const unsigned nblocks = (unsigned)((ndisc + MT_BLOCK - 1) / MT_BLOCK);
    HX_HIP(hipMemcpyAsync(words.p, &init, sizeof(init), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_mt_disc_check, dim3(nblocks), dim3(MT_BLOCK), 0, st, (long long)nside, (long long)ndisc, vlon.as<double>(), vlat.as<double>(),
                       vrad.as<double>(), radius_all, force_wide ? 1 : 0, words.as<MtWords>(), wide.as<unsigned>());
    HX_HIP(hipGetLastError());
    HX_HIP(hipMemcpyAsync(&got, words.p, sizeof(got), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (got.bad != MT_CLEAR)
        return fail(HX_ERR_ARG, "hx_mask_discs: disc %llu has a NaN or infinite coordinate, |lat| > 90 or a radius outside [0, 180] degrees", got.bad);
    const unsigned long long nwide = got.count < (unsigned long long)ndisc ? got.count : (unsigned long long)ndisc;
    {
        ProfScope prof("mask_discs");
        if (!force_wide && nwide < (unsigned long long)ndisc)
            hipLaunchKernelGGL(k_mt_disc_small, dim3(nblocks), dim3(MT_BLOCK), 0, st, (long long)nside, npix, (long long)ndisc, vlon.as<double>(), vlat.as<double>(),
                               vrad.as<double>(), radius_all, vm.as<double>());
        for (unsigned long long done = 0; done < nwide; done += 0x40000000ull) {
            const unsigned long long part = nwide - done < 0x40000000ull ? nwide - done : 0x40000000ull;
            hipLaunchKernelGGL(k_mt_disc_wide, dim3((unsigned)part), dim3(MT_BLOCK), 0, st, (long long)nside, npix, wide.as<unsigned>() + done, vlon.as<double>(),
                               vlat.as<double>(), vrad.as<double>(), radius_all, vm.as<double>());
        }
    }
    HX_HIP(hipGetLastError());
    HX_TRY(vm.finish());
    HX_HIP(hipStreamSynchronize(st));  // (the buffers are freed on return)
    return HX_OK;
}

extern "C" int hx_mask_polygons(int nside, double *mask, int64_t npoly, const int64_t *offsets, const double *lon, const double *lat, double value)
{
    HX_TRY(ensure_ready());
    if (nside < 1 || nside > 8192) return fail(HX_ERR_ARG, "hx_mask_polygons: nside = %d, 1 .. 8192 are supported", nside);
    if (npoly < 0 || npoly > 0xffffffffll) return fail(HX_ERR_ARG, "hx_mask_polygons: npoly = %lld, 0 .. 2^32 - 1 are supported", (long long)npoly);
    if (!mask || (npoly > 0 && (!offsets || !lon || !lat))) return fail(HX_ERR_ARG, "hx_mask_polygons: null pointer");
    if (!hxmask::finite(value)) return fail(HX_ERR_ARG, "hx_mask_polygons: value is NaN or infinite");
    const long long npix = 12ll * nside * nside;
    const size_t bytes = sizeof(double) * (size_t)npix;
    hipStream_t st = rt().stream;
    OutView vm;  // in and out: a host map is uploaded here and copied back by finish()
    HX_TRY(vm.bind(mask, bytes));
    if (vm.host) HX_TRY(copy_h2d(vm.dev, mask, bytes));
    DevBuf words, wide, verts, edges;
    unsigned long long nmasked = 0;
    HX_TRY(validate_mask("hx_mask_polygons", npix, vm.as<double>(), words, &nmasked));
    if (npoly == 0) return HX_OK;
    const char *hook = getenv("HX_MASK_WIDE");  // (tests) 1: every polygon down the wide path; read at every call
    const bool force_wide = hook && hook[0] == '1';
    // the offsets first: the number of vertices, and the bounds of every later read of lon and lat, come from them
    InView voff, vlon, vlat;
    HX_TRY(voff.bind(offsets, sizeof(long long) * (size_t)(npoly + 1)));
    const MtWords init = {MT_CLEAR, 0ull};
    MtWords got;
    long long nvert = 0;
    const unsigned nblocks = (unsigned)((npoly + MT_BLOCK - 1) / MT_BLOCK);
    HX_HIP(hipMemcpyAsync(words.p, &init, sizeof(init), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_mp_offsets, dim3(nblocks), dim3(MT_BLOCK), 0, st, (long long)npoly, voff.as<long long>(), words.as<MtWords>());
    HX_HIP(hipGetLastError());
    HX_HIP(hipMemcpyAsync(&got, words.p, sizeof(got), hipMemcpyDeviceToHost, st));
    HX_HIP(hipMemcpyAsync(&nvert, voff.as<long long>() + npoly, sizeof(nvert), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (got.bad != MT_CLEAR)
        return fail(HX_ERR_ARG, "hx_mask_polygons: polygon %llu has a vertex count outside 3 .. 64 (offsets must start at 0 and may not decrease)", got.bad);
    HX_TRY(vlon.bind(lon, sizeof(double) * (size_t)nvert));
    HX_TRY(vlat.bind(lat, sizeof(double) * (size_t)nvert));
    HX_TRY(verts.alloc(sizeof(double) * 3 * (size_t)nvert));
    HX_TRY(edges.alloc(sizeof(hxmask::Edge) * (size_t)nvert));
    HX_TRY(wide.alloc(sizeof(unsigned) * (size_t)npoly));
    HX_HIP(hipMemcpyAsync(words.p, &init, sizeof(init), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_mp_check, dim3(nblocks), dim3(MT_BLOCK), 0, st, (long long)nside, (long long)npoly, voff.as<long long>(), vlon.as<double>(), vlat.as<double>(),
                       force_wide ? 1 : 0, verts.as<double>(), edges.as<hxmask::Edge>(), words.as<MtWords>(), wide.as<unsigned>());
    HX_HIP(hipGetLastError());
    HX_HIP(hipMemcpyAsync(&got, words.p, sizeof(got), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (got.bad != MT_CLEAR)
        return fail(HX_ERR_ARG, (got.bad & 1ull) ? "hx_mask_polygons: polygon %llu is not convex (a repeated vertex, a collinear triple, a reflex vertex or antipodal neighbours)"
                                                 : "hx_mask_polygons: polygon %llu has a NaN or infinite coordinate or |lat| > 90",
                    got.bad >> 1);
    const unsigned long long nwide = got.count < (unsigned long long)npoly ? got.count : (unsigned long long)npoly;
    {
        ProfScope prof("mask_polygons");
        if (!force_wide && nwide < (unsigned long long)npoly)
            hipLaunchKernelGGL(k_mp_small, dim3(nblocks), dim3(MT_BLOCK), 0, st, (long long)nside, npix, (long long)npoly, voff.as<long long>(), verts.as<double>(),
                               edges.as<hxmask::Edge>(), value, vm.as<double>());
        for (unsigned long long done = 0; done < nwide; done += 0x40000000ull) {
            const unsigned long long part = nwide - done < 0x40000000ull ? nwide - done : 0x40000000ull;
            hipLaunchKernelGGL(k_mp_wide, dim3((unsigned)part), dim3(MT_BLOCK), 0, st, (long long)nside, npix, wide.as<unsigned>() + done, voff.as<long long>(),
                               verts.as<double>(), edges.as<hxmask::Edge>(), value, vm.as<double>());
        }
    }
    HX_HIP(hipGetLastError());
    HX_TRY(vm.finish());
    HX_HIP(hipStreamSynchronize(st));  // (the buffers are freed on return)
    return HX_OK;
}

extern "C" int hx_mask_distance(int nside, const double *mask, double max_distance, double *H)
{
    return distance_call("hx_mask_distance", nside, mask, max_distance, 0, H);
}

extern "C" int hx_mask_taper(int nside, const double *mask, double aposize, int kind, double *out)
{
    if (!hxmask::kind_valid(kind)) return fail(HX_ERR_ARG, "hx_mask_taper: kind = %d, 1 (C1) and 2 (C2) are supported", kind);
    return distance_call("hx_mask_taper", nside, mask, aposize, kind, out);
}
