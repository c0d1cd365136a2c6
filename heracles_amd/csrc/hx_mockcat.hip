// hx_mockcat.hip -- Poisson-sampled mock catalogues from expected-count maps: counts per pixel, then points with
// values, for a range [pix_begin, pix_end) of RING pixels.  The definition lives in hx_mockcat.h; this file is launch shape only.
// gfx950 only.
//
//   k_mockcat_counts   one work item per pixel (work-groups stride over the range): n_p ~ Poisson(lam_p), inversion below 32, PTRS
//                      above.  An invalid lam records its pixel in a flag word (atomicMin: the first such pixel wins); the block
//                      sums of the counts go to a 64-bit total.  Counts are written to a buffer of the library first, so a
//                      rejected call leaves the caller's array as it was.
//   k_mockcat_narrow   int64 counts -> the 32-bit array the scan of hx_sort.h works on, one extra 0 at the end (so the exclusive scan
//                      ends with the total); negative counts flag their pixel, the 64-bit total guards the 32-bit scan.
//   k_mockcat_points   the hot path, one work item per POINT: point g of the call lies in the pixel p with off[p] <= g < off[p + 1].
//                      k_mockcat_starts finds the pixel of every work-group's first point by binary search over all offsets (one work
//                      item per work-group of the point kernel); every work item of the point kernel then searches only between its
//                      group's pixel and the next group's, a handful of steps (7 at 2 points per pixel) however the counts are
//                      distributed: a pixel of 5000 points spans 20 work-groups that all resolve to it at once, a run of empty
//                      pixels costs its logarithm.  All stores are to index g: consecutive lanes, consecutive addresses.
#include "hx_common.h"
#include "hx_mockcat.h"
#include "hx_sort.h"

namespace hx {

namespace {

constexpr int MC_BLOCK = 256;
constexpr unsigned long long MC_FLAG_CLEAR = ~0ull;
constexpr long long MC_MAX_TOTAL = 0x7fffffffll;  // points of one call: < 2^31

__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long *lds /* [MC_BLOCK / 64] */)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < MC_BLOCK / 64; ++k) s += lds[k];
    return s;
}

__global__ __launch_bounds__(MC_BLOCK) void k_mockcat_counts(long long pix_begin, long long n, const double *__restrict__ lam, uint32_t key0,
                                                            uint32_t key1, uint32_t realisation, long long *__restrict__ counts,
                                                            unsigned long long *__restrict__ flag, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long lds[MC_BLOCK / 64];
    unsigned long long sum = 0;
    for (long long i = (long long)blockIdx.x * MC_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * MC_BLOCK) {
        const double l = lam[i];
        long long c = 0;
        if (hxmock::lambda_valid(l)) c = hxmock::poisson_count(l, (uint32_t)(pix_begin + i), realisation, key0, key1);
        else atomicMin(flag, (unsigned long long)i);
        counts[i] = c;
        sum += (unsigned long long)c;
    }
    const unsigned long long s = block_sum_u64(sum, lds);
    if (threadIdx.x == 0 && s) atomicAdd(total, s);  // one atomic per work-group, a few thousand per call
}

__global__ __launch_bounds__(MC_BLOCK) void k_mockcat_narrow(long long n, const long long *__restrict__ counts, unsigned *__restrict__ off,
                                                            unsigned long long *__restrict__ flag, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long lds[MC_BLOCK / 64];
    unsigned long long sum = 0;
    for (long long i = (long long)blockIdx.x * MC_BLOCK + threadIdx.x; i <= n; i += (long long)gridDim.x * MC_BLOCK) {
        long long c = i < n ? counts[i] : 0;  // off[n] = 0: the scan leaves the total there
        if (c < 0 || c > MC_MAX_TOTAL) {
            atomicMin(flag, (unsigned long long)i);
            c = 0;
        }
        off[i] = (unsigned)c;
        sum += (unsigned long long)c;
    }
    const unsigned long long s = block_sum_u64(sum, lds);
    if (threadIdx.x == 0 && s) atomicAdd(total, s);
}

// largest p in [lo, hi] with off[p] <= g (off is non-decreasing, off[lo] <= g)
__device__ __forceinline__ long long last_not_above(const unsigned *__restrict__ off, long long lo, long long hi, unsigned g)
{
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// starts[b] = the pixel (within the range) of point b MC_BLOCK, the first of work-group b of the point kernel; starts[nblocks] = the
// pixel of the last point.  One work item per work-group of that kernel: the 28 dependent loads of a search over 2 10^8 offsets
// are latency, which a million independent searches hide and one search per resident work-group does not.
__global__ __launch_bounds__(MC_BLOCK) void k_mockcat_starts(long long n, const unsigned *__restrict__ off, unsigned total, unsigned nblocks,
                                                            unsigned *__restrict__ starts)
{
    const unsigned b = blockIdx.x * (unsigned)MC_BLOCK + threadIdx.x;
    if (b > nblocks) return;
    const unsigned g = b < nblocks ? b * (unsigned)MC_BLOCK : total - 1u;
    starts[b] = (unsigned)last_not_above(off, 0, n - 1, g);
}

__global__ __launch_bounds__(MC_BLOCK) void k_mockcat_points(long long nside, long long pix_begin, long long n, const unsigned *__restrict__ off,
                                                            const unsigned *__restrict__ starts, unsigned total, uint32_t key0, uint32_t key1,
                                                            uint32_t realisation, int nval, const double *__restrict__ maps, const double *__restrict__ sigma,
                                                            double *__restrict__ lon, double *__restrict__ lat, double *__restrict__ values,
                                                            long long *__restrict__ pix)
{
    const unsigned g = blockIdx.x * (unsigned)MC_BLOCK + threadIdx.x;  // (total < 2^31: no wrap)
    if (g >= total) return;
    // off[p] <= g < off[p + 1]: the last pixel whose offset is not above g holds point g (empty pixels before it share its offset
    // and are passed over); it lies between the pixels of this work-group's first point and of the next one's
    const long long p = last_not_above(off, starts[blockIdx.x], starts[blockIdx.x + 1], g);
    const uint32_t index = g - off[p], pixel = (uint32_t)(pix_begin + p);
    double lo, la;
    hxmock::point_lonlat(nside, pixel, index, realisation, key0, key1, &lo, &la);
    lon[g] = lo;
    lat[g] = la;
    if (pix) pix[g] = pix_begin + p;
    for (int j = 0; j < nval; ++j) {
        double v = maps[(long long)j * n + p];
        const double s = sigma[j];
        if (s != 0.0) v += s * hxmock::value_noise(pixel, index, (uint32_t)j, realisation, key0, key1);
        values[(long long)j * total + g] = v;
    }
}

int check_range(const char *who, int nside, int64_t pix_begin, int64_t pix_end)
{
    if (nside < 1 || nside > 8192) return fail(HX_ERR_ARG, "%s: nside = %d, 1 .. 8192 are supported", who, nside);
    const int64_t npix = 12ll * nside * nside;
    if (pix_begin < 0 || pix_end < pix_begin || pix_end > npix)
        return fail(HX_ERR_ARG, "%s: pixel range [%lld, %lld) outside the %lld pixels of nside %d", who, (long long)pix_begin, (long long)pix_end,
                    (long long)npix, nside);
    return HX_OK;
}

// work-groups of the two per-pixel kernels: they stride over the pixels, so that a call makes a few thousand atomic additions to
// its total and not one per 256 pixels
unsigned stride_grid(long long items)
{
    const long long need = (items + MC_BLOCK - 1) / MC_BLOCK, cap = (long long)rt().cus * 16;
    return (unsigned)(need < cap ? need : cap);
}

struct Words2 {
    unsigned long long flag, total;
};

}  // namespace

}  // namespace hx

using namespace hx;

extern "C" int hx_mockcat_counts(int nside, int64_t pix_begin, int64_t pix_end, const double *lam, uint64_t seed, uint32_t realisation,
                                 int64_t *counts, int64_t *total)
{
    HX_TRY(ensure_ready());
    HX_TRY(check_range("hx_mockcat_counts", nside, pix_begin, pix_end));
    if (!total) return fail(HX_ERR_ARG, "hx_mockcat_counts: null pointer");
    const long long n = pix_end - pix_begin;
    if (n == 0) {
        *total = 0;
        return HX_OK;
    }
    if (!lam || !counts) return fail(HX_ERR_ARG, "hx_mockcat_counts: null pointer");
    hipStream_t st = rt().stream;
    InView vlam;
    HX_TRY(vlam.bind(lam, sizeof(double) * (size_t)n));
    // the counts go to a buffer of the library first: a rejected call writes nothing
    const bool dev_out = is_device_ptr(counts);
    DevBuf work, words;
    HX_TRY(work.alloc(sizeof(long long) * (size_t)n));
    HX_TRY(words.alloc(sizeof(Words2)));
    const Words2 init = {MC_FLAG_CLEAR, 0ull};
    HX_HIP(hipMemcpyAsync(words.p, &init, sizeof(init), hipMemcpyHostToDevice, st));
    {
        ProfScope prof("mockcat_counts");
        hipLaunchKernelGGL(k_mockcat_counts, dim3(stride_grid(n)), dim3(MC_BLOCK), 0, st, (long long)pix_begin, n,
                           vlam.as<double>(), (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), realisation, work.as<long long>(),
                           &words.as<Words2>()->flag, &words.as<Words2>()->total);
    }
    HX_HIP(hipGetLastError());
    Words2 got;
    HX_HIP(hipMemcpyAsync(&got, words.p, sizeof(got), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (got.flag != MC_FLAG_CLEAR)
        return fail(HX_ERR_ARG, "hx_mockcat_counts: the expected count of pixel %lld is NaN, negative or above 2^30", (long long)(pix_begin + (long long)got.flag));
    if (got.total > (unsigned long long)MC_MAX_TOTAL)
        return fail(HX_ERR_ARG, "hx_mockcat_counts: %llu points in pixels [%lld, %lld), one call makes fewer than 2^31: use pixel ranges", got.total,
                    (long long)pix_begin, (long long)pix_end);
    if (dev_out) {
        HX_HIP(hipMemcpyAsync(counts, work.p, sizeof(long long) * (size_t)n, hipMemcpyDeviceToDevice, st));
        HX_HIP(hipStreamSynchronize(st));  // (the buffer is freed on return)
    } else {
        HX_TRY(copy_d2h(counts, work.p, sizeof(long long) * (size_t)n));
    }
    *total = (int64_t)got.total;
    return HX_OK;
}

extern "C" int hx_mockcat_points(int nside, int64_t pix_begin, int64_t pix_end, const int64_t *counts, uint64_t seed, uint32_t realisation,
                                 int nval, const double *maps, const double *sigma, double *lon, double *lat, double *values, int64_t *pix)
{
    HX_TRY(ensure_ready());
    HX_TRY(check_range("hx_mockcat_points", nside, pix_begin, pix_end));
    if (nval < 0 || nval > 1024) return fail(HX_ERR_ARG, "hx_mockcat_points: nval = %d", nval);
    const long long n = pix_end - pix_begin;
    if (n == 0) return HX_OK;
    if (!counts || (nval > 0 && (!maps || !sigma))) return fail(HX_ERR_ARG, "hx_mockcat_points: null pointer");
    hipStream_t st = rt().stream;
    InView vcounts, vmaps, vsigma;
    HX_TRY(vcounts.bind(counts, sizeof(int64_t) * (size_t)n));
    DevBuf off, words, scan_tmp, starts;
    HX_TRY(off.alloc(sizeof(unsigned) * (size_t)(n + 1)));
    HX_TRY(words.alloc(sizeof(Words2)));
    const Words2 init = {MC_FLAG_CLEAR, 0ull};
    HX_HIP(hipMemcpyAsync(words.p, &init, sizeof(init), hipMemcpyHostToDevice, st));
    {
        ProfScope prof("mockcat_scan");
        hipLaunchKernelGGL(k_mockcat_narrow, dim3(stride_grid(n + 1)), dim3(MC_BLOCK), 0, st, n, (const long long *)vcounts.as<int64_t>(), off.as<unsigned>(),
                           &words.as<Words2>()->flag, &words.as<Words2>()->total);
    }
    HX_HIP(hipGetLastError());
    Words2 got;
    HX_HIP(hipMemcpyAsync(&got, words.p, sizeof(got), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (got.flag != MC_FLAG_CLEAR)
        return fail(HX_ERR_ARG, "hx_mockcat_points: the count of pixel %lld is negative or not below 2^31", (long long)(pix_begin + (long long)got.flag));
    if (got.total > (unsigned long long)MC_MAX_TOTAL)
        return fail(HX_ERR_ARG, "hx_mockcat_points: %llu points in pixels [%lld, %lld), one call makes fewer than 2^31: use pixel ranges", got.total,
                    (long long)pix_begin, (long long)pix_end);
    const unsigned total = (unsigned)got.total;
    if (total == 0) return HX_OK;
    if (!lon || !lat || (nval > 0 && !values)) return fail(HX_ERR_ARG, "hx_mockcat_points: null pointer");
    {   // exclusive scan of the n + 1 narrowed counts in place (hx_sort.h): off[p] = first point of pixel p, off[n] = total
        ProfScope prof("mockcat_scan");
        const unsigned long long e = (unsigned long long)n + 1;
        const unsigned nsb = (unsigned)((e + rsort::SCAN_TILE - 1) / rsort::SCAN_TILE);
        HX_TRY(scan_tmp.alloc(sizeof(unsigned) * (size_t)(nsb + 16)));
        hipLaunchKernelGGL(rsort::k_scan_sums, dim3(nsb), dim3(rsort::SCAN_T), 0, st, off.as<unsigned>(), e, scan_tmp.as<unsigned>());
        hipLaunchKernelGGL(rsort::k_scan_top, dim3(1), dim3(1024), 0, st, scan_tmp.as<unsigned>(), nsb);
        hipLaunchKernelGGL(rsort::k_scan_apply, dim3(nsb), dim3(rsort::SCAN_T), 0, st, off.as<unsigned>(), e, scan_tmp.as<unsigned>());
    }
    HX_HIP(hipGetLastError());
    if (nval > 0) {
        HX_TRY(vmaps.bind(maps, sizeof(double) * (size_t)nval * (size_t)n));
        HX_TRY(vsigma.bind(sigma, sizeof(double) * (size_t)nval));
    }
    OutView vlon, vlat, vval, vpix;
    HX_TRY(vlon.bind(lon, sizeof(double) * (size_t)total));
    HX_TRY(vlat.bind(lat, sizeof(double) * (size_t)total));
    if (nval > 0) HX_TRY(vval.bind(values, sizeof(double) * (size_t)nval * (size_t)total));
    if (pix) HX_TRY(vpix.bind(pix, sizeof(int64_t) * (size_t)total));
    const unsigned nblocks = (total + MC_BLOCK - 1) / MC_BLOCK;
    HX_TRY(starts.alloc(sizeof(unsigned) * (size_t)(nblocks + 1)));
    {
        ProfScope prof("mockcat_points");
        hipLaunchKernelGGL(k_mockcat_starts, dim3((nblocks + 1 + MC_BLOCK - 1) / MC_BLOCK), dim3(MC_BLOCK), 0, st, n, off.as<unsigned>(), total, nblocks,
                           starts.as<unsigned>());
        hipLaunchKernelGGL(k_mockcat_points, dim3(nblocks), dim3(MC_BLOCK), 0, st, (long long)nside, (long long)pix_begin, n, off.as<unsigned>(),
                           starts.as<unsigned>(), total, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), realisation, nval,
                           nval > 0 ? vmaps.as<double>() : nullptr, nval > 0 ? vsigma.as<double>() : nullptr, vlon.as<double>(), vlat.as<double>(),
                           nval > 0 ? vval.as<double>() : nullptr, pix ? (long long *)vpix.as<int64_t>() : nullptr);
    }
    HX_HIP(hipGetLastError());
    HX_TRY(vlon.finish());
    HX_TRY(vlat.finish());
    if (nval > 0) HX_TRY(vval.finish());
    if (pix) HX_TRY(vpix.finish());
    HX_HIP(hipStreamSynchronize(st));  // (the offsets are freed on return)
    return HX_OK;
}
