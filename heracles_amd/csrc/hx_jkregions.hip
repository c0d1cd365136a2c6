// hx_jkregions.hip -- equal-weight segmentation of a weighted footprint into njk compact regions by recursive weighted bisection along
// the principal axis.  The definition lives in hx_jkregions.h; this file is launch shape only.  gfx950 only.
//
// Once per call:
//   k_jk_validate    one work item per pixel (work-groups stride over the map): footprint flag (weight > 0) for the scan of hx_sort.h,
//                    the largest weight (integer atomicMax on the bits of a non-negative double: order-preserving, exact), the first
//                    pixel with a NaN, negative or infinite weight (atomicMin).
//   k_jk_compact     the footprint as an ascending list of pixels with their integer weights; every pixel in segment 0.
// Per level (all segments of a level together; the segments are contiguous ranges of `order`, the arrangement the level before left):
//   k_jk_partials    one work-group per chunk of JK_CHUNK positions of one segment: the 10 FP64 moments of the chunk -- per work item in
//                    position order, across the wave by shuffles, across the four waves in wave order.  No floating-point atomics.
//   k_jk_final       one work-group per segment over its partials in the same fixed order.  The (<= njk) 3 x 3 eigenproblems are solved
//                    on the host from the copied moments.
//   k_jk_keys        per footprint pixel, in ascending pixel order: the 64-bit key of its projection on the axis of its segment.
//   hx_sort.h        8 passes over (key, list index), then the passes of the segment id (<= 12 bits, read through the values by
//                    k_jk_gather): stable, so pixels of equal projection stay in ascending pixel order.
//   k_scan64_*       exclusive 64-bit scan of the integer weights in that order (k_jk_gather again); a segment's own scan is the
//                    difference to the value at its first position (integers: exact).
//   k_jk_targets / k_jk_count   T of every segment; the one position of a segment where "goes left" turns false writes the count.
//   k_jk_relabel     the host clamps the counts and numbers the children; every pixel gets the id of its child.
// At the end k_jk_labels writes first-label-of-segment through the pixel list, and the partial / final pair sums the weights of the
// regions in the same fixed order.
#include <algorithm>

#include "hx_common.h"
#include "hx_jkregions.h"
#include "hx_sort.h"

namespace hx {

namespace {

constexpr int JK_BLOCK = 256, JK_NW = JK_BLOCK / 64;
constexpr int JK_CHUNK = 4096;  // positions per work-group of the segmented reduction
constexpr unsigned long long JK_FLAG_CLEAR = ~0ull;

struct JkWords {
    unsigned long long bad, wmax_bits;
};

// sum of v[0 .. NV) over the work-group in a fixed order: lanes by shuffles, waves in wave order; the result is valid in thread 0
template <int NV>
__device__ __forceinline__ void block_sum_f64(double (&v)[NV], double (*lds)[NV] /* [JK_NW][NV] */)
{
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) lds[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double s = lds[0][k];
#pragma unroll
            for (int w = 1; w < JK_NW; ++w) s += lds[w][k];
            v[k] = s;
        }
    }
}

__global__ __launch_bounds__(JK_BLOCK) void k_jk_validate(long long npix, const double *__restrict__ weight, unsigned *__restrict__ flags /* [npix + 1] */,
                                                         JkWords *__restrict__ words)
{
    __shared__ unsigned long long lds[JK_NW];
    unsigned long long top = 0;
    for (long long i = (long long)blockIdx.x * JK_BLOCK + threadIdx.x; i <= npix; i += (long long)gridDim.x * JK_BLOCK) {
        unsigned f = 0;
        if (i < npix) {
            const double w = weight[i];
            if (!hxjk::weight_valid(w)) atomicMin(&words->bad, (unsigned long long)i);
            else if (w > 0.0) {
                f = 1;
                const unsigned long long b = (unsigned long long)__double_as_longlong(w);
                top = b > top ? b : top;
            }
        }
        flags[i] = f;  // flags[npix] = 0: the scan leaves the size of the footprint there
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_down(top, o, 64);
        top = other > top ? other : top;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = top;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < JK_NW; ++w) top = lds[w] > top ? lds[w] : top;
        if (top) atomicMax(&words->wmax_bits, top);
    }
}

__global__ __launch_bounds__(JK_BLOCK) void k_jk_compact(long long npix, const double *__restrict__ weight, const unsigned *__restrict__ off, double wmax,
                                                        unsigned m, unsigned *__restrict__ pix, unsigned long long *__restrict__ q,
                                                        unsigned *__restrict__ segid)
{
    for (long long p = (long long)blockIdx.x * JK_BLOCK + threadIdx.x; p < npix; p += (long long)gridDim.x * JK_BLOCK) {
        const double w = weight[p];
        if (w > 0.0) {
            const unsigned i = off[p];
            if (i < m) {
                pix[i] = (unsigned)p;
                q[i] = hxjk::quantise(w, wmax);
                segid[i] = 0;
            }
        }
    }
}

// largest s in [0, nseg) with choff[s] <= b (choff non-decreasing, choff[0] = 0 <= b < choff[nseg])
__device__ __forceinline__ unsigned segment_of_chunk(const unsigned *__restrict__ choff, unsigned nseg, unsigned b)
{
    unsigned lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const unsigned mid = (lo + hi + 1) >> 1;
        if (choff[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// MODE 0: the ten moments of (q, v); MODE 1: the plain sum of the weights.  order == nullptr: the ascending list itself.
template <int MODE>
__global__ __launch_bounds__(JK_BLOCK) void k_jk_partials(long long nside, unsigned nseg, const unsigned *__restrict__ start /* [nseg + 1] */,
                                                         const unsigned *__restrict__ choff /* [nseg + 1] */, const unsigned *__restrict__ order,
                                                         const unsigned *__restrict__ pix, const unsigned long long *__restrict__ q,
                                                         const double *__restrict__ weight, double *__restrict__ partial)
{
    constexpr int NV = MODE == 0 ? hxjk::NMOM : 1;
    __shared__ double lds[JK_NW][NV];
    const unsigned b = blockIdx.x;
    const unsigned s = segment_of_chunk(choff, nseg, b);
    const unsigned lo = start[s] + (b - choff[s]) * (unsigned)JK_CHUNK, end = start[s + 1];
    const unsigned hi = end - lo < (unsigned)JK_CHUNK ? end : lo + (unsigned)JK_CHUNK;
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    for (unsigned j = lo + threadIdx.x; j < hi; j += JK_BLOCK) {
        const unsigned i = order ? order[j] : j;
        if constexpr (MODE == 0) {
            double x, y, z;
            hxjk::pix2vec_ring(nside, (long long)pix[i], &x, &y, &z);
            const double w = (double)q[i];
            const double wx = w * x, wy = w * y, wz = w * z;
            v[0] += w;
            v[1] += wx;
            v[2] += wy;
            v[3] += wz;
            v[4] += wx * x;
            v[5] += wx * y;
            v[6] += wx * z;
            v[7] += wy * y;
            v[8] += wy * z;
            v[9] += wz * z;
        } else {
            v[0] += weight[pix[i]];
        }
    }
    block_sum_f64<NV>(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) partial[(size_t)b * NV + k] = v[k];
    }
}

template <int NV>
__global__ __launch_bounds__(JK_BLOCK) void k_jk_final(const unsigned *__restrict__ choff /* [nseg + 1] */, const double *__restrict__ partial,
                                                      double *__restrict__ out /* [nseg][NV] */)
{
    __shared__ double lds[JK_NW][NV];
    const unsigned s = blockIdx.x, lo = choff[s], hi = choff[s + 1];
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    for (unsigned c = lo + threadIdx.x; c < hi; c += JK_BLOCK) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] += partial[(size_t)c * NV + k];
    }
    block_sum_f64<NV>(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) out[(size_t)s * NV + k] = v[k];
    }
}

__global__ __launch_bounds__(JK_BLOCK) void k_jk_keys(unsigned m, long long nside, const unsigned *__restrict__ pix, const unsigned *__restrict__ segid,
                                                     const unsigned *__restrict__ segn, const double *__restrict__ axes /* [nseg][3] */,
                                                     unsigned long long *__restrict__ keys, unsigned *__restrict__ vals)
{
    const unsigned i = blockIdx.x * (unsigned)JK_BLOCK + threadIdx.x;
    if (i >= m) return;
    const unsigned s = segid[i];
    unsigned long long key = 0;
    if (segn[s] >= 2) {
        double x, y, z;
        hxjk::pix2vec_ring(nside, (long long)pix[i], &x, &y, &z);
        const double a[3] = {axes[3 * s], axes[3 * s + 1], axes[3 * s + 2]};
        key = hxjk::order_key(hxjk::project(a, x, y, z));
    }
    keys[i] = key;
    vals[i] = i;
}

// seg[j] = segid[order[j]];  E[j] = q[order[j]], E[m] = 0 (the scan leaves the total there)
__global__ __launch_bounds__(JK_BLOCK) void k_jk_gather(unsigned m, const unsigned *__restrict__ order, const unsigned *__restrict__ segid,
                                                       const unsigned long long *__restrict__ q, unsigned *__restrict__ seg,
                                                       unsigned long long *__restrict__ E)
{
    const unsigned j = blockIdx.x * (unsigned)JK_BLOCK + threadIdx.x;
    if (j > m) return;
    if (j == m) {
        if (E) E[m] = 0;
        return;
    }
    const unsigned i = order[j];
    if (seg) seg[j] = segid[i];
    if (E) E[j] = q[i];
}

// ---- exclusive scan of e 64-bit integers in place: the three kernels of hx_sort.h at twice the width ----
constexpr int S64_T = 256, S64_IPT = 8, S64_TILE = S64_T * S64_IPT;

__device__ __forceinline__ unsigned long long block_exclusive_scan64(unsigned long long v, unsigned long long *lds /* [waves] */,
                                                                     unsigned long long &total)
{
    unsigned long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o, 64);
        if ((int)(threadIdx.x & 63) >= o) x += y;
    }
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 63) lds[w] = x;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int k = 0; k < nw; ++k) {
        const unsigned long long s = lds[k];
        if (k < w) before += s;
        all += s;
    }
    __syncthreads();
    total = all;
    return before + x - v;
}

__global__ __launch_bounds__(S64_T) void k_scan64_sums(const unsigned long long *__restrict__ a, unsigned long long e, unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long lds[8];
    const unsigned long long base = (unsigned long long)blockIdx.x * S64_TILE + (unsigned long long)threadIdx.x * S64_IPT;
    unsigned long long s = 0;
#pragma unroll
    for (int i = 0; i < S64_IPT; ++i)
        if (base + i < e) s += a[base + i];
    unsigned long long total;
    (void)block_exclusive_scan64(s, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void k_scan64_top(unsigned long long *__restrict__ sums, unsigned nb)
{
    __shared__ unsigned long long lds[20];
    const unsigned per = (nb + blockDim.x - 1) / blockDim.x;
    const unsigned lo = min(nb, threadIdx.x * per), hi = min(nb, lo + per);
    unsigned long long s = 0;
    for (unsigned i = lo; i < hi; ++i) s += sums[i];
    unsigned long long total;
    unsigned long long run = block_exclusive_scan64(s, lds, total);
    for (unsigned i = lo; i < hi; ++i) {
        const unsigned long long v = sums[i];
        sums[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(S64_T) void k_scan64_apply(unsigned long long *__restrict__ a, unsigned long long e, const unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long lds[8];
    const unsigned long long base = (unsigned long long)blockIdx.x * S64_TILE + (unsigned long long)threadIdx.x * S64_IPT;
    unsigned long long v[S64_IPT], s = 0;
#pragma unroll
    for (int i = 0; i < S64_IPT; ++i) {
        v[i] = base + i < e ? a[base + i] : 0ull;
        s += v[i];
    }
    unsigned long long total;
    unsigned long long run = sums[blockIdx.x] + block_exclusive_scan64(s, lds, total);
#pragma unroll
    for (int i = 0; i < S64_IPT; ++i) {
        if (base + i < e) a[base + i] = run;
        run += v[i];
    }
}

__global__ __launch_bounds__(JK_BLOCK) void k_jk_targets(unsigned nseg, const unsigned *__restrict__ start, const unsigned *__restrict__ segn,
                                                        const unsigned long long *__restrict__ E, unsigned long long *__restrict__ T)
{
    const unsigned s = blockIdx.x * (unsigned)JK_BLOCK + threadIdx.x;
    if (s >= nseg) return;
    const unsigned n = segn[s];
    T[s] = n >= 2 ? hxjk::split_target(E[start[s + 1]] - E[start[s]], n / 2, n) : 0ull;
}

// 2 E + q grows strictly along a segment, so "goes left" is true on a prefix: the last position of that prefix writes its length
__global__ __launch_bounds__(JK_BLOCK) void k_jk_count(unsigned m, const unsigned *__restrict__ seg, const unsigned *__restrict__ start,
                                                      const unsigned *__restrict__ segn, const unsigned long long *__restrict__ E /* [m + 1] */,
                                                      const unsigned long long *__restrict__ T, unsigned *__restrict__ count)
{
    const unsigned j = blockIdx.x * (unsigned)JK_BLOCK + threadIdx.x;
    if (j >= m) return;
    const unsigned s = seg[j];
    if (segn[s] < 2) return;
    const unsigned first = start[s], end = start[s + 1];
    const unsigned long long base = E[first], t = T[s], e0 = E[j], e1 = E[j + 1];
    if (!hxjk::goes_left(e0 - base, e1 - e0, t)) return;
    if (j + 1 < end && hxjk::goes_left(e1 - base, E[j + 2] - e1, t)) return;  // (j + 2 <= end <= m)
    count[s] = j + 1 - first;
}

__global__ __launch_bounds__(JK_BLOCK) void k_jk_relabel(unsigned m, const unsigned *__restrict__ order, const unsigned *__restrict__ seg,
                                                        const unsigned *__restrict__ start, const unsigned *__restrict__ segn,
                                                        const unsigned *__restrict__ count, const unsigned *__restrict__ newid,
                                                        unsigned *__restrict__ segid)
{
    const unsigned j = blockIdx.x * (unsigned)JK_BLOCK + threadIdx.x;
    if (j >= m) return;
    const unsigned s = seg[j];
    unsigned id = newid[s];
    if (segn[s] >= 2 && j - start[s] >= count[s]) ++id;
    const unsigned i = order[j];
    if (i < m) segid[i] = id;
}

__global__ __launch_bounds__(JK_BLOCK) void k_jk_labels(unsigned m, long long npix, const unsigned *__restrict__ pix, const unsigned *__restrict__ segid,
                                                       const unsigned *__restrict__ first, int32_t *__restrict__ labels)
{
    const unsigned i = blockIdx.x * (unsigned)JK_BLOCK + threadIdx.x;
    if (i >= m) return;
    const unsigned p = pix[i];
    if ((long long)p < npix) labels[p] = (int32_t)first[segid[i]];
}

unsigned stride_grid(long long items)
{
    const long long need = (items + JK_BLOCK - 1) / JK_BLOCK, cap = (long long)rt().cus * 16;
    return (unsigned)(need < cap ? need : cap);
}

inline unsigned blocks_for(unsigned long long items) { return (unsigned)((items + JK_BLOCK - 1) / JK_BLOCK); }

struct Segment {
    unsigned first, n, start, m;  // labels [first, first + n), positions [start, start + m) of the level's arrangement
};

// the segment table of a level on the device: start [nseg + 1] | choff [nseg + 1] | n [nseg] | count [nseg] | newid [nseg] | first [nseg]
struct Table {
    DevBuf buf;
    unsigned cap = 0;
    unsigned *start() const { return buf.as<unsigned>(); }
    unsigned *choff() const { return start() + cap + 1; }
    unsigned *n() const { return choff() + cap + 1; }
    unsigned *count() const { return n() + cap; }
    unsigned *newid() const { return count() + cap; }
    unsigned *first() const { return newid() + cap; }
    int alloc(unsigned njk)
    {
        cap = njk;
        return buf.alloc(sizeof(unsigned) * ((size_t)6 * cap + 2));
    }
};

// uploads start / choff / n / first of `segs`; split_only: chunks for the segments with n >= 2 only.  Returns the number of chunks.
int upload_segments(const Table &tb, const std::vector<Segment> &segs, bool split_only, hipStream_t st, unsigned *nchunks)
{
    const unsigned nseg = (unsigned)segs.size();
    std::vector<unsigned> start(nseg + 1), choff(nseg + 1), n(nseg), first(nseg);
    unsigned c = 0;
    for (unsigned s = 0; s < nseg; ++s) {
        start[s] = segs[s].start;
        choff[s] = c;
        n[s] = segs[s].n;
        first[s] = segs[s].first;
        if (!split_only || segs[s].n >= 2) c += (segs[s].m + JK_CHUNK - 1) / JK_CHUNK;
    }
    start[nseg] = segs[nseg - 1].start + segs[nseg - 1].m;
    choff[nseg] = c;
    *nchunks = c;
    HX_HIP(hipMemcpyAsync(tb.start(), start.data(), sizeof(unsigned) * (nseg + 1), hipMemcpyHostToDevice, st));
    HX_HIP(hipMemcpyAsync(tb.choff(), choff.data(), sizeof(unsigned) * (nseg + 1), hipMemcpyHostToDevice, st));
    HX_HIP(hipMemcpyAsync(tb.n(), n.data(), sizeof(unsigned) * nseg, hipMemcpyHostToDevice, st));
    HX_HIP(hipMemcpyAsync(tb.first(), first.data(), sizeof(unsigned) * nseg, hipMemcpyHostToDevice, st));
    HX_HIP(hipStreamSynchronize(st));  // (the vectors go out of scope)
    return HX_OK;
}

}  // namespace

}  // namespace hx

using namespace hx;

extern "C" int hx_jk_regions(int nside, const double *weight, int njk, int32_t *labels, double *region_weight, double *axes)
{
    HX_TRY(ensure_ready());
    if (nside < 1 || nside > 8192) return fail(HX_ERR_ARG, "hx_jk_regions: nside = %d, 1 .. 8192 are supported", nside);
    if (njk < 1 || njk > hxjk::NJK_MAX) return fail(HX_ERR_ARG, "hx_jk_regions: njk = %d, 1 .. %d are supported", njk, hxjk::NJK_MAX);
    if (!weight || !labels) return fail(HX_ERR_ARG, "hx_jk_regions: null pointer");
    const long long npix = 12ll * nside * nside;
    hipStream_t st = rt().stream;
    InView vw;
    HX_TRY(vw.bind(weight, sizeof(double) * (size_t)npix));

    // ---- footprint, largest weight, validity ----
    DevBuf off, words, scan_tmp;
    HX_TRY(off.alloc(sizeof(unsigned) * (size_t)(npix + 1)));
    HX_TRY(words.alloc(sizeof(JkWords)));
    const JkWords init = {JK_FLAG_CLEAR, 0ull};
    HX_HIP(hipMemcpyAsync(words.p, &init, sizeof(init), hipMemcpyHostToDevice, st));
    {
        ProfScope prof("jk_compact");
        hipLaunchKernelGGL(k_jk_validate, dim3(stride_grid(npix + 1)), dim3(JK_BLOCK), 0, st, npix, vw.as<double>(), off.as<unsigned>(), words.as<JkWords>());
        const unsigned long long e = (unsigned long long)npix + 1;
        const unsigned nsb = (unsigned)((e + rsort::SCAN_TILE - 1) / rsort::SCAN_TILE);
        HX_TRY(scan_tmp.alloc(sizeof(unsigned) * (size_t)(nsb + 16)));
        hipLaunchKernelGGL(rsort::k_scan_sums, dim3(nsb), dim3(rsort::SCAN_T), 0, st, off.as<unsigned>(), e, scan_tmp.as<unsigned>());
        hipLaunchKernelGGL(rsort::k_scan_top, dim3(1), dim3(1024), 0, st, scan_tmp.as<unsigned>(), nsb);
        hipLaunchKernelGGL(rsort::k_scan_apply, dim3(nsb), dim3(rsort::SCAN_T), 0, st, off.as<unsigned>(), e, scan_tmp.as<unsigned>());
    }
    HX_HIP(hipGetLastError());
    JkWords got;
    unsigned m = 0;
    HX_HIP(hipMemcpyAsync(&got, words.p, sizeof(got), hipMemcpyDeviceToHost, st));
    HX_HIP(hipMemcpyAsync(&m, off.as<unsigned>() + npix, sizeof(m), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (got.bad != JK_FLAG_CLEAR) return fail(HX_ERR_ARG, "hx_jk_regions: the weight of pixel %llu is NaN, negative or infinite", got.bad);
    if (m < (unsigned)njk) return fail(HX_ERR_ARG, "hx_jk_regions: the footprint has %u pixels, fewer than njk = %d", m, njk);
    double wmax;
    std::memcpy(&wmax, &got.wmax_bits, sizeof wmax);

    // ---- buffers of the call ----
    DevBuf pix, segid, q, keyA, keyB, valA, valB, sort_tmp, partial, moments, daxes, targets, scan64;
    Table tb;
    HX_TRY(pix.alloc(sizeof(unsigned) * (size_t)m));
    HX_TRY(segid.alloc(sizeof(unsigned) * (size_t)m));
    HX_TRY(q.alloc(sizeof(unsigned long long) * (size_t)m));
    HX_TRY(tb.alloc((unsigned)njk));
    const unsigned max_chunks = m / JK_CHUNK + (unsigned)njk + 1;
    HX_TRY(partial.alloc(sizeof(double) * hxjk::NMOM * (size_t)max_chunks));
    HX_TRY(moments.alloc(sizeof(double) * hxjk::NMOM * (size_t)njk));
    {
        ProfScope prof("jk_compact");
        hipLaunchKernelGGL(k_jk_compact, dim3(stride_grid(npix)), dim3(JK_BLOCK), 0, st, npix, vw.as<double>(), off.as<unsigned>(), wmax, m, pix.as<unsigned>(),
                           q.as<unsigned long long>(), segid.as<unsigned>());
    }
    HX_HIP(hipGetLastError());

    std::vector<Segment> segs(1, Segment{1u, (unsigned)njk, 0u, m});
    std::vector<double> axes_host(njk > 1 ? 3 * (size_t)(njk - 1) : 0, 0.0);
    const unsigned *order = nullptr;  // the arrangement the last level left (nullptr: the ascending list)
    if (njk > 1) {
        HX_TRY(keyA.alloc(sizeof(unsigned long long) * ((size_t)m + 1)));
        HX_TRY(keyB.alloc(sizeof(unsigned long long) * ((size_t)m + 1)));
        HX_TRY(valA.alloc(sizeof(unsigned) * (size_t)m));
        HX_TRY(valB.alloc(sizeof(unsigned) * (size_t)m));
        HX_TRY(daxes.alloc(sizeof(double) * 3 * (size_t)njk));
        HX_TRY(targets.alloc(sizeof(unsigned long long) * (size_t)njk));
        const unsigned long long e64 = (unsigned long long)m + 1;
        const unsigned nsb64 = (unsigned)((e64 + S64_TILE - 1) / S64_TILE);
        HX_TRY(scan64.alloc(sizeof(unsigned long long) * ((size_t)nsb64 + 16)));
        std::vector<double> mom_host, ax_level;
        std::vector<unsigned> count_host, newid;
        while (std::any_of(segs.begin(), segs.end(), [](const Segment &s) { return s.n >= 2; })) {
            const unsigned nseg = (unsigned)segs.size();
            unsigned nchunks = 0;
            HX_TRY(upload_segments(tb, segs, true, st, &nchunks));
            {   // moments of the segments that split, their axes on the host
                ProfScope prof("jk_moments");
                hipLaunchKernelGGL(k_jk_partials<0>, dim3(nchunks), dim3(JK_BLOCK), 0, st, (long long)nside, nseg, tb.start(), tb.choff(), order,
                                   pix.as<unsigned>(), q.as<unsigned long long>(), (const double *)nullptr, partial.as<double>());
                hipLaunchKernelGGL(k_jk_final<hxjk::NMOM>, dim3(nseg), dim3(JK_BLOCK), 0, st, tb.choff(), partial.as<double>(), moments.as<double>());
            }
            HX_HIP(hipGetLastError());
            mom_host.resize((size_t)hxjk::NMOM * nseg);
            HX_HIP(hipMemcpyAsync(mom_host.data(), moments.p, sizeof(double) * mom_host.size(), hipMemcpyDeviceToHost, st));
            HX_HIP(hipStreamSynchronize(st));
            ax_level.assign((size_t)3 * nseg, 0.0);
            for (unsigned s = 0; s < nseg; ++s) {
                if (segs[s].n < 2) continue;
                double C[6];
                hxjk::covariance(&mom_host[(size_t)hxjk::NMOM * s], C);
                hxjk::principal_axis(C, &ax_level[3 * (size_t)s]);
                const unsigned b = segs[s].first + segs[s].n / 2;  // the first label of the right part: 2 .. njk, each once
                std::memcpy(&axes_host[3 * (size_t)(b - 2)], &ax_level[3 * (size_t)s], 3 * sizeof(double));
            }
            HX_HIP(hipMemcpyAsync(daxes.p, ax_level.data(), sizeof(double) * ax_level.size(), hipMemcpyHostToDevice, st));
            unsigned long long *ks = nullptr;
            unsigned *vs = nullptr;
            {   // order every segment by its projection: 8 passes over the 64-bit keys, then the passes of the segment id
                ProfScope prof("jk_sort");
                hipLaunchKernelGGL(k_jk_keys, dim3(blocks_for(m)), dim3(JK_BLOCK), 0, st, m, (long long)nside, pix.as<unsigned>(), segid.as<unsigned>(), tb.n(),
                                   daxes.as<double>(), keyA.as<unsigned long long>(), valA.as<unsigned>());
                HX_TRY(rsort::radix_sort_pairs<unsigned long long>(keyA.as<unsigned long long>(), valA.as<unsigned>(), keyB.as<unsigned long long>(),
                                                                   valB.as<unsigned>(), m, 64, sort_tmp, st, &ks, &vs));
            }
            // the keys are spent: one key buffer holds the segment ids of the second sort (two arrays of m), the other the scan
            unsigned long long *E = ks;
            unsigned *seg0 = (unsigned *)(ks == keyA.as<unsigned long long>() ? keyB.p : keyA.p), *seg1 = seg0 + m;
            unsigned *vfree = vs == valA.as<unsigned>() ? valB.as<unsigned>() : valA.as<unsigned>();
            unsigned *segs_sorted = seg0;
            {
                ProfScope prof("jk_sort");
                hipLaunchKernelGGL(k_jk_gather, dim3(blocks_for((unsigned long long)m + 1)), dim3(JK_BLOCK), 0, st, m, vs, segid.as<unsigned>(),
                                   (const unsigned long long *)nullptr, seg0, (unsigned long long *)nullptr);
                int bits = 0;
                while ((1u << bits) < nseg) ++bits;
                HX_TRY(rsort::radix_sort_pairs<unsigned>(seg0, vs, seg1, vfree, m, bits, sort_tmp, st, &segs_sorted, &vs));
            }
            {   // integer weights in that order, their exclusive scan, the targets, the counts
                ProfScope prof("jk_split");
                hipLaunchKernelGGL(k_jk_gather, dim3(blocks_for((unsigned long long)m + 1)), dim3(JK_BLOCK), 0, st, m, vs, segid.as<unsigned>(),
                                   q.as<unsigned long long>(), (unsigned *)nullptr, E);
                hipLaunchKernelGGL(k_scan64_sums, dim3(nsb64), dim3(S64_T), 0, st, E, e64, scan64.as<unsigned long long>());
                hipLaunchKernelGGL(k_scan64_top, dim3(1), dim3(1024), 0, st, scan64.as<unsigned long long>(), nsb64);
                hipLaunchKernelGGL(k_scan64_apply, dim3(nsb64), dim3(S64_T), 0, st, E, e64, scan64.as<unsigned long long>());
                hipLaunchKernelGGL(k_jk_targets, dim3(blocks_for(nseg)), dim3(JK_BLOCK), 0, st, nseg, tb.start(), tb.n(), E, targets.as<unsigned long long>());
                HX_HIP(hipMemsetAsync(tb.count(), 0, sizeof(unsigned) * nseg, st));
                hipLaunchKernelGGL(k_jk_count, dim3(blocks_for(m)), dim3(JK_BLOCK), 0, st, m, segs_sorted, tb.start(), tb.n(), E, targets.as<unsigned long long>(),
                                   tb.count());
            }
            HX_HIP(hipGetLastError());
            count_host.resize(nseg);
            HX_HIP(hipMemcpyAsync(count_host.data(), tb.count(), sizeof(unsigned) * nseg, hipMemcpyDeviceToHost, st));
            HX_HIP(hipStreamSynchronize(st));
            // clamp, number the children
            std::vector<Segment> next;
            next.reserve((size_t)2 * nseg);
            newid.resize(nseg);
            for (unsigned s = 0; s < nseg; ++s) {
                const Segment &g = segs[s];
                newid[s] = (unsigned)next.size();
                if (g.n < 2) {
                    count_host[s] = 0;
                    next.push_back(g);
                    continue;
                }
                const unsigned n1 = g.n / 2, c = hxjk::clamp_count(count_host[s], g.m, n1, g.n);
                count_host[s] = c;
                next.push_back(Segment{g.first, n1, g.start, c});
                next.push_back(Segment{g.first + n1, g.n - n1, g.start + c, g.m - c});
            }
            HX_HIP(hipMemcpyAsync(tb.count(), count_host.data(), sizeof(unsigned) * nseg, hipMemcpyHostToDevice, st));
            HX_HIP(hipMemcpyAsync(tb.newid(), newid.data(), sizeof(unsigned) * nseg, hipMemcpyHostToDevice, st));
            {
                ProfScope prof("jk_split");
                hipLaunchKernelGGL(k_jk_relabel, dim3(blocks_for(m)), dim3(JK_BLOCK), 0, st, m, vs, segs_sorted, tb.start(), tb.n(), tb.count(), tb.newid(),
                                   segid.as<unsigned>());
            }
            HX_HIP(hipGetLastError());
            HX_HIP(hipStreamSynchronize(st));  // (count_host / newid are rewritten by the next level)
            segs.swap(next);
            order = vs;
        }
    }

    // ---- labels, and the diagnostics ----
    unsigned nchunks = 0;
    HX_TRY(upload_segments(tb, segs, false, st, &nchunks));
    OutView vlab, vrw;
    HX_TRY(vlab.bind(labels, sizeof(int32_t) * (size_t)npix));
    {
        ProfScope prof("jk_labels");
        HX_HIP(hipMemsetAsync(vlab.dev, 0, sizeof(int32_t) * (size_t)npix, st));
        hipLaunchKernelGGL(k_jk_labels, dim3(blocks_for(m)), dim3(JK_BLOCK), 0, st, m, npix, pix.as<unsigned>(), segid.as<unsigned>(), tb.first(),
                           vlab.as<int32_t>());
    }
    HX_HIP(hipGetLastError());
    if (region_weight) {
        // after the last level every segment is one region, in label order
        HX_TRY(vrw.bind(region_weight, sizeof(double) * (size_t)njk));
        ProfScope prof("jk_labels");
        hipLaunchKernelGGL(k_jk_partials<1>, dim3(nchunks), dim3(JK_BLOCK), 0, st, (long long)nside, (unsigned)segs.size(), tb.start(), tb.choff(), order,
                           pix.as<unsigned>(), (const unsigned long long *)nullptr, vw.as<double>(), partial.as<double>());
        hipLaunchKernelGGL(k_jk_final<1>, dim3((unsigned)segs.size()), dim3(JK_BLOCK), 0, st, tb.choff(), partial.as<double>(), vrw.as<double>());
        HX_HIP(hipGetLastError());
        HX_TRY(vrw.finish());
    }
    HX_TRY(vlab.finish());
    if (axes && njk > 1) {
        if (is_device_ptr(axes)) HX_HIP(hipMemcpyAsync(axes, axes_host.data(), sizeof(double) * axes_host.size(), hipMemcpyHostToDevice, st));
        else std::memcpy(axes, axes_host.data(), sizeof(double) * axes_host.size());
    }
    HX_HIP(hipStreamSynchronize(st));  // (the buffers are freed on return)
    return HX_OK;
}
