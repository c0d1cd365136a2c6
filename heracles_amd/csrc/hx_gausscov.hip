// hx_gausscov.hip -- mask-aware Gaussian covariance of pseudo-Cl under the narrow-kernel approximation: one coupling
// table Xi_{ll'} = g00[l][l'] / (2l' + 1) and a list of spectra into blocks of the (binned) covariance,
//   cov[(row + b) ldc + col + b'] += sum_{l in b, l' in b'} w_l w_l' Xi_{ll'} (Sbar^{s0} Sbar^{s1} + Sbar^{s2} Sbar^{s3}) / (norm_b norm_b'),
//   Sbar_{ll'} = (S_l + S_l') / 2.  gfx950 only.
//
// Binned, two stages ((S_l + S_l')(T_l + T_l') is four bilinear forms in Xi w):
//   k_gc_coef    coef[u][l] = w_l S^u_l for the spectra the items name (slot 0: the all-ones spectrum).
//   k_gc_fold    stage A, once per call: Z[u][b'][l] = sum_{l' in b'} w_l' Xi_{ll'} S^u_l'.  A work-group owns 64 multipoles l, one bin
//                b' and 32 slots u; it walks the members l' of the bin in chunks of 64: rows l' of the table (lines contiguous in l;
//                Xi_{ll'} is read as Xi_{l'l}) and the coefficients of the chunk go through LDS, a wave keeps 8 slots in registers.
//                The table is read once per 32 slots.  A thread owns an element of Z and adds the members in ascending order.
//   k_gc_blocks  stage B: a wave owns one output element (b, b') of one item.  Per term (S, T)
//                  sum_{l in b} [ w_l S_l T_l Z^1[b'][l] + w_l S_l Z^T[b'][l] + w_l T_l Z^S[b'][l] ] + sum_{l' in b'} w_l' S_l' T_l' Z^1[b][l']
//                (the last sum is the column term: Z^1[b][l'] = sum_{l in b} w_l Xi_{ll'} by the table's symmetry); the lanes stride
//                over the members, the 64 partial sums are added by a fixed xor tree, lane 0 adds a quarter of it over the norms to cov.
// Unbinned (nbins = 0: every l its own bin, weight 1) the output has as many elements as the direct sum has terms, so
//   k_gc_direct  forms every element from its own table entry; no Z.
// No floating-point atomics; every element is owned by one thread or wave and summed in an order that depends on the bins alone, so a
// block has the same bits in every run and whatever other items share the call.  Blocks of one call must not overlap (checked).
#include <algorithm>
#include <climits>
#include <cmath>
#include <unordered_map>

#include "hx_common.h"

namespace hx {
namespace {

constexpr int GC_T = 64;            // multipoles per tile (the lanes of a wave) and members per LDS chunk
constexpr int GC_W = 4;             // waves per work-group
constexpr int GC_U = 8;             // rows of Z a wave accumulates
constexpr int GC_S = GC_W * GC_U;   // slots per work-group of stage A

struct GcItem {
    long long row, col;
    int s[4];  // spectra (s[2] < 0: one term)
    int z[4];  // their slots in coef / Z
};

struct GcScratch {
    DevBuf z, coef;
};
GcScratch *g_gc = nullptr;
unsigned long long g_gc_flops = 0;  // counted on the host from the launch shapes

__global__ __launch_bounds__(256) void k_gc_coef(int n, int nz, const int *__restrict__ ulist, const double *__restrict__ w,
                                                 const double *__restrict__ spec, double *__restrict__ coef)
{
    const int l = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
    if (l >= n || u >= nz) return;
    coef[(size_t)u * n + l] = u == 0 ? w[l] : w[l] * spec[(size_t)ulist[u] * n + l];
}

__global__ __launch_bounds__(GC_T *GC_W) void k_gc_fold(int n, int nb, int nz, const double *__restrict__ g00, const double *__restrict__ coef,
                                                         const int *__restrict__ bstart, const int *__restrict__ mem, double *__restrict__ Z)
{
    __shared__ double xt[GC_T][GC_T];      // [member of the chunk][l of the tile]
    __shared__ double ct[GC_S][GC_T + 1];  // [slot of the group][member of the chunk]
    const int lane = threadIdx.x & (GC_T - 1), wv = threadIdx.x / GC_T;
    const int l = blockIdx.x * GC_T + lane, bp = blockIdx.y, u0 = blockIdx.z * GC_S;
    const int m0 = bstart[bp], m1 = bstart[bp + 1];
    double acc[GC_U];
#pragma unroll
    for (int k = 0; k < GC_U; ++k) acc[k] = 0.0;
    for (int mc = m0; mc < m1; mc += GC_T) {
        const int cnt = min(GC_T, m1 - mc);
        __syncthreads();  // (the tiles are free)
        for (int i = wv; i < cnt; i += GC_W) xt[i][lane] = l < n ? g00[(size_t)mem[mc + i] * n + l] : 0.0;
        for (int k = wv; k < GC_S; k += GC_W) ct[k][lane] = (u0 + k < nz && lane < cnt) ? coef[(size_t)(u0 + k) * n + mem[mc + lane]] : 0.0;
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
            const double g = xt[i][lane];
#pragma unroll
            for (int k = 0; k < GC_U; ++k) acc[k] = fma(ct[wv * GC_U + k][i], g, acc[k]);
        }
    }
    if (l < n) {
        const double d = (double)(2 * l + 1);
#pragma unroll
        for (int k = 0; k < GC_U; ++k) {
            const int u = u0 + wv * GC_U + k;
            if (u < nz) Z[((size_t)u * nb + bp) * n + l] = acc[k] / d;
        }
    }
}

__global__ __launch_bounds__(GC_T *GC_W) void k_gc_blocks(int n, int nb, const GcItem *__restrict__ items, const double *__restrict__ spec,
                                                           const double *__restrict__ coef, const double *__restrict__ Z,
                                                           const int *__restrict__ bstart, const int *__restrict__ mem,
                                                           const double *__restrict__ inorm, double *cov, long long ldc)
{
    const int lane = threadIdx.x & (GC_T - 1), wv = threadIdx.x / GC_T;
    const GcItem &it = items[blockIdx.x / (unsigned)nb];  // (read in place: a private copy indexed by the term would go to LDS)
    const int b = (int)(blockIdx.x % (unsigned)nb);
    const int r0 = bstart[b], r1 = bstart[b + 1];
    if (r0 == r1) return;  // an empty bin adds nothing
    const int nterm = it.s[2] >= 0 ? 2 : 1;
    const double *Z1b = Z + (size_t)b * n;  // slot 0, bin b
    for (int bp = wv; bp < nb; bp += GC_W) {
        const int c0 = bstart[bp], c1 = bstart[bp + 1];
        if (c0 == c1) continue;
        const double *Z1p = Z + (size_t)bp * n;
        double acc = 0.0;
        for (int t = 0; t < nterm; ++t) {
            const double *Sb = spec + (size_t)it.s[2 * t + 1] * n;
            const double *Ca = coef + (size_t)it.z[2 * t] * n, *Cb = coef + (size_t)it.z[2 * t + 1] * n;
            const double *Za = Z + ((size_t)it.z[2 * t] * nb + bp) * n, *Zb = Z + ((size_t)it.z[2 * t + 1] * nb + bp) * n;
            for (int p = r0 + lane; p < r1; p += GC_T) {
                const int l = mem[p];
                const double ca = Ca[l];
                acc = fma(ca * Sb[l], Z1p[l], acc);
                acc = fma(ca, Zb[l], acc);
                acc = fma(Cb[l], Za[l], acc);
            }
            for (int p = c0 + lane; p < c1; p += GC_T) {
                const int l = mem[p];
                acc = fma(Ca[l] * Sb[l], Z1b[l], acc);
            }
        }
        for (int s = GC_T / 2; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
        if (lane == 0) {
            double *o = cov + (it.row + b) * ldc + it.col + bp;
            *o += 0.25 * acc * inorm[b] * inorm[bp];
        }
    }
}

__global__ __launch_bounds__(256) void k_gc_direct(int n, const GcItem *__restrict__ items, const double *__restrict__ g00,
                                                   const double *__restrict__ spec, double *cov, long long ldc)
{
    const int lp = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    if (lp >= n) return;
    const GcItem it = items[blockIdx.z];
    const double xi = g00[(size_t)l * n + lp] / (double)(2 * lp + 1);
    const double *Sa = spec + (size_t)it.s[0] * n, *Sb = spec + (size_t)it.s[1] * n;
    double v = (0.5 * (Sa[l] + Sa[lp])) * (0.5 * (Sb[l] + Sb[lp]));
    if (it.s[2] >= 0) {
        const double *Sc = spec + (size_t)it.s[2] * n, *Sd = spec + (size_t)it.s[3] * n;
        v = fma(0.5 * (Sc[l] + Sc[lp]), 0.5 * (Sd[l] + Sd[lp]), v);
    }
    double *o = cov + (it.row + l) * ldc + it.col + lp;
    *o += xi * v;
}

// true if two of the nbe x nbe blocks overlap: blocks are hashed by the cell (row / nbe, col / nbe) of their corner, an overlapping
// partner lies in one of the nine cells around it
bool blocks_overlap(int64_t nitem, const hx_cov_item *items, int64_t nbe, int64_t *first, int64_t *second)
{
    struct H {
        size_t operator()(const std::pair<int64_t, int64_t> &k) const { return std::hash<int64_t>()(k.first * 0x9E3779B97F4A7C15LL ^ k.second); }
    };
    std::unordered_multimap<std::pair<int64_t, int64_t>, int64_t, H> cells;
    cells.reserve((size_t)nitem);
    for (int64_t i = 0; i < nitem; ++i) {
        const int64_t cr = items[i].row / nbe, cc = items[i].col / nbe;
        for (int64_t dr = -1; dr <= 1; ++dr)
            for (int64_t dc = -1; dc <= 1; ++dc) {
                auto range = cells.equal_range({cr + dr, cc + dc});
                for (auto q = range.first; q != range.second; ++q) {
                    const hx_cov_item &o = items[q->second];
                    if (std::llabs(o.row - items[i].row) < nbe && std::llabs(o.col - items[i].col) < nbe) {
                        *first = q->second;
                        *second = i;
                        return true;
                    }
                }
            }
        cells.insert({{cr, cc}, i});
    }
    return false;
}

}  // namespace

void gausscov_drop_cache()
{
    if (!g_gc) return;
    g_gc->z.release();
    g_gc->coef.release();
}

int gausscov_exec_flops(unsigned long long *v, bool reset)
{
    *v = g_gc_flops;
    if (reset) g_gc_flops = 0;
    return HX_OK;
}

}  // namespace hx

using namespace hx;

extern "C" int hx_gauss_cov_accumulate(int lmax, const double *g00, int nspec, const double *spec, int nbins, const int *which,
                                       const double *w, const double *norm, int64_t nitem, const hx_cov_item *items, double *cov, int64_t ldc)
{
    HX_TRY(ensure_ready());
    // ---- arguments: everything is checked before anything is written ----
    if (lmax < 0 || lmax >= 65535) return fail(HX_ERR_ARG, "hx_gauss_cov_accumulate: lmax = %d (0 .. 65534)", lmax);
    if (nspec < 1 || nbins < 0 || nitem < 0 || ldc < 1)
        return fail(HX_ERR_ARG, "hx_gauss_cov_accumulate: nspec = %d, nbins = %d, nitem = %lld, ldc = %lld", nspec, nbins, (long long)nitem, (long long)ldc);
    if (!g00 || !spec || !cov || (nitem > 0 && !items) || (nbins > 0 && (!which || !w || !norm)))
        return fail(HX_ERR_ARG, "hx_gauss_cov_accumulate: null pointer");
    if (!is_device_ptr(cov)) return fail(HX_ERR_ARG, "hx_gauss_cov_accumulate: cov must be device memory (the call adds into it)");
    const int n = lmax + 1;
    const int64_t nbe = nbins > 0 ? nbins : n;  // edge of a block
    for (int64_t i = 0; i < nitem; ++i) {
        const hx_cov_item &it = items[i];
        const int ns = it.s[2] < 0 ? 2 : 4;
        for (int k = 0; k < ns; ++k)
            if (it.s[k] < 0 || it.s[k] >= nspec)
                return fail(HX_ERR_ARG, "hx_gauss_cov_accumulate: item %lld names spectrum %d, there are %d", (long long)i, it.s[k], nspec);
        if (it.row < 0 || it.col < 0 || it.col > ldc - nbe)
            return fail(HX_ERR_ARG, "hx_gauss_cov_accumulate: block %lld at (%lld, %lld) of edge %lld leaves ldc = %lld", (long long)i,
                        (long long)it.row, (long long)it.col, (long long)nbe, (long long)ldc);
    }
    {
        int64_t a = 0, b = 0;
        if (blocks_overlap(nitem, items, nbe, &a, &b))
            return fail(HX_ERR_ARG, "hx_gauss_cov_accumulate: the blocks of items %lld and %lld overlap (one call owns each element once: use two calls)",
                        (long long)a, (long long)b);
    }
    // bins as member lists (ascending l within a bin: the order of every sum), 1 / norm
    std::vector<int> bstart, mem;
    std::vector<double> inorm;
    int nonempty = 0;
    if (nbins > 0) {
        bstart.assign((size_t)nbins + 1, 0);
        for (int l = 0; l < n; ++l) {
            if (which[l] < -1 || which[l] >= nbins) return fail(HX_ERR_ARG, "hx_gauss_cov_accumulate: which[%d] = %d with %d bins", l, which[l], nbins);
            if (which[l] >= 0) {
                if (!std::isfinite(w[l])) return fail(HX_ERR_ARG, "hx_gauss_cov_accumulate: w[%d] is not finite", l);
                ++bstart[(size_t)which[l] + 1];
            }
        }
        inorm.assign((size_t)nbins, 0.0);
        for (int b = 0; b < nbins; ++b) {
            if (bstart[(size_t)b + 1] > 0) {
                if (!(std::isfinite(norm[b]) && norm[b] != 0.0)) return fail(HX_ERR_ARG, "hx_gauss_cov_accumulate: norm[%d] = %g of a bin with members", b, norm[b]);
                inorm[b] = 1.0 / norm[b];
                ++nonempty;
            }
            bstart[(size_t)b + 1] += bstart[b];
        }
        mem.assign((size_t)std::max(bstart[nbins], 1), 0);
        std::vector<int> at(bstart.begin(), bstart.end() - 1);
        for (int l = 0; l < n; ++l)
            if (which[l] >= 0) mem[(size_t)at[which[l]]++] = l;
    }
    // the spectra the items name -> slots of coef / Z (slot 0: ones), in order of first use
    std::vector<int> slot((size_t)nspec, -1), ulist(1, 0);
    std::vector<GcItem> gi((size_t)std::max<int64_t>(nitem, 1));
    for (int64_t i = 0; i < nitem; ++i) {
        GcItem &g = gi[(size_t)i];
        g.row = items[i].row;
        g.col = items[i].col;
        for (int k = 0; k < 4; ++k) {
            const int s = (k >= 2 && items[i].s[2] < 0) ? -1 : items[i].s[k];
            g.s[k] = s;
            g.z[k] = 0;
            if (s >= 0 && nbins > 0) {
                if (slot[s] < 0) {
                    slot[s] = (int)ulist.size();
                    ulist.push_back(s);
                }
                g.z[k] = slot[s];
            }
        }
    }
    const int nz = (int)ulist.size();
    if (!g_gc) g_gc = new GcScratch;
    const size_t zbytes = sizeof(double) * (size_t)nz * (size_t)nbe * n, cbytes = sizeof(double) * (size_t)nz * n;
    if (nbins > 0 && nitem > 0 && g_gc->z.bytes < zbytes) {
        // the guard of the dense matrices (covariance._check_dense): the scratch must fit in 0.9 of what is free (its old copy goes first)
        size_t free_b = 0, total_b = 0;
        HX_HIP(hipMemGetInfo(&free_b, &total_b));
        if ((double)zbytes > 0.9 * ((double)free_b + (double)g_gc->z.bytes))
            return fail(HX_ERR_MEM, "hx_gauss_cov_accumulate: %d spectra x %d bins x %d multipoles need %.1f GiB of scratch, %.1f GiB are free; "
                        "split the item list by spectra", nz, nbins, n, zbytes / 1073741824.0, free_b / 1073741824.0);
    }
    if (nitem == 0) return HX_OK;

    InView vg, vs;
    HX_TRY(vg.bind(g00, sizeof(double) * (size_t)n * n));
    HX_TRY(vs.bind(spec, sizeof(double) * (size_t)nspec * n));
    DevBuf b_items, b_bstart, b_mem, b_inorm, b_w, b_ulist;
    HX_TRY(upload_vec(b_items, gi));
    hipStream_t st = rt().stream;
    ProfScope prof("gauss_cov");
    if (nbins == 0) {
        const unsigned gx = (unsigned)((n + 255) / 256);
        for (int64_t i0 = 0; i0 < nitem; i0 += 65535) {
            const unsigned cnt = (unsigned)std::min<int64_t>(65535, nitem - i0);
            hipLaunchKernelGGL(k_gc_direct, dim3(gx, (unsigned)n, cnt), dim3(256), 0, st, n, b_items.as<GcItem>() + i0, vg.as<double>(), vs.as<double>(),
                               cov, (long long)ldc);
        }
        for (int64_t i = 0; i < nitem; ++i) g_gc_flops += (unsigned long long)(items[i].s[2] < 0 ? 9 : 15) * n * n;
    } else {
        HX_TRY(upload_vec(b_bstart, bstart));
        HX_TRY(upload_vec(b_mem, mem));
        HX_TRY(upload_vec(b_inorm, inorm));
        HX_TRY(upload_vec(b_ulist, ulist));
        HX_TRY(upload_vec(b_w, std::vector<double>(w, w + n)));
        if (g_gc->z.bytes < zbytes) g_gc->z.release();  // (not both copies at once)
        HX_TRY(g_gc->z.alloc(zbytes));
        HX_TRY(g_gc->coef.alloc(cbytes));
        double *Z = g_gc->z.as<double>(), *coef = g_gc->coef.as<double>();
        hipLaunchKernelGGL(k_gc_coef, dim3((unsigned)((n + 255) / 256), (unsigned)nz), dim3(256), 0, st, n, nz, b_ulist.as<int>(), b_w.as<double>(),
                           vs.as<double>(), coef);
        hipLaunchKernelGGL(k_gc_fold, dim3((unsigned)((n + GC_T - 1) / GC_T), (unsigned)nbins, (unsigned)((nz + GC_S - 1) / GC_S)), dim3(GC_T * GC_W), 0, st,
                           n, nbins, nz, vg.as<double>(), coef, b_bstart.as<int>(), b_mem.as<int>(), Z);
        const int64_t per = std::max<int64_t>(1, (int64_t)INT_MAX / nbins);  // items per launch: the grid's first extent is 31 bits
        for (int64_t i0 = 0; i0 < nitem; i0 += per) {
            const int64_t cnt = std::min<int64_t>(per, nitem - i0);
            hipLaunchKernelGGL(k_gc_blocks, dim3((unsigned)(cnt * nbins)), dim3(GC_T * GC_W), 0, st, n, nbins, b_items.as<GcItem>() + i0, vs.as<double>(),
                               coef, Z, b_bstart.as<int>(), b_mem.as<int>(), b_inorm.as<double>(), cov, (long long)ldc);
        }
        const unsigned long long members = (unsigned long long)bstart[nbins];
        g_gc_flops += 2ull * nz * members * n + (unsigned long long)nz * nbins * n;
        for (int64_t i = 0; i < nitem; ++i)
            g_gc_flops += (items[i].s[2] < 0 ? 1ull : 2ull) * 10ull * members * nonempty + 67ull * nonempty * nonempty;
    }
    HX_HIP(hipGetLastError());
    return finish_call();
}
