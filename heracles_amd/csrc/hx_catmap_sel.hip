// hx_catmap_sel.hip -- the hx_catmap_sel context: the views of one base catalogue (heracles/catalog/base.py:204-310) mapped in one pass
// over the base's pages (hx_catalog.h states the shared core).
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
#include "hx_catalog.h"
#include "hx_sort.h"

namespace hx {
namespace {

using namespace cat;

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

}  // namespace
}  // namespace hx

using namespace hx;
using namespace hx::cat;

struct hx_catmap_sel : CatBase {
    SelArgs args{};
    DevBuf mrows[kCatF];  // per field: for each of its rows, the nsel map-row pointers
    DevBuf pix[kCatG], mem, cnt, scan_sums, key, ord;
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
            ok = d[0] == HX_CAT_FILTER_FOOTPRINT && col_ok(d[1], ncols, true) && col_ok(d[2], ncols, true) && d[3] >= 1 &&
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
    HX_TRY(cat_sums_init(c, &a.slab, &a.nan, &a.nbad));
    a.fcount = a.nbad + c->n_bad();
    a.extra = a.fcount + c->n_fcount();
    return HX_OK;
}

extern "C" hx_catmap_sel *hx_catmap_create_sel(int64_t page_size, int ncols, int nfields, const int *desc, int nsel, int npred,
                                               const int *preds, const double *pval, int nfilt, const int *filters,
                                               const double *const *footprints, double *const *maps)
{
    return cat_create<hx_catmap_sel>([&](hx_catmap_sel *c) {
        return catmap_sel_init(c, page_size, ncols, nfields, desc, nsel, npred, preds, pval, nfilt, filters, footprints, maps);
    });
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
    const unsigned nblocks = prepare_blocks(n);
    unsigned long long extra = 0;
    {
        ProfScope ps("catmap_prepare");
        const size_t lds = sizeof(double) * 4 * c->nsel * c->nfield * 4;
        HX_HIP(hipMemsetAsync(a.extra, 0, sizeof(unsigned long long), st));
        HX_TRY(cat_prepare(c, nblocks, [&](auto nf) {
            hipLaunchKernelGGL(k_sel_prepare<decltype(nf)::value>, dim3(nblocks), dim3(256), lds, st, (long long)n, a);
        }));
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
    for (int g = 0; g < c->ngroup; ++g) {
        const long long npix = 12ll * a.c.gnside[g] * a.c.gnside[g], npix1 = npix + 1;
        rsort::SortedPairs sp;
        {
            ProfScope ps("catmap_sort");
            hipLaunchKernelGGL(k_sel_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n, c->mem.as<unsigned>(), off,
                               c->pix[g].as<unsigned>(), npix1, c->nsel, c->key.as<long long>(), c->ord.as<unsigned>());
            HX_HIP(hipGetLastError());
            // the largest key: nsel (npix + 1), that of the rows in no selection
            HX_TRY(rsort::sort_pairs_by_key(c->key.as<long long>(), c->ord.as<unsigned>(), nkeys,
                                            (unsigned long long)c->nsel * (unsigned long long)npix1, false, c->k2, c->v1, c->sort_tmp, st, &sp));
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
                    if (sp.k32)
                        hipLaunchKernelGGL(k_sel_run_add<unsigned>, dim3(blocks), dim3(256), 0, st, (long long)nkeys, sp.k32, sp.idx, npix1,
                                           c->nsel, vrow, mrows);
                    else
                        hipLaunchKernelGGL(k_sel_run_add<long long>, dim3(blocks), dim3(256), 0, st, (long long)nkeys, sp.k64, sp.idx, npix1,
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
    return cat_moments(c, "hx_catmap_moments_sel", out, bad, true, fcount);
}

extern "C" int hx_catmap_finish_sel(hx_catmap_sel *c, int sel, int field, double norm, const double *vis)
{
    return cat_finish(c, "hx_catmap_finish_sel", sel, field, norm, vis);
}
