// hx_catmap.hip -- the hx_catmap context: one catalogue -> the maps of its fields, page by page (hx_catalog.h states the shared core).
//
// k_cat_prepare reads the page's columns once, writes value rows, pixel keys and row indices, and sums the moments in registers.  Each
// group is then stably sorted once (hx_sort.h) and k_cat_run_add adds every map row of its fields in catalogue order, one pass per row,
// stopping at the sentinel.
#include "hx_catalog.h"
#include "hx_sort.h"

namespace hx {
namespace {

using namespace cat;

struct CatArgs {
    CatCore c;
    long long *key[kCatG];
    unsigned *ord[kCatG];
    unsigned long long *nan;   // [nfield][5]
    unsigned long long *nbad;  // [ngroup]
    double *slab;              // [gridDim.x][nfield * 4]
};

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

}  // namespace
}  // namespace hx

using namespace hx;
using namespace hx::cat;

struct hx_catmap : CatBase {
    CatArgs args{};
    DevBuf key[kCatG], ord[kCatG];
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
    HX_TRY(c->k2.alloc(sizeof(long long) * page_size));
    HX_TRY(c->v1.alloc(sizeof(unsigned) * page_size));
    return cat_sums_init(c, &a.slab, &a.nan, &a.nbad);
}

extern "C" hx_catmap *hx_catmap_create(int64_t page_size, int ncols, int nfields, const int *desc, double *const *maps)
{
    return cat_create<hx_catmap>([&](hx_catmap *c) { return catmap_init(c, page_size, ncols, nfields, desc, maps); });
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
    const unsigned nblocks = prepare_blocks(n);
    {
        ProfScope ps("catmap_prepare");
        HX_TRY(cat_prepare(c, nblocks, [&](auto nf) {
            hipLaunchKernelGGL(k_cat_prepare<decltype(nf)::value>, dim3(nblocks), dim3(256), 0, st, (long long)n, a);
        }));
    }
    for (int g = 0; g < c->ngroup; ++g) {
        const long long npix = 12ll * a.c.gnside[g] * a.c.gnside[g];
        rsort::SortedPairs sp;
        {
            ProfScope ps("catmap_sort");
            // the largest key is the sentinel npix, which sorts after every pixel; nside <= 16384 keeps it within 32 bits
            HX_TRY(rsort::sort_pairs_by_key(c->key[g].as<long long>(), c->ord[g].as<unsigned>(), (unsigned long long)n, (unsigned long long)npix,
                                            false, c->k2, c->v1, c->sort_tmp, st, &sp));
        }
        {
            ProfScope ps("catmap_add");
            // one pass per map row: the live set of a pass (one value row, one map) stays small enough for the cache (all rows of the
            // group in one pass: 21 instead of 17 ms per 10^8 rows for four rows at nside 4096)
            for (int f = 0; f < c->nfield; ++f) {
                if (c->grp[f] != g) continue;
                for (int r = 0; r < c->nrow[f]; ++r)
                    hipLaunchKernelGGL(k_cat_run_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n, sp.k32, sp.idx,
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
