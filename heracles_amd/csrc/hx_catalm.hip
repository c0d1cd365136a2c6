// hx_catalm.hip -- catalogues -> alms through the point transform (heracles.map_catalogs with a DiscreteMapper: heracles/fields.py:197-559
// over heracles/ducc.py:92-133)
//
// The third context on the shared core (hx_catalog.h): the field rules, the moments and the page protocol are those of hx_catmap; what a
// page adds to is not a map but the oversampled (theta, phi) grid of the point transform (hx_nufft.hip), one per component, owned by the
// context and resident from the first page to hx_catalm_finish.  Spreading is additive in the points, so the grid after the last page is
// the grid of the whole catalogue, and the FFT stages and the Legendre analysis run once per field instead of once per page.  Per page and
// (lmax, lon, lat) group: at most one tile sort, shared by every component of the group, then one spread per component.
// The spread adds with hardware float64 atomics: alms are NOT bit-repeatable between runs (unlike the maps of hx_catmap); the moments are.
#include "hx_catalog.h"

namespace hx {
namespace {

using namespace cat;

// the same page, prepared for the point transform (no pixels, no sort key)
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

}  // namespace
}  // namespace hx

using namespace hx;
using namespace hx::cat;

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
    return cat_sums_init(c, &a.slab, &a.nan, &a.nbad);
}

extern "C" hx_catalm *hx_catalm_create(int64_t page_size, int ncols, int nfields, const int *desc, hx_pointsht *const *ps)
{
    return cat_create<hx_catalm>([&](hx_catalm *c) { return catalm_init(c, page_size, ncols, nfields, desc, ps); });
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
    const unsigned nblocks = prepare_blocks(n);
    {
        ProfScope ps("catalm_prepare");
        HX_TRY(cat_prepare(c, nblocks, [&](auto nf) {
            hipLaunchKernelGGL(k_catalm_prepare<decltype(nf)::value>, dim3(nblocks), dim3(256), 0, st, (long long)n, a);
        }));
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
        HX_TRY(cat_scale(2 * nlm, nrow, va.as<double>(), norm, vv.as<double>()));
    }
    HX_TRY(va.finish());
    HX_HIP(hipStreamSynchronize(rt().stream));  // (a staged visibility dies with this scope)
    return HX_OK;
}
