// hx_catalog.h -- what the three catalogue contexts share: the core their prepare kernels inline (device part) and the context base,
// the page protocol and the readout they call (host part, defined once in hx_catalog.hip).
//
// catalogues -> field maps (heracles.map_catalogs, heracles/fields.py:197-559): one pass over each page for every field of a catalogue
//
// Three contexts share one core.  hx_catmap (hx_catmap.hip) maps one catalogue; hx_catmap_sel (hx_catmap_sel.hip) maps the views of one
// base catalogue (heracles/catalog/base.py:204-310) in one pass over the base's pages; hx_catalm (hx_catalm.hip) spreads the same value
// rows onto the grids of the point transform.  The rules of the reference's fields are stated once, in
// field_step (keep rule, value rows w v with every product rounded on its own, as numpy's `v * w`; 0 on a dropped row, which adds
// nothing to a sum that starts at +0; the moment contributions {1, w, w^2, |w v|^2}; which columns count their NaNs) and group_step
// (the pixel of a row in an (nside, lon, lat) group; the sentinel npix for rows no field of the group keeps and for invalid positions,
// which are counted).  Moments are summed per block into a slab and over blocks in a fixed order (k_cat_reduce); no float atomics.
//
// Counters, one layout for every context (CatBase::counters): nan [nsel][nfield][5], then nbad [nsel][ngroup], then
// fcount [nsel][nfilt + 1], then extra; nsel = 1 and nfilt = 0 for hx_catmap and hx_catalm.  The kernels see only the pointers.
#pragma once
#include <algorithm>
#include <type_traits>

#include "hx_common.h"

#include "hx_ang2pix.h"

namespace hx {
namespace cat {

constexpr int kCatF = HX_CAT_MAX_FIELDS, kCatG = HX_CAT_MAX_GROUPS, kCatC = HX_CAT_MAX_COLUMNS;
constexpr int kSelS = HX_CAT_MAX_SELECTIONS, kSelP = HX_CAT_MAX_PREDICATES, kSelFl = HX_CAT_MAX_FILTERS;
constexpr int kCatBlocks = 2048;  // most blocks of a prepare kernel: rows per thread grow beyond 2048 x 256 rows

// what every prepare kernel reads about the page, the fields and their (nside, lon, lat) groups (the scalars before the pointers: with the
// pointers first the compiler reserves a scratch slot for the prepare kernels that it never uses)
struct CatCore {
    long long cap;
    int nfield, ngroup;
    int kind[kCatF], grp[kCatF], cv[kCatF], ci[kCatF], cw[kCatF];
    int gnside[kCatG], glon[kCatG], glat[kCatG];
    const double *col[kCatC];
    double *val[kCatF];  // row r of field f at val[f] + r * cap
};

namespace {

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

}  // namespace

// What the contexts hold: the fields, their value rows and maps ([nsel][nfield]; one selection for hx_catmap), the sort's buffers, the
// moments and counters, and the two staging sets of the page protocol.
struct CatBase {
    long long cap = 0;
    int ncols = 0, nfield = 0, ngroup = 0, nsel = 1, nfilt = 0;
    int kind[kCatF] = {}, grp[kCatF] = {}, nside[kCatF] = {}, nrow[kCatF] = {};
    double *map[kSelS * kCatF] = {};
    DevBuf val[kCatF], k2, v1, sort_tmp;
    DevBuf stage[2][kCatC + 1];  // the columns, then the mask words
    DevBuf slab, acc, counters;
    hipEvent_t ev_up[2] = {}, ev_done[2] = {};
    long long page_no = 0;
    size_t n_nan() const { return (size_t)nsel * nfield * 5; }
    size_t n_bad() const { return (size_t)nsel * ngroup; }
    size_t n_fcount() const { return (size_t)nsel * (nfilt + 1); }
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
                    double *const *maps, int res_lo = 1, int res_hi = 16384);

// The zeroed moments ([nsel][nfield][4], and their slab) and counters (c->nsel, nfield, ngroup and nfilt must be set), and the events of
// the page protocol; gives the slab and the first two counter arrays, which every prepare kernel takes
int cat_sums_init(CatBase *c, double **slab, unsigned long long **nan, unsigned long long **nbad);

// The one shape of a create entry point: a context whose init fails is deleted
template <class Ctx, class Init>
Ctx *cat_create(Init init)
{
    if (ensure_ready() != HX_OK) return nullptr;
    Ctx *c = new Ctx;
    if (init(c) != HX_OK) {
        delete c;
        return nullptr;
    }
    return c;
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

int page_open(CatBase *c, const char *who, int64_t n, const double *const *cols, const uint32_t *mask, PageIO *io);
int page_close(CatBase *c, const PageIO &io);

inline unsigned prepare_blocks(int64_t n) { return (unsigned)std::min<long long>((n + 255) / 256, kCatBlocks); }

// acc += the sum over the prepare kernel's blocks of their slab rows, in block order (k_cat_reduce)
int cat_reduce(CatBase *c, unsigned nblocks);

// A page's prepare step: launch(std::integral_constant<int, NF>) starts the context's prepare kernel for its NF = nfield fields (a
// template argument of those kernels, so that only the moments of NF fields occupy registers), then the blocks' moments are added up
template <class Launch>
int cat_prepare(CatBase *c, unsigned nblocks, Launch launch)
{
    switch (c->nfield) {
#define HX_CAT_NF(NF) case NF: launch(std::integral_constant<int, NF>{}); break;
        HX_CAT_NF(1) HX_CAT_NF(2) HX_CAT_NF(3) HX_CAT_NF(4) HX_CAT_NF(5) HX_CAT_NF(6) HX_CAT_NF(7) HX_CAT_NF(8)
#undef HX_CAT_NF
    }
    return cat_reduce(c, nblocks);
}

// Waits for the pages; the moments out [nsel][nfield][4], the counters bad [nsel][nfield][6] (five NaN slots, then the invalid positions
// of the field's group) and, for a context with filters (with_fcount), fcount [nsel][nfilt + 1]
int cat_moments(CatBase *c, const char *who, double *out, int64_t *bad, bool with_fcount = false, int64_t *fcount = nullptr);

// rows <- rows / norm - vis over nrow rows of npix doubles on the library's stream (k_cat_finish; vis may be null)
int cat_scale(long long npix, int nrow, double *rows, double norm, const double *vis);

// map <- map / norm - vis for the map of (sel, field)
int cat_finish(CatBase *c, const char *who, int sel, int field, double norm, const double *vis);

}  // namespace cat
}  // namespace hx
