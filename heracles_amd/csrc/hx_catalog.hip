// hx_catalog.hip -- the host side the catalogue contexts share (hx_catalog.h): field descriptors and groups, moments and counters, the
// page protocol, the readout, and the two small kernels every context launches.
#include "hx_catalog.h"

namespace hx {
namespace cat {

namespace {

// acc[t] += sum over blocks of slab[b][t], b in order: the moments of the page added to the context's
__global__ __launch_bounds__(256) void k_cat_reduce(int nblocks, int width, const double *__restrict__ slab, double *__restrict__ acc)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= width) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += slab[(long long)b * width + t];
    acc[t] += s;
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

}  // namespace

int cat_fields_init(CatBase *c, CatCore &a, const char *who, int64_t page_size, int ncols, int nfields, const int *desc, int nsel,
                    double *const *maps, int res_lo, int res_hi)
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

int cat_sums_init(CatBase *c, double **slab, unsigned long long **nan, unsigned long long **nbad)
{
    const int width = c->nsel * c->nfield * 4;
    HX_TRY(c->slab.alloc(sizeof(double) * kCatBlocks * width));
    HX_TRY(c->acc.alloc(sizeof(double) * width));
    HX_TRY(c->counters.alloc(sizeof(unsigned long long) * (c->n_nan() + c->n_bad() + c->n_fcount() + 1)));
    hipStream_t st = rt().stream;
    HX_HIP(hipMemsetAsync(c->acc.p, 0, c->acc.bytes, st));
    HX_HIP(hipMemsetAsync(c->counters.p, 0, c->counters.bytes, st));
    for (int s = 0; s < 2; ++s) {
        HX_HIP(hipEventCreateWithFlags(&c->ev_up[s], hipEventDisableTiming));
        HX_HIP(hipEventCreateWithFlags(&c->ev_done[s], hipEventDisableTiming));
        HX_HIP(hipEventRecord(c->ev_done[s], st));
    }
    *slab = c->slab.as<double>();
    *nan = c->counters.as<unsigned long long>();
    *nbad = *nan + c->n_nan();
    return HX_OK;
}

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

int cat_reduce(CatBase *c, unsigned nblocks)
{
    const int width = c->nsel * c->nfield * 4;
    hipLaunchKernelGGL(k_cat_reduce, dim3((width + 255) / 256), dim3(256), 0, rt().stream, (int)nblocks, width, c->slab.as<double>(),
                       c->acc.as<double>());
    HX_HIP(hipGetLastError());
    return HX_OK;
}

int cat_moments(CatBase *c, const char *who, double *out, int64_t *bad, bool with_fcount, int64_t *fcount)
{
    HX_TRY(ensure_ready());
    if (!c || !out || !bad || (with_fcount && !fcount)) return fail(HX_ERR_ARG, "%s: bad arguments", who);
    hipStream_t st = rt().stream;
    const int nf = c->nfield, width = c->nsel * nf * 4;
    std::vector<double> acc(width);
    std::vector<unsigned long long> cnt(c->n_nan() + c->n_bad() + c->n_fcount());
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
        for (int k = 0; with_fcount && k <= c->nfilt; ++k) fcount[(c->nfilt + 1) * s + k] = (int64_t)fc[(c->nfilt + 1) * s + k];
    }
    return HX_OK;
}

int cat_scale(long long npix, int nrow, double *rows, double norm, const double *vis)
{
    const long long total = npix * nrow;
    const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(k_cat_finish, dim3(blocks), dim3(256), 0, rt().stream, npix, nrow, rows, norm, vis);
    HX_HIP(hipGetLastError());
    return HX_OK;
}

int cat_finish(CatBase *c, const char *who, int sel, int field, double norm, const double *vis)
{
    HX_TRY(ensure_ready());
    if (!c || sel < 0 || sel >= c->nsel || field < 0 || field >= c->nfield) return fail(HX_ERR_ARG, "%s: bad arguments", who);
    const long long npix = 12ll * c->nside[field] * c->nside[field];
    InView vv;
    HX_TRY(vv.bind(vis, sizeof(double) * npix));
    {
        ProfScope ps("catmap_finish");
        HX_TRY(cat_scale(npix, c->nrow[field], c->map[sel * c->nfield + field], norm, vv.as<double>()));
    }
    HX_HIP(hipStreamSynchronize(rt().stream));  // (a staged visibility dies with this scope)
    return HX_OK;
}

}  // namespace cat
}  // namespace hx
