// hx_deproject.hip -- template deprojection of maps: the Gram matrix of mask-weighted templates and maps over the
// pixel axis, the streaming removal of the fitted templates, and the per-l product of alms with a block of spectra that the
// deprojection bias needs.  gfx950 only.
//
//   k_dp_gram     X^T X for the columns X = (v t_1 .. v t_k, d_1 .. d_m), inner dimension ncomp npix (2 10^8 at nside 4096).  The
//                 inner axis is cut into slabs; a work-group owns one 64 x 64 output tile (I <= J) and one slab.  Columns are
//                 contiguous along the pixel axis, so operands are staged through LDS: 32 consecutive lanes read 256 contiguous bytes
//                 of one column, the mask is multiplied in on the way, and the MFMA lanes (A[i = lane & 15][k = lane >> 4]) read LDS rows
//                 of stride DK + 2 doubles, which spreads a half-wave's 64-bit reads over all 64 banks.  The next stage's global loads
//                 (the next two on a diagonal tile) are in flight while the matrix unit works on the current one.  Accumulation: v_mfma_f64_16x16x4_f64, 2 x 2 blocks
//                 per wave; blocks past column n and below the diagonal of a diagonal tile are skipped (n = 33: 6 of 16).  The partial
//                 tile goes to library scratch.
//   k_dp_reduce   adds the slabs of a tile in ascending order and writes the element and its mirror image from the same value.
//   k_dp_apply    out[m] = d[m] - v * sum_i alpha[m][i] t_i, one pass: a template element is read once for up to 8 maps (more maps
//                 take another pass), alpha and the pointer table are uniform reads (scalar registers).
//   k_alm_apply_cl  alm_out[x][l, m] = sum_y cl[x][y][l] alm_in[y][l, m].
// No floating-point atomics; the slab partition depends on (ncomp npix, n) alone: results are bit-identical between runs and devices.
// Floating-point contraction is OFF in k_dp_apply (products and sums round separately, in the order the header states).
#include <cmath>
#include <cstdlib>

#include "hx_common.h"

namespace hx {
namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int DT = 64;           // output tile of a work-group
constexpr int DK = 32;           // inner elements per LDS stage
constexpr int DLD = DK + 2;      // LDS row stride in doubles: 4 r + 2 k (mod 64 banks) is distinct over a half-wave
constexpr int DP_MAX_N = 1024;   // columns of one call
constexpr long long DP_MIN_SLAB = 8192;
constexpr int DP_TARGET_GROUPS = 2048;  // work-groups aimed at (a constant: the partition must not depend on the device)
constexpr int DA_MB = 8;         // maps per pass of k_dp_apply

// DIAG: the tile pairs a column block with itself -- one operand, the two halves of LDS hold alternate stages (one barrier per stage)
// and two stages of global loads are in flight; this is the kernel of every call with n <= 64.  Otherwise the halves hold the two
// operands of one stage.  tbase: index of the launch's first tile in `tiles` and `part`.
template <bool DIAG>
__global__ __launch_bounds__(256) void k_dp_gram(long long Q, long long npix, int n, int ntemp, const double *const *__restrict__ cols,
                                                 const double *__restrict__ mask, long long slab, int nslab, const int2 *__restrict__ tiles,
                                                 int tbase, double *__restrict__ part)
{
    __shared__ double sm[2][DT][DLD];
    const int tile = tbase + blockIdx.y;
    const int2 tl = tiles[tile];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int px = t & (DK - 1), cg = t >> 5;  // staging: inner element and column group of this thread
    const long long q0 = (long long)blockIdx.x * slab, q1 = q0 + slab < Q ? q0 + slab : Q;
    constexpr int NB = DIAG ? 1 : 8;

    const double *pa[8], *pb[NB];
    bool ta[8], tb[NB];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int ca = tl.x * DT + u * 8 + cg;
        pa[u] = ca < n ? cols[ca] : nullptr;
        ta[u] = ca < ntemp;
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int cb = tl.y * DT + u * 8 + cg;
        pb[u] = (!DIAG && cb < n) ? cols[cb] : nullptr;
        tb[u] = cb < ntemp;
    }
    // one stage of one operand into registers: zeros past the slab's end and past column n, the mask multiplied into templates
    auto fetch = [&](double *dst, const double *const *ptr, const bool *tmpl, int cnt, long long q) __attribute__((always_inline)) {
        const long long p = q + px;
        const bool ok = p < q1;
        const double m = (ok && mask) ? mask[p >= npix ? p - npix : p] : 1.0;
#pragma unroll
        for (int u = 0; u < cnt; ++u) {
            double a = (ok && ptr[u]) ? ptr[u][p] : 0.0;
            if (mask && tmpl[u]) a *= m;
            dst[u] = a;
        }
    };
    double4_t acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (double4_t){0.0, 0.0, 0.0, 0.0};
    const int ai = (w >> 1) * 32 + r, bj = (w & 1) * 32 + r;
    // a 16 x 16 block is worked on only if it holds a column pair the result keeps (wave-uniform): rows and columns below n, and on a
    // diagonal tile the blocks on or above the diagonal (k_dp_reduce reads li <= lj there)
    bool live[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int bi = (w >> 1) * 2 + x, bjb = (w & 1) * 2 + y;
            live[x][y] = tl.x * DT + 16 * bi < n && tl.y * DT + 16 * bjb < n && (!DIAG || bi <= bjb);
        }
    auto stage = [&](const double(*A)[DLD], const double(*B)[DLD]) __attribute__((always_inline)) {
#pragma unroll
        for (int kk = 0; kk < DK / 4; ++kk) {
            const int k = 4 * kk + kq;
            const double a0 = A[ai][k], a1 = A[ai + 16][k];
            const double b0 = B[bj][k], b1 = B[bj + 16][k];
            if (live[0][0]) acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            if (live[0][1]) acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            if (live[1][0]) acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            if (live[1][1]) acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    };
    double ra[8], rb[8];  // DIAG: rb is the stage after ra's
    fetch(ra, pa, ta, 8, q0);
    if (DIAG) {
        fetch(rb, pa, ta, 8, q0 + DK);
        int s = 0;
        for (long long q = q0; q < q1; q += DK, s ^= 1) {
            // half s was last read two stages ago: every wave has passed the barrier of the stage between
#pragma unroll
            for (int u = 0; u < 8; ++u) sm[s][u * 8 + cg][px] = ra[u];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 8; ++u) ra[u] = rb[u];
            fetch(rb, pa, ta, 8, q + 2 * DK);
            stage(sm[s], sm[s]);
        }
    } else {
        fetch(rb, pb, tb, NB, q0);
        for (long long q = q0; q < q1; q += DK) {
            __syncthreads();  // the previous stage has been read
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                sm[0][u * 8 + cg][px] = ra[u];
                sm[1][u * 8 + cg][px] = rb[u];
            }
            __syncthreads();
            if (q + DK < q1) {
                fetch(ra, pa, ta, 8, q + DK);
                fetch(rb, pb, tb, NB, q + DK);
            }
            stage(sm[0], sm[1]);
        }
    }
    double *po = part + ((long long)tile * nslab + blockIdx.x) * (DT * DT);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int li = (w >> 1) * 32 + 16 * x + kq + 4 * q, lj = (w & 1) * 32 + 16 * y + r;
                po[li * DT + lj] = acc[x][y][q];
            }
}

// full[gi][gj] = full[gj][gi] = sum over the slabs of the tile's element, slab 0 first.  Grid (16, tiles): one element per thread.
__global__ __launch_bounds__(256) void k_dp_reduce(int n, int nslab, const int2 *__restrict__ tiles, const double *__restrict__ part,
                                                   double *__restrict__ full)
{
    const int2 tl = tiles[blockIdx.y];
    const int e = blockIdx.x * 256 + threadIdx.x, li = e >> 6, lj = e & 63;
    const int gi = tl.x * DT + li, gj = tl.y * DT + lj;
    if (gi >= n || gj >= n || (tl.x == tl.y && li > lj)) return;
    const double *p = part + (long long)blockIdx.y * nslab * (DT * DT) + e;
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += p[(long long)k * (DT * DT)];
    full[(long long)gi * n + gj] = s;
    full[(long long)gj * n + gi] = s;
}

struct ApplyMaps {
    const double *in[DA_MB];
    double *out[DA_MB];
};

template <int NM>
__global__ __launch_bounds__(256) void k_dp_apply(long long Q, long long npix, int ntemp, const double *const *__restrict__ tp,
                                                  const double *__restrict__ mask, int nm, ApplyMaps am, const double *__restrict__ alpha)
{
#pragma clang fp contract(off)
    const long long st = (long long)gridDim.x * 256;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < Q; q += st) {
        double s[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) s[m] = 0.0;
#pragma unroll 4
        for (int i = 0; i < ntemp; ++i) {
            const double tv = tp[i][q];
#pragma unroll
            for (int m = 0; m < NM; ++m)
                if (m < nm) s[m] = s[m] + alpha[(long long)m * ntemp + i] * tv;
        }
        const double v = mask ? mask[q >= npix ? q - npix : q] : 1.0;
#pragma unroll
        for (int m = 0; m < NM; ++m)
            if (m < nm) {
                const double f = mask ? v * s[m] : s[m];
                am.out[m][q] = am.in[m][q] - f;
            }
    }
}

__global__ __launch_bounds__(256) void k_alm_apply_cl(int lmax, int nin, int nout, const double *__restrict__ cl, const double2 *__restrict__ in,
                                                      double2 *__restrict__ out)
{
    const int m = blockIdx.y, l = m + blockIdx.x * 256 + threadIdx.x;
    if (l > lmax) return;
    const long long nlm = (long long)(lmax + 1) * (lmax + 2) / 2, at = (long long)m * (2 * lmax + 1 - m) / 2 + l;
    const int nl = lmax + 1;
    const double2 a0 = in[at], a1 = nin > 1 ? in[nlm + at] : make_double2(0.0, 0.0);
    for (int x = 0; x < nout; ++x) {
        const double c0 = cl[(long long)(x * nin) * nl + l];
        double2 o = make_double2(c0 * a0.x, c0 * a0.y);
        if (nin > 1) {
            const double c1 = cl[(long long)(x * nin + 1) * nl + l];
            o.x += c1 * a1.x;
            o.y += c1 * a1.y;
        }
        out[(long long)x * nlm + at] = o;
    }
}

struct DpScratch {
    DevBuf part, full;
};
DpScratch *g_dp = nullptr;
unsigned long long g_dp_flops = 0;

bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

void deproject_drop_cache()
{
    if (!g_dp) return;
    g_dp->part.release();
    g_dp->full.release();
}

int deproject_exec_flops(unsigned long long *v, bool reset)
{
    *v = g_dp_flops;
    if (reset) g_dp_flops = 0;
    return HX_OK;
}

}  // namespace hx

using namespace hx;

extern "C" int hx_deproject_gram(int64_t npix, int ncomp, int ntemp, const double *const *templates, int nmap, const double *const *maps,
                                 const double *mask, double *gram)
{
    HX_TRY(ensure_ready());
    // ---- arguments: everything is checked before anything is written ----
    if (npix < 1) return fail(HX_ERR_ARG, "hx_deproject_gram: npix = %lld", (long long)npix);
    if (ncomp != 1 && ncomp != 2) return fail(HX_ERR_ARG, "hx_deproject_gram: ncomp = %d (1 or 2)", ncomp);
    if (ntemp < 0 || nmap < 0) return fail(HX_ERR_ARG, "hx_deproject_gram: ntemp = %d, nmap = %d", ntemp, nmap);
    const long long nn = (long long)ntemp + nmap;
    if (nn < 1 || nn > DP_MAX_N) return fail(HX_ERR_ARG, "hx_deproject_gram: %lld columns (templates + maps), 1 .. %d are supported", nn, DP_MAX_N);
    if (!gram || (ntemp > 0 && !templates) || (nmap > 0 && !maps)) return fail(HX_ERR_ARG, "hx_deproject_gram: null pointer");
    for (int i = 0; i < ntemp; ++i)
        if (!templates[i]) return fail(HX_ERR_ARG, "hx_deproject_gram: template %d is a null pointer", i);
    for (int i = 0; i < nmap; ++i)
        if (!maps[i]) return fail(HX_ERR_ARG, "hx_deproject_gram: map %d is a null pointer", i);
    const int n = (int)nn;
    const long long Q = (long long)npix * ncomp;
    const size_t colbytes = sizeof(double) * (size_t)Q, gbytes = sizeof(double) * (size_t)n * n;
    for (int c = 0; c < n; ++c) {
        const void *p = c < ntemp ? templates[c] : maps[c - ntemp];
        if (ranges_overlap(p, colbytes, gram, gbytes) || (mask && ranges_overlap(mask, sizeof(double) * (size_t)npix, gram, gbytes)))
            return fail(HX_ERR_ARG, "hx_deproject_gram: gram overlaps an input");
    }
    // the slab partition: a function of (Q, n) alone
    const int nt = (n + DT - 1) / DT, ntiles = nt * (nt + 1) / 2;
    const long long target = (DP_TARGET_GROUPS + ntiles - 1) / ntiles;
    long long slab = std::max((Q + target - 1) / target, DP_MIN_SLAB);
    if (const char *hook = getenv("HX_DEPROJ_SLAB")) {  // (tests) the slab length; read at every call
        const long long h = atoll(hook);
        if (h > 0) slab = h;
    }
    slab = (slab + DK - 1) / DK * DK;
    const long long nslab_ll = (Q + slab - 1) / slab;
    if (nslab_ll > 1 << 20) return fail(HX_ERR_ARG, "hx_deproject_gram: HX_DEPROJ_SLAB = %lld cuts %lld elements into %lld slabs", slab, Q, nslab_ll);
    const int nslab = (int)nslab_ll;
    if (!g_dp) g_dp = new DpScratch;
    const size_t pbytes = sizeof(double) * (size_t)ntiles * nslab * (DT * DT);
    if (g_dp->part.bytes < pbytes) {
        size_t free_b = 0, total_b = 0;
        HX_HIP(hipMemGetInfo(&free_b, &total_b));
        if ((double)pbytes > 0.9 * ((double)free_b + (double)g_dp->part.bytes))
            return fail(HX_ERR_MEM, "hx_deproject_gram: %d tiles x %d slabs need %.2f GiB of scratch, %.2f GiB are free", ntiles, nslab,
                        pbytes / 1073741824.0, free_b / 1073741824.0);
        g_dp->part.release();  // (not both copies at once)
    }
    HX_TRY(g_dp->part.alloc(pbytes));
    HX_TRY(g_dp->full.alloc(gbytes));

    std::vector<InView> views((size_t)n);
    std::vector<const double *> cols((size_t)n);
    for (int c = 0; c < n; ++c) {
        HX_TRY(views[c].bind(c < ntemp ? templates[c] : maps[c - ntemp], colbytes));
        cols[c] = views[c].as<double>();
    }
    InView vmask;
    if (mask) HX_TRY(vmask.bind(mask, sizeof(double) * (size_t)npix));
    std::vector<int2> tiles;  // the diagonal tiles first: they have a kernel of their own
    for (int I = 0; I < nt; ++I) tiles.push_back(make_int2(I, I));
    for (int I = 0; I < nt; ++I)
        for (int J = I + 1; J < nt; ++J) tiles.push_back(make_int2(I, J));
    DevBuf b_cols, b_tiles;
    HX_TRY(upload_vec(b_cols, cols));
    HX_TRY(upload_vec(b_tiles, tiles));
    hipStream_t st = rt().stream;
    double *full = g_dp->full.as<double>();
    {
        ProfScope prof("deproject_gram");
        const double *dm = mask ? vmask.as<double>() : nullptr;
        hipLaunchKernelGGL(k_dp_gram<true>, dim3((unsigned)nslab, (unsigned)nt), dim3(256), 0, st, Q, (long long)npix, n, ntemp,
                           b_cols.as<const double *>(), dm, slab, nslab, b_tiles.as<int2>(), 0, g_dp->part.as<double>());
        if (ntiles > nt)
            hipLaunchKernelGGL(k_dp_gram<false>, dim3((unsigned)nslab, (unsigned)(ntiles - nt)), dim3(256), 0, st, Q, (long long)npix, n, ntemp,
                               b_cols.as<const double *>(), dm, slab, nslab, b_tiles.as<int2>(), nt, g_dp->part.as<double>());
        hipLaunchKernelGGL(k_dp_reduce, dim3(DT * DT / 256, (unsigned)ntiles), dim3(256), 0, st, n, nslab, b_tiles.as<int2>(),
                           g_dp->part.as<double>(), full);
        HX_HIP(hipGetLastError());
    }
    // stages executed: every work-group runs ceil(its slab / DK) stages of DK / 4 steps, one instruction of 2 * 16 * 16 * 4 flops per live block
    {
        const long long last = Q - (long long)(nslab - 1) * slab;
        const unsigned long long stages = (unsigned long long)(nslab - 1) * (slab / DK) + (unsigned long long)((last + DK - 1) / DK);
        unsigned long long blocks = 0;  // live 16 x 16 blocks of all tiles
        for (const int2 &tl : tiles) {
            const int rb = std::min(4, (n - tl.x * DT + 15) / 16), cb = std::min(4, (n - tl.y * DT + 15) / 16);
            blocks += tl.x == tl.y ? (unsigned long long)rb * (rb + 1) / 2 : (unsigned long long)rb * cb;
        }
        g_dp_flops += stages * (DK / 4) * blocks * 2048ull;
    }
    std::vector<double> diag((size_t)n);
    HX_HIP(hipMemcpy2DAsync(diag.data(), sizeof(double), full, sizeof(double) * (size_t)(n + 1), sizeof(double), (size_t)n, hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < n; ++c)
        if (!std::isfinite(diag[c]))
            return c < ntemp ? fail(HX_ERR_ARG, "hx_deproject_gram: template %d holds a NaN or an infinite value (or its square sum overflows)", c)
                             : fail(HX_ERR_ARG, "hx_deproject_gram: map %d holds a NaN or an infinite value (or its square sum overflows)", c - ntemp);
    if (is_device_ptr(gram)) HX_HIP(hipMemcpyAsync(gram, full, gbytes, hipMemcpyDeviceToDevice, st));
    else HX_TRY(copy_d2h(gram, full, gbytes));
    HX_HIP(hipStreamSynchronize(st));
    return HX_OK;
}

extern "C" int hx_deproject_apply(int64_t npix, int ncomp, int ntemp, const double *const *templates, const double *mask, int nmap,
                                  const double *const *maps, const double *alpha, double *const *out)
{
    HX_TRY(ensure_ready());
    if (npix < 1) return fail(HX_ERR_ARG, "hx_deproject_apply: npix = %lld", (long long)npix);
    if (ncomp != 1 && ncomp != 2) return fail(HX_ERR_ARG, "hx_deproject_apply: ncomp = %d (1 or 2)", ncomp);
    if (ntemp < 0 || ntemp > DP_MAX_N || nmap < 0) return fail(HX_ERR_ARG, "hx_deproject_apply: ntemp = %d (0 .. %d), nmap = %d", ntemp, DP_MAX_N, nmap);
    if ((ntemp > 0 && (!templates || (nmap > 0 && !alpha))) || (nmap > 0 && (!maps || !out))) return fail(HX_ERR_ARG, "hx_deproject_apply: null pointer");
    for (int i = 0; i < ntemp; ++i)
        if (!templates[i]) return fail(HX_ERR_ARG, "hx_deproject_apply: template %d is a null pointer", i);
    for (int m = 0; m < nmap; ++m)
        if (!maps[m] || !out[m]) return fail(HX_ERR_ARG, "hx_deproject_apply: map or output %d is a null pointer", m);
    const long long Q = (long long)npix * ncomp;
    const size_t colbytes = sizeof(double) * (size_t)Q, abytes = sizeof(double) * (size_t)nmap * (size_t)ntemp;
    for (int m = 0; m < nmap; ++m) {
        for (int k = 0; k < nmap; ++k) {
            if (k != m && ranges_overlap(out[m], colbytes, out[k], colbytes)) return fail(HX_ERR_ARG, "hx_deproject_apply: outputs %d and %d overlap", m, k);
            if (ranges_overlap(out[m], colbytes, maps[k], colbytes) && !(k == m && out[m] == maps[m]))
                return fail(HX_ERR_ARG, "hx_deproject_apply: output %d overlaps map %d (only out[m] == maps[m] is allowed)", m, k);
        }
        for (int i = 0; i < ntemp; ++i)
            if (ranges_overlap(out[m], colbytes, templates[i], colbytes)) return fail(HX_ERR_ARG, "hx_deproject_apply: output %d overlaps template %d", m, i);
        if (mask && ranges_overlap(out[m], colbytes, mask, sizeof(double) * (size_t)npix)) return fail(HX_ERR_ARG, "hx_deproject_apply: output %d overlaps the mask", m);
        if (abytes && ranges_overlap(out[m], colbytes, alpha, abytes)) return fail(HX_ERR_ARG, "hx_deproject_apply: output %d overlaps alpha", m);
    }
    if (nmap == 0) return HX_OK;

    std::vector<InView> vt((size_t)ntemp), vm((size_t)nmap);
    std::vector<OutView> vo((size_t)nmap);
    std::vector<const double *> tp((size_t)ntemp);
    for (int i = 0; i < ntemp; ++i) {
        HX_TRY(vt[i].bind(templates[i], colbytes));
        tp[i] = vt[i].as<double>();
    }
    for (int m = 0; m < nmap; ++m) {
        HX_TRY(vm[m].bind(maps[m], colbytes));
        HX_TRY(vo[m].bind(out[m], colbytes));
    }
    InView vmask, va;
    if (mask) HX_TRY(vmask.bind(mask, sizeof(double) * (size_t)npix));
    if (abytes) HX_TRY(va.bind(alpha, abytes));
    DevBuf b_tp;
    HX_TRY(upload_vec(b_tp, tp));
    hipStream_t st = rt().stream;
    const unsigned grid = (unsigned)std::min<long long>((Q + 255) / 256, 1 << 16);
    {
        ProfScope prof("deproject_apply");
        for (int m0 = 0; m0 < nmap; m0 += DA_MB) {
            const int nm = std::min(DA_MB, nmap - m0);
            ApplyMaps am;
            for (int m = 0; m < DA_MB; ++m) {
                am.in[m] = m < nm ? vm[m0 + m].as<double>() : nullptr;
                am.out[m] = m < nm ? vo[m0 + m].as<double>() : nullptr;
            }
            const double *al = abytes ? va.as<double>() + (size_t)m0 * ntemp : nullptr;
            const double *const *dtp = b_tp.as<const double *>();
            const double *dm = mask ? vmask.as<double>() : nullptr;
            if (nm == 1) hipLaunchKernelGGL(k_dp_apply<1>, dim3(grid), dim3(256), 0, st, Q, (long long)npix, ntemp, dtp, dm, nm, am, al);
            else if (nm == 2) hipLaunchKernelGGL(k_dp_apply<2>, dim3(grid), dim3(256), 0, st, Q, (long long)npix, ntemp, dtp, dm, nm, am, al);
            else if (nm <= 4) hipLaunchKernelGGL(k_dp_apply<4>, dim3(grid), dim3(256), 0, st, Q, (long long)npix, ntemp, dtp, dm, nm, am, al);
            else hipLaunchKernelGGL(k_dp_apply<DA_MB>, dim3(grid), dim3(256), 0, st, Q, (long long)npix, ntemp, dtp, dm, nm, am, al);
        }
        HX_HIP(hipGetLastError());
    }
    for (int m = 0; m < nmap; ++m) HX_TRY(vo[m].finish());
    HX_HIP(hipStreamSynchronize(st));
    return HX_OK;
}

extern "C" int hx_alm_apply_cl(int lmax, int nin, int nout, const double *cl, const double _Complex *alm_in, double _Complex *alm_out)
{
    HX_TRY(ensure_ready());
    if (lmax < 0 || lmax >= 65535) return fail(HX_ERR_ARG, "hx_alm_apply_cl: lmax = %d (0 .. 65534)", lmax);
    if (nin < 1 || nin > 2 || nout < 1 || nout > 2) return fail(HX_ERR_ARG, "hx_alm_apply_cl: nin = %d, nout = %d (1 or 2 each)", nin, nout);
    if (!cl || !alm_in || !alm_out) return fail(HX_ERR_ARG, "hx_alm_apply_cl: null pointer");
    const size_t nl = (size_t)lmax + 1, nlm = nl * (nl + 1) / 2;
    const size_t ibytes = sizeof(double2) * nlm * nin, obytes = sizeof(double2) * nlm * nout, cbytes = sizeof(double) * nl * nin * nout;
    if (ranges_overlap(alm_in, ibytes, alm_out, obytes) || ranges_overlap(cl, cbytes, alm_out, obytes))
        return fail(HX_ERR_ARG, "hx_alm_apply_cl: the output overlaps an input");
    InView vc, vi;
    OutView vo;
    HX_TRY(vc.bind(cl, cbytes));
    HX_TRY(vi.bind(alm_in, ibytes));
    HX_TRY(vo.bind(alm_out, obytes));
    {
        ProfScope prof("alm_apply_cl");
        hipLaunchKernelGGL(k_alm_apply_cl, dim3((unsigned)((nl + 255) / 256), (unsigned)nl), dim3(256), 0, rt().stream, lmax, nin, nout, vc.as<double>(),
                           vi.as<double2>(), vo.as<double2>());
        HX_HIP(hipGetLastError());
    }
    HX_TRY(vo.finish());
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}
