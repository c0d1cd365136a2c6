// hx_lognormal.hip -- the three device passes of the lognormal mocks.  gfx950 only.
//
//   k_lognormal_xi     element-wise over a batch of correlation-function columns [ncol][nnodes]: direction 0 (Gaussianise)
//                      out = log1p(xi f_c), direction 1 (realise) out = f_c expm1(xi), f_c one host factor per column.  Plain IEEE,
//                      contraction off: numpy's log1p(xi * f) and f * expm1(xi) are the definition.  Direction 0 is preceded by
//                      k_lognormal_xi_check, which records the smallest (column, node) whose argument is not > -1 in a flag word
//                      (64-bit atomicMin, as k_cl_cholesky does); the host reads it and launches nothing more when it is set.
//   k_lognormal_maps   out[r][p] = shift_r expm1(g[r][p] - sigma2_r / 2): one streaming pass, 16-byte loads and stores over the
//                      aligned middle of each row, the (at most one) element before it and after it by single lanes.
//   k_cl_nearest_psd   per multipole l the symmetric N x N matrix C_l of the packed spectra is scaled to unit diagonal,
//                      R = D^-1/2 C D^-1/2, diagonalised by cyclic Jacobi in round-robin order (hx_lognormal.h), its eigenvalues are
//                      raised to a floor and C' = D^1/2 V max(L, floor) V^T D^1/2 is written; a matrix with no eigenvalue below the
//                      floor is copied through bit for bit.
//                      One wave per l (work-groups of 64), lane i owning row / column i.  R and V live in LDS as [N][ld] doubles
//                      each: ld = N | 1 for N < 64 (an odd row stride: lanes walking down a column hit 32 different 8-byte bank
//                      pairs per half-wave), ld = 64 with the column index XOR-ed by (row & 31) for N = 64, which does the same
//                      without padding and keeps the footprint at the 64 KiB a work-group may have by default; along a row the lanes
//                      are a permutation of consecutive addresses either way.  A step of a sweep is: (1) lane k forms the rotation
//                      of pair k from a_pp, a_qq, a_pq; (2) rows p, q of every pair turn, lanes along the columns; (3) columns p, q
//                      of R and of V turn, lanes along the rows; (4) lane k writes the exact zeros and the diagonal of its pair.
//                      The (c, s) of pair k reach the other lanes by a lane read, not through LDS.  A sweep ends with the largest
//                      |off-diagonal| (lane i scans row i, then a wave maximum); the loop stops at <= 2^-50 or fails at PSD_SWEEPS.
//                      Global traffic is the packed [pair][l] array read with stride lmax + 1 between lanes; work-groups of
//                      neighbouring l are neighbours in the grid, so the lines they share are fetched once into L2.  No
//                      floating-point atomics, one owner per output element, every sum in a fixed order: the same bits in every run
//                      and for every split of the l range.
#include "hx_common.h"
#include "hx_lognormal.h"

namespace hx {

constexpr int PSD_MAXN = 64;     // components (one lane per row)
constexpr int PSD_SWEEPS = 40;   // sweep cap; reaching it is an error
constexpr int LNM_BLOCK = 256;   // threads per work-group of the element-wise passes

namespace {

constexpr unsigned long long FLAG_CLEAR = ~0ull;
constexpr double PSD_OFFDIAG = 0x1p-50;

struct LognScratch {
    DevBuf flag, out, change, par;
};
LognScratch *g_logn = nullptr;  // heap, never destroyed at exit (the HIP runtime may be gone by then)
LognScratch &logn_scratch()
{
    if (!g_logn) g_logn = new LognScratch;
    return *g_logn;
}

bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

int read_flag(unsigned long long *flag)
{
    hipStream_t st = rt().stream;
    *flag = FLAG_CLEAR;
    HX_HIP(hipMemcpyAsync(flag, logn_scratch().flag.p, sizeof(*flag), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    return HX_OK;
}

int clear_flag()
{
    LognScratch &sc = logn_scratch();
    HX_TRY(sc.flag.alloc(sizeof(unsigned long long)));
    HX_HIP(hipMemsetAsync(sc.flag.p, 0xff, sizeof(unsigned long long), rt().stream));
    return HX_OK;
}

// ---- xi <-> xi_G ------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(LNM_BLOCK) void k_lognormal_xi_check(int nnodes, long long total, const double *__restrict__ fac,
                                                                  const double *__restrict__ xi, unsigned long long *flag)
{
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * LNM_BLOCK + threadIdx.x;
    if (e >= total) return;
    const double arg = xi[e] * fac[e / nnodes];
    if (!(arg > -1.0)) atomicMin(flag, (unsigned long long)e);  // e = column * nnodes + node: the smallest (column, node)
}

__global__ __launch_bounds__(LNM_BLOCK) void k_lognormal_xi(int direction, int nnodes, long long total, const double *__restrict__ fac,
                                                            const double *xi, double *out)
{
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * LNM_BLOCK + threadIdx.x;
    if (e >= total) return;
    const double f = fac[e / nnodes], x = xi[e];
    if (direction == 0) {
        const double arg = x * f;
        out[e] = log1p(arg);
    } else {
        const double y = expm1(x);
        out[e] = f * y;
    }
}

// ---- the map pass -----------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double lognormal_value(double g, double half, double shift)
{
#pragma clang fp contract(off)
    const double x = g - half;
    const double y = expm1(x);
    return shift * y;
}

// par: [nrow][2] = (sigma2 / 2, shift).  vec: the rows of g and of out have the same alignment modulo 16 bytes.
__global__ __launch_bounds__(LNM_BLOCK) void k_lognormal_maps(long long npix, const double *__restrict__ par, const double *g, double *out, int vec)
{
    const int r = blockIdx.y;
    const double half = par[2 * r], shift = par[2 * r + 1];
    const double *gp = g + (long long)r * npix;
    double *op = out + (long long)r * npix;
    const long long tid = (long long)blockIdx.x * LNM_BLOCK + threadIdx.x, nth = (long long)gridDim.x * LNM_BLOCK;
    long long head = 0, nvec = 0;
    if (vec) {
        head = (long long)(((uintptr_t)gp >> 3) & 1);  // one element up to the next 16-byte boundary
        if (head > npix) head = npix;
        nvec = (npix - head) / 2;
    }
    const double2 *gv = reinterpret_cast<const double2 *>(gp + head);
    double2 *ov = reinterpret_cast<double2 *>(op + head);
    for (long long v = tid; v < nvec; v += nth) {
        const double2 x = gv[v];
        ov[v] = make_double2(lognormal_value(x.x, half, shift), lognormal_value(x.y, half, shift));
    }
    // what the vectors leave: [0, head) and [head + 2 nvec, npix) -- everything when vec is off
    const long long done = head + 2 * nvec, nrest = head + (npix - done);
    for (long long i = tid; i < nrest; i += nth) {
        const long long p = i < head ? i : done + (i - head);
        op[p] = lognormal_value(gp[p], half, shift);
    }
}

// ---- the nearest positive semi-definite spectra ------------------------------------------------------------------------------------

__device__ __forceinline__ long long pair_row(int a, int b, int n) { return (long long)a * n - (long long)a * (a - 1) / 2 + (b - a); }

// flag word: l << 16 | component << 2 | kind (0 negative diagonal, 1 non-finite entry, 2 sweep cap reached)
__global__ __launch_bounds__(LNM_BLOCK) void k_psd_check(int n, int lmax, const double *__restrict__ cl, unsigned long long *flag)
{
    const long long nl = lmax + 1, total = (long long)n * (n + 1) / 2 * nl;
    const long long e = (long long)blockIdx.x * LNM_BLOCK + threadIdx.x;
    if (e >= total) return;
    const double v = cl[e];
    const long long row = e / nl, l = e - row * nl;
    // the pair (a, b) of a packed row: a is the largest index with pair_row(a, a, n) <= row
    int a = 0;
    while (a + 1 < n && pair_row(a + 1, a + 1, n) <= row) ++a;
    const int b = a + (int)(row - pair_row(a, a, n));
    if (!isfinite(v)) atomicMin(flag, ((unsigned long long)l << 16) | ((unsigned long long)a << 2) | 1ull);
    else if (a == b && v < 0.0) atomicMin(flag, ((unsigned long long)l << 16) | ((unsigned long long)a << 2));
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(64) void k_cl_nearest_psd(int n, int lmax, int ld, int swm, double floor_, const double *__restrict__ cl,
                                                       double *__restrict__ out, double *__restrict__ change, unsigned long long *flag)
{
    extern __shared__ double lds[];
    double *R = lds, *V = lds + (size_t)n * ld;
    const int lane = threadIdx.x;
    const bool on = lane < n;
    const long long nl = lmax + 1;
    const int steps = hxlogn::rr_steps(n), npairs = hxlogn::rr_pairs(n);
#define AT(i, j) ((i) * ld + ((j) ^ ((i) & swm)))
    for (int l = blockIdx.x; l <= lmax; l += gridDim.x) {
        __syncthreads();  // (the previous l is done with the LDS)
        // scale to unit diagonal; lane j fills column j of R and V
        const double dj = on ? cl[pair_row(lane, lane, n) * nl + l] : 0.0;
        const double isj = dj > 0.0 ? 1.0 / sqrt(dj) : 0.0, sqj = sqrt(dj);
        bool dirty = false;  // a non-zero entry in the row or column of a component with C_jj = 0: to be zeroed
        if (on)
            for (int i = 0; i < n; ++i) {
                const double isi = __shfl(isj, i, 64);
                double r;
                if (i == lane) {
                    r = 1.0;  // (a component left out is a unit block of its own: eigenvalue 1, never raised)
                } else {
                    const double c = cl[(i < lane ? pair_row(i, lane, n) : pair_row(lane, i, n)) * nl + l];
                    r = c * isi * isj;
                    if (c != 0.0 && (isi == 0.0 || isj == 0.0)) dirty = true;
                }
                R[AT(i, lane)] = r;
                V[AT(i, lane)] = i == lane ? 1.0 : 0.0;
            }
        __syncthreads();

        bool converged = n == 1;
        for (int sweep = 0; sweep < PSD_SWEEPS && !converged; ++sweep) {
            for (int step = 0; step < steps; ++step) {
                // (1) lane k: the rotation of pair k
                int mp = 0, mq = 0;
                hxlogn::Rotation rot = {1.0, 0.0, 0.0};
                double app = 0.0, aqq = 0.0, apq = 0.0;
                const bool mine = lane < npairs && hxlogn::rr_pair(n, step, lane, &mp, &mq);
                if (mine) {
                    app = R[AT(mp, mp)];
                    aqq = R[AT(mq, mq)];
                    apq = R[AT(mp, mq)];
                    rot = hxlogn::jacobi_rotation(app, aqq, apq);
                }
                __syncthreads();
                // (2) rows p, q <- J^T rows; lane = column
                for (int k = 0; k < npairs; ++k) {
                    int p, q;
                    const bool valid = hxlogn::rr_pair(n, step, k, &p, &q);
                    const double c = __shfl(rot.c, k, 64), s = __shfl(rot.s, k, 64);
                    if (!valid || !on) continue;
                    const double x = R[AT(p, lane)], y = R[AT(q, lane)];
                    R[AT(p, lane)] = c * x - s * y;
                    R[AT(q, lane)] = s * x + c * y;
                }
                __syncthreads();
                // (3) columns p, q <- columns J, of R and of V; lane = row
                for (int k = 0; k < npairs; ++k) {
                    int p, q;
                    const bool valid = hxlogn::rr_pair(n, step, k, &p, &q);
                    const double c = __shfl(rot.c, k, 64), s = __shfl(rot.s, k, 64);
                    if (!valid || !on) continue;
                    const int ip = AT(lane, p), iq = AT(lane, q);
                    const double x = R[ip], y = R[iq];
                    R[ip] = c * x - s * y;
                    R[iq] = s * x + c * y;
                    const double u = V[ip], w = V[iq];
                    V[ip] = c * u - s * w;
                    V[iq] = s * u + c * w;
                }
                __syncthreads();
                // (4) lane k: what the rotation makes exactly
                if (mine && apq != 0.0) {
                    R[AT(mp, mp)] = app - rot.t * apq;
                    R[AT(mq, mq)] = aqq + rot.t * apq;
                    R[AT(mp, mq)] = 0.0;
                    R[AT(mq, mp)] = 0.0;
                }
                __syncthreads();
            }
            double off = 0.0;
            if (on)
                for (int j = 0; j < n; ++j)
                    if (j != lane) off = fmax(off, fabs(R[AT(lane, j)]));
            off = wave_max(off);
            converged = off <= PSD_OFFDIAG;  // (a NaN never converges and ends at the cap)
        }
        if (!converged) {
            if (lane == 0) atomicMin(flag, ((unsigned long long)l << 16) | 2ull);
            continue;
        }
        const double lam = on ? R[AT(lane, lane)] : 1.0;
        const bool low = lam < floor_;
        const bool repair = __any(low || dirty);
        double ch = 0.0;
        if (!repair) {
            if (on)
                for (int i = 0; i <= lane; ++i) {
                    const long long at = pair_row(i, lane, n) * nl + l;
                    out[at] = cl[at];
                }
        } else {
            // W = V max(L, floor) over R (lane = column k of V), then C'_ij = sqrt(d_i d_j) sum_k W_ik V_jk for i <= j, lane = j
            const double lk = low ? floor_ : lam;
            __syncthreads();
            if (on)
                for (int i = 0; i < n; ++i) R[AT(i, lane)] = V[AT(i, lane)] * lk;
            __syncthreads();
            if (on)
                for (int i = 0; i <= lane; ++i) {
                    double s = 0.0;
                    for (int k = 0; k < n; ++k) s += R[AT(i, k)] * V[AT(lane, k)];
                    const double sqi = __shfl(sqj, i, 64), isi = __shfl(isj, i, 64);
                    const long long at = pair_row(i, lane, n) * nl + l;
                    const double c0 = cl[at], c1 = sqi * sqj * s;
                    out[at] = c1;
                    const double w = isi * isj;
                    if (w != 0.0) ch = fmax(ch, fabs(c1 - c0) * w);
                    else if (c0 != 0.0) ch = INFINITY;
                }
        }
        ch = wave_max(ch);
        if (lane == 0) change[l] = ch;
    }
#undef AT
}

}  // namespace

void lognormal_drop_cache()
{
    if (!g_logn) return;
    g_logn->flag.release();
    g_logn->out.release();
    g_logn->change.release();
    g_logn->par.release();
}

}  // namespace hx

using namespace hx;

extern "C" int hx_lognormal_xi(int direction, int ncol, int nnodes, const double *factor, const double *xi, double *out)
{
    HX_TRY(ensure_ready());
    if (direction != 0 && direction != 1) return fail(HX_ERR_ARG, "hx_lognormal_xi: direction = %d (0: log1p, 1: expm1)", direction);
    if (ncol < 1 || nnodes < 1) return fail(HX_ERR_ARG, "hx_lognormal_xi: ncol = %d, nnodes = %d", ncol, nnodes);
    if (!factor || !xi || !out) return fail(HX_ERR_ARG, "hx_lognormal_xi: null pointer");
    const long long total = (long long)ncol * nnodes;
    const size_t bytes = sizeof(double) * (size_t)total;
    if (out != xi && ranges_overlap(xi, bytes, out, bytes)) return fail(HX_ERR_ARG, "hx_lognormal_xi: out overlaps xi (only out == xi is allowed)");
    LognScratch &sc = logn_scratch();
    hipStream_t st = rt().stream;
    HX_TRY(sc.par.alloc(sizeof(double) * (size_t)ncol));
    HX_HIP(hipMemcpyAsync(sc.par.p, factor, sizeof(double) * (size_t)ncol, hipMemcpyHostToDevice, st));
    HX_HIP(hipStreamSynchronize(st));  // (factor is the caller's pageable memory)
    InView vin;
    HX_TRY(vin.bind(xi, bytes));
    const dim3 grid((unsigned)((total + LNM_BLOCK - 1) / LNM_BLOCK));
    if (direction == 0) {
        HX_TRY(clear_flag());
        hipLaunchKernelGGL(k_lognormal_xi_check, grid, dim3(LNM_BLOCK), 0, st, nnodes, total, sc.par.as<double>(), vin.as<double>(),
                           sc.flag.as<unsigned long long>());
        HX_HIP(hipGetLastError());
        unsigned long long flag;
        HX_TRY(read_flag(&flag));
        if (flag != FLAG_CLEAR)
            return fail(HX_ERR_ARG, "hx_lognormal_xi: the argument of log1p is <= -1 or NaN at column %lld, node %lld", (long long)(flag / (unsigned long long)nnodes),
                        (long long)(flag % (unsigned long long)nnodes));
    }
    OutView vout;
    HX_TRY(vout.bind(out, bytes));
    {
        ProfScope prof("lognormal_xi");
        hipLaunchKernelGGL(k_lognormal_xi, grid, dim3(LNM_BLOCK), 0, st, direction, nnodes, total, sc.par.as<double>(), vin.as<double>(), vout.as<double>());
        HX_HIP(hipGetLastError());
    }
    HX_TRY(vout.finish());
    HX_HIP(hipStreamSynchronize(st));
    return HX_OK;
}

extern "C" int hx_lognormal_maps(int nrow, int64_t npix, const double *sigma2, const double *shift, const double *g, double *out)
{
    HX_TRY(ensure_ready());
    if (nrow < 1 || nrow > 65535) return fail(HX_ERR_ARG, "hx_lognormal_maps: nrow = %d (1 .. 65535)", nrow);
    if (npix < 1) return fail(HX_ERR_ARG, "hx_lognormal_maps: npix = %lld", (long long)npix);
    if (!sigma2 || !shift || !g || !out) return fail(HX_ERR_ARG, "hx_lognormal_maps: null pointer");
    const size_t bytes = sizeof(double) * (size_t)nrow * (size_t)npix;
    if (out != g && ranges_overlap(g, bytes, out, bytes)) return fail(HX_ERR_ARG, "hx_lognormal_maps: out overlaps g (only out == g is allowed)");
    std::vector<double> par((size_t)2 * nrow);
    for (int r = 0; r < nrow; ++r) {
        if (!(shift[r] > 0.0) || !std::isfinite(shift[r]) || !(sigma2[r] >= 0.0) || !std::isfinite(sigma2[r]))
            return fail(HX_ERR_ARG, "hx_lognormal_maps: row %d has shift = %g, sigma2 = %g (shift > 0, sigma2 >= 0, both finite)", r, shift[r], sigma2[r]);
        par[2 * (size_t)r] = 0.5 * sigma2[r];
        par[2 * (size_t)r + 1] = shift[r];
    }
    LognScratch &sc = logn_scratch();
    HX_TRY(upload_vec(sc.par, par));
    InView vin;
    HX_TRY(vin.bind(g, bytes));
    OutView vout;
    HX_TRY(vout.bind(out, bytes));
    const uintptr_t ga = (uintptr_t)vin.dev, oa = (uintptr_t)vout.dev;
    if ((ga | oa) & 7) return fail(HX_ERR_ARG, "hx_lognormal_maps: a buffer is not aligned to 8 bytes");
    const int vec = ((ga ^ oa) & 15) == 0 ? 1 : 0;
    const long long per_thread = 4;  // 16-byte vectors per work item: enough in flight per lane, and a grid that covers nside 8192
    const long long nvec = npix / 2 + 1;
    const unsigned gx = (unsigned)std::min<long long>((nvec + LNM_BLOCK * per_thread - 1) / (LNM_BLOCK * per_thread), 1 << 20);
    {
        ProfScope prof("lognormal_maps");
        hipLaunchKernelGGL(k_lognormal_maps, dim3(gx, (unsigned)nrow), dim3(LNM_BLOCK), 0, rt().stream, (long long)npix, sc.par.as<double>(), vin.as<double>(),
                           vout.as<double>(), vec);
        HX_HIP(hipGetLastError());
    }
    HX_TRY(vout.finish());
    return finish_call();
}

extern "C" int hx_cl_nearest_psd(int ncomp, int lmax, const double *cl, double floor_, double *out, double *change)
{
    HX_TRY(ensure_ready());
    if (ncomp < 1 || ncomp > PSD_MAXN) return fail(HX_ERR_ARG, "hx_cl_nearest_psd: ncomp = %d, 1 .. %d components are supported", ncomp, PSD_MAXN);
    if (lmax < 0 || lmax >= (1 << 30)) return fail(HX_ERR_ARG, "hx_cl_nearest_psd: lmax = %d", lmax);
    if (!cl || !out) return fail(HX_ERR_ARG, "hx_cl_nearest_psd: null pointer");
    if (floor_ < 0.0) floor_ = 64.0 * ncomp * ncomp * 0x1p-52;  // the default
    if (!(floor_ >= 0.0) || !(floor_ < 1.0)) return fail(HX_ERR_ARG, "hx_cl_nearest_psd: floor = %g (0 <= floor < 1, negative: the default)", floor_);
    const size_t nl = (size_t)lmax + 1, bytes = sizeof(double) * (size_t)(ncomp * (ncomp + 1) / 2) * nl;
    if (change && (ranges_overlap(change, sizeof(double) * nl, cl, bytes) || ranges_overlap(change, sizeof(double) * nl, out, bytes)))
        return fail(HX_ERR_ARG, "hx_cl_nearest_psd: change overlaps cl or out");
    if (out != cl && ranges_overlap(cl, bytes, out, bytes)) return fail(HX_ERR_ARG, "hx_cl_nearest_psd: out overlaps cl (only out == cl is allowed)");
    LognScratch &sc = logn_scratch();
    hipStream_t st = rt().stream;
    InView vin;
    HX_TRY(vin.bind(cl, bytes));
    // into scratch first: a rejected input, or a matrix that does not converge, leaves the caller's arrays as they were
    HX_TRY(sc.out.alloc(bytes));
    HX_TRY(sc.change.alloc(sizeof(double) * nl));
    HX_TRY(clear_flag());
    const long long total = (long long)(bytes / sizeof(double));
    hipLaunchKernelGGL(k_psd_check, dim3((unsigned)((total + LNM_BLOCK - 1) / LNM_BLOCK)), dim3(LNM_BLOCK), 0, st, ncomp, lmax, vin.as<double>(),
                       sc.flag.as<unsigned long long>());
    HX_HIP(hipGetLastError());
    unsigned long long flag;
    HX_TRY(read_flag(&flag));
    if (flag == FLAG_CLEAR) {
        const int ld = ncomp == PSD_MAXN ? PSD_MAXN : (ncomp | 1), swm = ncomp == PSD_MAXN ? 31 : 0;
        const size_t lds = sizeof(double) * 2 * (size_t)ncomp * ld;  // <= 64 KiB
        ProfScope prof("cl_nearest_psd");
        hipLaunchKernelGGL(k_cl_nearest_psd, dim3((unsigned)std::min<size_t>(nl, 1 << 16)), dim3(64), lds, st, ncomp, lmax, ld, swm, floor_, vin.as<double>(),
                           sc.out.as<double>(), sc.change.as<double>(), sc.flag.as<unsigned long long>());
        HX_HIP(hipGetLastError());
    }
    if (flag == FLAG_CLEAR) HX_TRY(read_flag(&flag));
    if (flag != FLAG_CLEAR) {
        const long long l = (long long)(flag >> 16);
        const int comp = (int)((flag & 0xffffull) >> 2), kind = (int)(flag & 3ull);
        if (kind == 1) return fail(HX_ERR_ARG, "hx_cl_nearest_psd: NaN or Inf in the spectra at l = %lld (component %d)", l, comp);
        if (kind == 0) return fail(HX_ERR_ARG, "hx_cl_nearest_psd: negative auto-spectrum at l = %lld (component %d)", l, comp);
        return fail(HX_ERR_UNSUPPORTED, "hx_cl_nearest_psd: the Jacobi sweeps did not converge within %d sweeps at l = %lld", PSD_SWEEPS, l);
    }
    if (is_device_ptr(out)) HX_HIP(hipMemcpyAsync(out, sc.out.p, bytes, hipMemcpyDeviceToDevice, st));
    else HX_TRY(copy_d2h(out, sc.out.p, bytes));
    if (change) {
        if (is_device_ptr(change)) HX_HIP(hipMemcpyAsync(change, sc.change.p, sizeof(double) * nl, hipMemcpyDeviceToDevice, st));
        else HX_TRY(copy_d2h(change, sc.change.p, sizeof(double) * nl));
    }
    HX_HIP(hipStreamSynchronize(st));  // (the scratch may be reused by the next call)
    return HX_OK;
}
