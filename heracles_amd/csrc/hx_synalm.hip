// hx_synalm.hip -- Gaussian mock alms of a set of spectra: a_lm^i = sum_{j <= i} L_ij(l) z_lm^j, L_l the lower Cholesky factor of
// the cross-spectrum matrix C_l and z complex standard normals from a counter-based generator (hx_philox.h).  gfx950 only.
//
// Packing: the symmetric N x N matrices come as rows p(a, b) = a N - a (a - 1) / 2 + (b - a), a <= b (the order of
// itertools.combinations_with_replacement), each lmax + 1 long; the factor is kept the same way, L_ij (i >= j) at row p(j, i), so
// that lanes along l read and write neighbouring addresses in both kernels.
//
//   k_cl_cholesky  one work item per l: the factor column by column in f64, a pivot d <= tau_j = 4 N 2^-52 C_jj zeroes its column,
//                  d < -tau_j or a non-finite input records (l, component) in a flag word (atomicMin: the smallest l wins).
//   k_synalm       the hot path.  A work item owns one l (SYN_LT consecutive l per work-group, so a wave stores 64 consecutive
//                  complex coefficients per component) and SYN_MC consecutive orders m.  Output components go in register blocks
//                  of RB rows: for each column j <= the block's last row the item loads its RB factor entries once, draws
//                  z^j for its SYN_MC orders and adds the products, so the factor is fetched once per chunk of orders and not
//                  once per coefficient.  Draws are recomputed per register block (nothing is spilled; the sum over j runs
//                  in ascending order, as the definition asks).  The kernel is bound by the arithmetic of the draws (about 500
//                  lane cycles each), so RB is as large as the registers allow: SYN_RB = 16, and SYN_RB_SMALL = 8 for calls of
//                  at most 8 components, which would only add zeros in the larger block.  Work-groups of one l tile are
//                  neighbours in the grid (blockIdx.x runs over the orders): they share the tile's factor in L2.
#include "hx_common.h"
#include "hx_philox.h"

namespace hx {

constexpr int SYN_LT = 256;  // l per work-group (4 waves)
constexpr int SYN_MC = 2;    // orders m per work item
constexpr int SYN_RB = 16;   // output components per register block
constexpr int SYN_RB_SMALL = 8;  // the same for calls of at most this many components
constexpr int SYN_MAXN = 64;

namespace {

struct SynalmScratch {
    DevBuf chol, flag;
};
SynalmScratch *g_synalm_scratch = nullptr;  // heap, never destroyed at exit (the HIP runtime may be gone by then)
SynalmScratch &synalm_scratch()
{
    if (!g_synalm_scratch) g_synalm_scratch = new SynalmScratch;
    return *g_synalm_scratch;
}

constexpr unsigned long long FLAG_CLEAR = ~0ull;

__device__ __forceinline__ long long pair_row(int a, int b, int n) { return (long long)a * n - (long long)a * (a - 1) / 2 + (b - a); }

// flag word: l << 16 | component << 1 | (1 = non-finite input, 0 = negative pivot)
__global__ __launch_bounds__(64) void k_cl_cholesky(int n, int lmax, const double *__restrict__ cl, double *chol, unsigned long long *flag)
{
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l > lmax) return;
    const long long nl = lmax + 1;
    const int npair = n * (n + 1) / 2;
    for (int p = 0; p < npair; ++p)
        if (!isfinite(cl[p * nl + l])) {
            atomicMin(flag, ((unsigned long long)l << 16) | 1ull);
            return;
        }
    const double eps4n = 4.0 * n * 0x1p-52;
    for (int j = 0; j < n; ++j) {
        const double cjj = cl[pair_row(j, j, n) * nl + l];
        double d = cjj;
        for (int k = 0; k < j; ++k) {
            const double v = chol[pair_row(k, j, n) * nl + l];
            d -= v * v;
        }
        const double tau = eps4n * cjj;
        if (d < -tau) {
            atomicMin(flag, ((unsigned long long)l << 16) | ((unsigned long long)j << 1));
            return;
        }
        if (d <= tau) {
            for (int i = j; i < n; ++i) chol[pair_row(j, i, n) * nl + l] = 0.0;
            continue;
        }
        const double ljj = sqrt(d);
        chol[pair_row(j, j, n) * nl + l] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double s = cl[pair_row(j, i, n) * nl + l];
            for (int k = 0; k < j; ++k) s -= chol[pair_row(k, i, n) * nl + l] * chol[pair_row(k, j, n) * nl + l];
            chol[pair_row(j, i, n) * nl + l] = s / ljj;
        }
    }
}

template <int RB>
__global__ __launch_bounds__(SYN_LT) void k_synalm(int n, int lmax, const double *__restrict__ chol, uint32_t key0, uint32_t key1,
                                                   uint32_t realisation, double2 *__restrict__ alms)
{
    const int l = blockIdx.y * SYN_LT + threadIdx.x;
    const int m0 = blockIdx.x * SYN_MC;
    if (l > lmax || m0 > l) return;
    const long long nl = lmax + 1, nlm = nl * (nl + 1) / 2;
    for (int i0 = 0; i0 < n; i0 += RB) {
        double ar[RB][SYN_MC], ai[RB][SYN_MC];
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int q = 0; q < SYN_MC; ++q) ar[r][q] = ai[r][q] = 0.0;
        const int jend = min(i0 + RB, n);
        for (int j = 0; j < jend; ++j) {
            double f[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int i = i0 + r;
                f[r] = (i >= j && i < n) ? chol[pair_row(j, i, n) * nl + l] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < SYN_MC; ++q) {
                double zr, zi;
                hxphilox::complex_normal((uint32_t)l, (uint32_t)(m0 + q), (uint32_t)j, realisation, key0, key1, &zr, &zi);
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    ar[r][q] += f[r] * zr;
                    ai[r][q] += f[r] * zi;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = i0 + r;
            if (i >= n) break;
#pragma unroll
            for (int q = 0; q < SYN_MC; ++q) {
                const int m = m0 + q;
                if (m <= l) alms[i * nlm + (long long)m * (2 * nl - 1 - m) / 2 + l] = make_double2(ar[r][q], ai[r][q]);
            }
        }
    }
}

// the factor of cl (device) into chol (device); HX_ERR_ARG with the smallest failing l named
int factor(const char *who, int n, int lmax, const double *d_cl, double *d_chol)
{
    SynalmScratch &sc = synalm_scratch();
    HX_TRY(sc.flag.alloc(sizeof(unsigned long long)));
    hipStream_t st = rt().stream;
    HX_HIP(hipMemsetAsync(sc.flag.p, 0xff, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_cl_cholesky, dim3((lmax + 64) / 64), dim3(64), 0, st, n, lmax, d_cl, d_chol, sc.flag.as<unsigned long long>());
    HX_HIP(hipGetLastError());
    unsigned long long flag = FLAG_CLEAR;
    HX_HIP(hipMemcpyAsync(&flag, sc.flag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (flag == FLAG_CLEAR) return HX_OK;
    const long long l = (long long)(flag >> 16);
    if (flag & 1ull) return fail(HX_ERR_ARG, "%s: NaN or Inf in the spectra at l = %lld", who, l);
    return fail(HX_ERR_ARG, "%s: the spectra are not positive semi-definite at l = %lld (component %d)", who, l, (int)((flag & 0xffffull) >> 1));
}

int check_args(const char *who, int n, int lmax, const void *cl, const void *out)
{
    if (n < 1 || n > SYN_MAXN) return fail(HX_ERR_ARG, "%s: ncomp = %d, 1 .. %d components are supported", who, n, SYN_MAXN);
    if (lmax < 0) return fail(HX_ERR_ARG, "%s: lmax = %d", who, lmax);
    if (!cl || !out) return fail(HX_ERR_ARG, "%s: null pointer", who);
    return HX_OK;
}

}  // namespace

void synalm_drop_cache()
{
    if (!g_synalm_scratch) return;
    g_synalm_scratch->chol.release();
    g_synalm_scratch->flag.release();
}

}  // namespace hx

using namespace hx;

extern "C" int hx_cl_cholesky(int ncomp, int lmax, const double *cl, double *chol)
{
    HX_TRY(ensure_ready());
    HX_TRY(check_args("hx_cl_cholesky", ncomp, lmax, cl, chol));
    const size_t bytes = sizeof(double) * (size_t)(ncomp * (ncomp + 1) / 2) * (size_t)(lmax + 1);
    InView vin;
    HX_TRY(vin.bind(cl, bytes));
    // into scratch first: a rejected input leaves the caller's array as it was
    SynalmScratch &sc = synalm_scratch();
    HX_TRY(sc.chol.alloc(bytes));
    HX_TRY(factor("hx_cl_cholesky", ncomp, lmax, vin.as<double>(), sc.chol.as<double>()));
    if (is_device_ptr(chol)) {
        HX_HIP(hipMemcpyAsync(chol, sc.chol.p, bytes, hipMemcpyDeviceToDevice, rt().stream));
        HX_HIP(hipStreamSynchronize(rt().stream));  // (the scratch may be reused by the next call)
    } else {
        HX_TRY(copy_d2h(chol, sc.chol.p, bytes));
    }
    return HX_OK;
}

extern "C" int hx_synalm(int ncomp, int lmax, const double *cl, uint64_t seed, uint32_t realisation, double *alms)
{
    HX_TRY(ensure_ready());
    HX_TRY(check_args("hx_synalm", ncomp, lmax, cl, alms));
    const size_t nl = (size_t)lmax + 1, nlm = nl * (nl + 1) / 2;
    const size_t cl_bytes = sizeof(double) * (size_t)(ncomp * (ncomp + 1) / 2) * nl;
    InView vin;
    HX_TRY(vin.bind(cl, cl_bytes));
    SynalmScratch &sc = synalm_scratch();
    HX_TRY(sc.chol.alloc(cl_bytes));
    HX_TRY(factor("hx_synalm", ncomp, lmax, vin.as<double>(), sc.chol.as<double>()));  // fails before anything is written
    OutView vout;
    HX_TRY(vout.bind(alms, sizeof(double2) * nlm * ncomp));
    {
        ProfScope prof("synalm");
        const dim3 grid((unsigned)((nl + SYN_MC - 1) / SYN_MC), (unsigned)((nl + SYN_LT - 1) / SYN_LT));
        hipLaunchKernelGGL(ncomp <= SYN_RB_SMALL ? k_synalm<SYN_RB_SMALL> : k_synalm<SYN_RB>, grid, dim3(SYN_LT), 0, rt().stream, ncomp, lmax,
                           sc.chol.as<double>(), (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), realisation, vout.as<double2>());
    }
    HX_HIP(hipGetLastError());
    HX_TRY(vout.finish());
    return finish_call();
}
