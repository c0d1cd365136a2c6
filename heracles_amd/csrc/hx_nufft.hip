// hx_nufft.hip -- adjoint spherical-harmonic synthesis at arbitrary points:
//     a_lm = sum_p v_p conj( sY_lm(theta_p, phi_p) ),    s = 0 (one real value per point) or 2 ((Q, U) -> (E, B)),
// the operation behind heracles.ducc.DiscreteMapper.map_values (heracles/ducc.py:92-133: one call of
// ducc0.sht.adjoint_synthesis_general(map, spin, lmax, loc, epsilon) per catalogue page; ducc0 is a third-party dependency that is
// not part of the reference tree -- what is built here is the published construction of that routine: a type-1 non-uniform FFT
// onto the doubly periodic (theta, phi) torus followed by the adjoint Legendre stage on equidistant rings).
//
// lambda_lm(theta), continued to the full circle, is a trigonometric polynomial of degree <= l with
// lambda_lm(2 pi - theta) = (-1)^m lambda_lm(theta) (both spins: d^l_{m,+-2}(-theta) = (-1)^(m-+2) d^l_{m,+-2}(theta)).  Hence, with
//     G(k, m) = sum_p v_p exp(-i (k theta_p + m phi_p)),  |k| <= lmax, 0 <= m <= lmax          (type-1 NUFFT, 2-D)
//     h_m(theta) = sum_k G(k, m) exp(i k theta),
// Parseval on N > 2 lmax equidistant points theta_j = 2 pi (j + 1/2) / N gives EXACTLY
//     a_lm = (1 / N) sum_{j < N/2} lambda_lm(theta_j) [ h_m(theta_j) + (-1)^m h_m(2 pi - theta_j) ],
// i.e. the Legendre analysis kernel of the HEALPix path (hx_analysis.hip) on N / 2 rings with ring "spectra" h_m and weight
// 1 / N -- no quadrature error, no iteration.  The only approximation is the NUFFT:
//   1. spread: every point adds v_p psi(x - theta_p) psi(y - phi_p) to an n1 x n1 grid over [0, 2 pi)^2, n1 = 2 N >= 2 (2 lmax + 1),
//      psi = "exponential of semicircle" kernel exp(beta (sqrt(1 - (2u/W)^2) - 1)) of W grid cells, beta = 2.3 W
//      (Barnett, Magland & af Klinteberg 2019); W = ceil(log10(1 / epsilon)) + 3 <= 16: 1e-12 -> 15 cells, error 4e-14 at the
//      smallest oversampling that can occur (n1 / (2 lmax + 1) >= 2);
//   2. FFT along phi of the rows the points can touch, divided by psi^(m): T[m][row];
//   3. FFT along theta of every m, divided by psi^(k), shifted by half a cell of the N-grid: U[m][k mod N], |k| <= lmax;
//   4. inverse FFT of length N: h_m(theta_j).
// FFTs: the in-LDS power-of-two kernels of the ring stage (hx_fft_core.h); lengths above 8192 points (128 KiB) as a radix-2 / 4
// decimation-in-frequency step over sub-transforms of 8192.
//
// Step 1 is additive in the points and steps 2-4 are linear, so the transform has two halves with one owner each here (declared in
// hx_common.h): "spread n points of one component into a given grid" (pointsht_order + pointsht_spread_one: no memset) and "grids to
// alm" (pointsht_grids_to_alm).  hx_pointsht_adjoint is memset + half one + half two on the one grid the object owns; hx_catalm
// (hx_catalm.hip) keeps one grid per component resident over the pages of a catalogue and runs half two once at the end.
// The spread adds with hardware float64 atomics (global, and LDS in the tile kernel), whose order is not fixed: results agree from run
// to run to rounding, NOT bit for bit.
// The forward direction, alm -> values at the points (hx_pointsht_synthesis, hx_pointgrid_*), is the same chain transposed; it is
// described where its kernels start, below k_nufft_fft.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <memory>

#include "hx_sht_common.h"

#include "hx_sort.h"
#include "hx_wigner.h"

using namespace hx;
using namespace hxfft;

struct hx_pointsht {
    int lmax = 0, N = 0, n1 = 0, W = 0, twN = 2;
    double beta = 0.0, epsilon = 0.0;
    hx_plan *eq = nullptr;
    hx::DevBuf tw, dec_phi, fac_theta, grid, T, U, h, nbad, key, key2, idx, idx2, sort_tmp;
    // forward direction: the rings next to the poles (k_polar_modes), nodes x + xlo and one Wigner-d table per spin weight
    int polar_K = 0, polar_M = 0;
    hx::DevBuf polar_x, polar_xlo;
    std::map<int, std::unique_ptr<hx::DevBuf>> polar_tab;
};

namespace hx {

constexpr int NUFFT_LDS_MAX = 8192;  // points of one in-LDS transform
constexpr int NUFFT_WMAX = 16;

__device__ __host__ inline double es_kernel(double u, double inv_hw, double beta)
{
    const double t = u * inv_hw, a = 1.0 - t * t;
    return a > 0.0 ? exp(beta * (sqrt(a) - 1.0)) : 0.0;
}

// One thread per point: W x W atomic additions per component grid.  loc = (theta, phi) pairs in radians (ducc's `loc`).
__global__ __launch_bounds__(256) void k_nufft_spread(long long npts, const double2 *__restrict__ loc, const double *__restrict__ val,
                                                      double *__restrict__ grid, int n1, int W, double beta,
                                                      unsigned long long *__restrict__ nbad)
{
    const double sc = (double)n1 / (2.0 * M_PI), inv_hw = 2.0 / W, hw = 0.5 * W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npts; p += (long long)gridDim.x * blockDim.x) {
        const double2 tp = loc[p];
        const double v = val[p];
        if (!(tp.x >= 0.0 && tp.x <= M_PI) || !isfinite(tp.y) || !isfinite(v)) {
            atomicAdd(nbad, 1ULL);
            continue;
        }
        if (v == 0.0) continue;
        const double x = tp.x * sc;
        double ph = fmod(tp.y, 2.0 * M_PI);
        if (ph < 0.0) ph += 2.0 * M_PI;
        const double y = ph * sc;
        const long long i0 = (long long)ceil(x - hw), j0 = (long long)ceil(y - hw);
        double wi[NUFFT_WMAX], wj[NUFFT_WMAX];
#pragma unroll
        for (int a = 0; a < NUFFT_WMAX; ++a) {
            wi[a] = a < W ? v * es_kernel((double)(i0 + a) - x, inv_hw, beta) : 0.0;
            wj[a] = a < W ? es_kernel((double)(j0 + a) - y, inv_hw, beta) : 0.0;
        }
        int jj[NUFFT_WMAX];
#pragma unroll
        for (int b = 0; b < NUFFT_WMAX; ++b) jj[b] = (int)(((j0 + b) % n1 + n1) % n1);
#pragma unroll
        for (int a = 0; a < NUFFT_WMAX; ++a) {
            double *row = grid + (((i0 + a) % n1 + n1) % n1) * (long long)n1;
#pragma unroll
            for (int b = 0; b < NUFFT_WMAX; ++b)
                if (a < W && b < W) unsafeAtomicAdd(row + jj[b], wi[a] * wj[b]);
        }
    }
}

// ---- spreading through LDS tiles (large catalogues) ----------------------------------------------------------------
// The support of a point is the W x W block of cells whose lower corner is (i0, j0) = (ceil(x - W/2), ceil(y - W/2)).  Tile
// (ti, tj) = ((i0 + 16) / 64, (j0 + 16) / 64) owns the points whose corner lies in its 64 x 64 cells; their supports fit a
// (64 + 15)^2 window that the work-group accumulates in LDS (hardware LDS atomics) and adds to the grid once
// ((64 + 15)^2 = 6241 global atomics per occupied tile instead of W^2 per point).  Points are brought into tile order by
// one radix sort of (tile, point index) per call -- the order is shared by all components.
constexpr int NUFFT_TS = 64, NUFFT_TPAD = 16, NUFFT_TW = NUFFT_TS + NUFFT_WMAX - 1, NUFFT_TLD = NUFFT_TS + NUFFT_WMAX;

__device__ inline bool nufft_corner(const double2 tp, int n1, int W, double &x, double &y, long long &i0, long long &j0)
{
    if (!(tp.x >= 0.0 && tp.x <= M_PI) || !isfinite(tp.y)) return false;
    const double sc = (double)n1 / (2.0 * M_PI), hw = 0.5 * W;
    x = tp.x * sc;
    double ph = fmod(tp.y, 2.0 * M_PI);
    if (ph < 0.0) ph += 2.0 * M_PI;
    y = ph * sc;
    i0 = (long long)ceil(x - hw);
    j0 = (long long)ceil(y - hw);
    return true;
}

__global__ __launch_bounds__(256) void k_nufft_keys(long long npts, const double2 *__restrict__ loc, int n1, int W, int ntx,
                                                    unsigned *__restrict__ key, unsigned *__restrict__ idx,
                                                    unsigned long long *__restrict__ nbad)
{
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npts; p += (long long)gridDim.x * blockDim.x) {
        double x, y;
        long long i0, j0;
        unsigned k = 0xffffffffu;  // invalid points sort behind every tile
        if (nufft_corner(loc[p], n1, W, x, y, i0, j0)) k = (unsigned)((i0 + NUFFT_TPAD) / NUFFT_TS) * (unsigned)ntx + (unsigned)((j0 + NUFFT_TPAD) / NUFFT_TS);
        else atomicAdd(nbad, 1ULL);
        key[p] = k;
        idx[p] = (unsigned)p;
    }
}

__global__ __launch_bounds__(256) void k_nufft_spread_tiles(long long npts, const double2 *__restrict__ loc,
                                                            const double *__restrict__ val, const unsigned *__restrict__ key,
                                                            const unsigned *__restrict__ idx, double *__restrict__ grid, int n1,
                                                            int W, double beta, int ntx, unsigned long long *__restrict__ nbad)
{
    __shared__ double tile[NUFFT_TW * NUFFT_TLD];
    __shared__ long long seg[2];
    const unsigned me = blockIdx.x;
    if (threadIdx.x < 2) {  // first sorted position with key >= me (+ 1)
        const unsigned want = me + threadIdx.x;
        long long lo = 0, hi = npts;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (key[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        seg[threadIdx.x] = lo;
    }
    __syncthreads();
    const long long p0 = seg[0], p1 = seg[1];
    if (p0 == p1) return;
    for (int c = threadIdx.x; c < NUFFT_TW * NUFFT_TLD; c += blockDim.x) tile[c] = 0.0;
    __syncthreads();
    const long long ti0 = (long long)(me / ntx) * NUFFT_TS - NUFFT_TPAD, tj0 = (long long)(me % ntx) * NUFFT_TS - NUFFT_TPAD;
    const double inv_hw = 2.0 / W;
    for (long long q = p0 + threadIdx.x; q < p1; q += blockDim.x) {
        const unsigned p = idx[q];
        const double v = val[p];
        if (!isfinite(v)) {
            atomicAdd(nbad, 1ULL);
            continue;
        }
        if (v == 0.0) continue;
        double x, y;
        long long i0, j0;
        nufft_corner(loc[p], n1, W, x, y, i0, j0);
        double wj[NUFFT_WMAX];
#pragma unroll
        for (int b = 0; b < NUFFT_WMAX; ++b) wj[b] = b < W ? es_kernel((double)(j0 + b) - y, inv_hw, beta) : 0.0;
        double *base = tile + (i0 - ti0) * NUFFT_TLD + (j0 - tj0);
        for (int a = 0; a < W; ++a) {
            const double wa = v * es_kernel((double)(i0 + a) - x, inv_hw, beta);
#pragma unroll
            for (int b = 0; b < NUFFT_WMAX; ++b)
                if (b < W) atomicAdd(base + a * NUFFT_TLD + b, wa * wj[b]);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < NUFFT_TW * NUFFT_TW; c += blockDim.x) {
        const int r = c / NUFFT_TW, cc = c % NUFFT_TW;
        const double v = tile[r * NUFFT_TLD + cc];
        if (v != 0.0) unsafeAtomicAdd(grid + (((ti0 + r) % n1 + n1) % n1) * (long long)n1 + (((tj0 + cc) % n1 + n1) % n1), v);
    }
}

struct NufftFft {
    const double *src_real;   // MODE 0: grid
    const double2 *src;       // MODE 1: T, MODE 2: U
    double2 *dst;             // MODE 0: T, MODE 1: U, MODE 2: h
    const double *dec;        // MODE 0: 1 / psi^(m)
    const double2 *fac;       // MODE 1: exp(i pi k / N) / psi^(k), index k + lmax
    const double2 *tw;
    int n, lmax, N, n1, row0, twN;
};

__device__ inline double2 rot4(double2 x, int k)  // x * (-i)^k
{
    switch (k & 3) {
    case 0: return x;
    case 1: return mul_mi(x);
    case 2: return mk(-x.x, -x.y);
    default: return mul_pi(x);
    }
}

// One work-group per row.  Length n = R ns with ns <= 8192 in LDS: X[R k + r] = FFT_ns( (sum_q x[j + q ns] w_R^{q r}) w_n^{j r} )[k].
// MODE 0: real row (row0 + blockIdx.x) mod n1 of the grid -> T[m][row] = X[m] dec[m], m <= lmax
// MODE 1: row m of T -> U[m][k mod N] = X[k mod n1] fac[k], |k| <= lmax
// MODE 2: row m of U, inverse transform -> h[m][j]
template <int MODE>
__global__ __launch_bounds__(512) void k_nufft_fft(NufftFft a)
{
    extern __shared__ double2 buf[];
    __shared__ double2 tw_hi[TW_HI_MAX], tw_lo[64];
    const TwFactored twf = load_tw_factored(tw_hi, tw_lo, a.tw, a.twN);
    const int n = a.n;
    const int R = n > NUFFT_LDS_MAX ? n / NUFFT_LDS_MAX : 1, ns = n / R, p = ilog2(ns);
    const int row = MODE == 0 ? (a.row0 + (int)blockIdx.x) % a.n1 : (int)blockIdx.x;
    const double *xr = MODE == 0 ? a.src_real + (long long)row * n : nullptr;
    const double2 *xc = MODE == 0 ? nullptr : a.src + (long long)row * n;
    for (int r = 0; r < R; ++r) {
        __syncthreads();  // twiddle tables written / previous sub-transform read out
        for (int j = threadIdx.x; j < ns; j += blockDim.x) {
            double2 t = mk(0.0, 0.0);
            for (int q = 0; q < R; ++q) {
                double2 x;
                if (MODE == 0) x = mk(xr[j + q * ns], 0.0);
                else if (MODE == 1) x = xc[j + q * ns];
                else x = cconj(xc[j + q * ns]);
                t = cadd(t, rot4(x, (4 / R) * q * r));
            }
            if (r && j) t = cmul(t, expipi(-2.0 * (double)(((long long)j * r) % n) / (double)n));
            buf[lds_slot(j)] = t;
        }
        __syncthreads();
        lds_fft_dif(buf, ns, twf, a.twN);
        for (int k = threadIdx.x; k < ns; k += blockDim.x) {
            const int idx = R * k + r;
            const double2 v = buf[lds_slot(bitrev(k, p))];
            if (MODE == 0) {
                if (idx <= a.lmax) a.dst[(long long)idx * a.n1 + row] = cscale(v, a.dec[idx]);
            } else if (MODE == 1) {
                int kk;
                if (idx <= a.lmax) kk = idx;
                else if (idx >= n - a.lmax) kk = idx - n;
                else continue;
                a.dst[(long long)row * a.N + ((kk + a.N) % a.N)] = cmul(v, a.fac[kk + a.lmax]);
            } else {
                a.dst[(long long)row * a.N + idx] = cconj(v);
            }
        }
    }
}

// ---- the forward direction: alm -> values at the points (ducc0's synthesis_general) -----------------------------------------------
//     v_p = Re sum_m c_m F_m(theta_p) exp(i m phi_p),   F_m(theta) = sum_l a_lm lambda_lm(theta),   c_0 = 1, c_m = 2,
// is the transpose of the chain above, stage by stage (a type-2 non-uniform FFT):
//   0. the Legendre synthesis sweeps of alm2map (hx_legendre_valu.hip) on the equiangular plan: ring modes Fv[m][ring pair] = F_m at
//      theta_r (N) and pi - theta_r (S); ring j = r is N, ring j = N/2 - 1 - r is S, and F_m(theta_{N-1-j}) = (-1)^(m+s) F_m(theta_j)
//      continues them to the full circle (the transpose of the fold in ring_modes_ns, hx_sht_common.h);
//   1. F_m is a trigonometric polynomial of degree <= lmax and N > 2 lmax, so ONE forward FFT of length N gives its coefficients
//      exactly: f(k, m) = (1/N) sum_j F_m(theta_j) exp(-i k theta_j) = X[k mod N] exp(-i pi k / N) / N; divided by psi^(k):
//      U[m][k mod N] = X[k mod N] conj(fac[k]) / N;
//   2. zero-padded inverse FFT of length n1: T[m][a] = sum_k U[m][k] exp(2 pi i k a / n1), kept for the band of rows a point reads;
//   3. per band row, inverse FFT of length n1 over m with c_m dec[m], real part: the grid row g[a][.];
//   4. gather: v_p = sum_{a, b < W} psi(i0 + a - x_p) psi(j0 + b - y_p) g[i0 + a][j0 + b], corner (i0, j0) of nufft_corner.
// Nothing is added to memory that another thread adds to: a call's result is bit-identical from run to run.
// n1 is a power of two (2 N, N = 16 * 2^k): indices wrap with a mask here.
struct NufftSyn {
    const double *Fv;       // MODE 0: ring modes [m][nrp_pad][nv], component c = (N_re, N_im, S_re, S_im) at 4 c
    const double2 *src;     // MODE 1: U, MODE 2: T
    double2 *dst;           // MODE 0: U, MODE 1: T
    double *grid;           // MODE 2
    const double *dec;      // MODE 2: 1 / psi^(m)
    const double2 *fac;     // MODE 0: exp(i pi k / N) / psi^(k), index k + lmax
    const double2 *tw;
    long long mstride;      // MODE 0: doubles between two orders of Fv
    int nv, comp4, parity;  // MODE 0: doubles per ring pair, 4 c, spin weight & 1
    int n, lmax, N, n1, row0, band, twN;
};

// One work-group per row, the R x 8192 split of k_nufft_fft.  Inverse transforms: conjugate in, conjugate out.
// MODE 0: ring modes of order m = blockIdx.x, continued to N rings -> U[m][k mod N], |k| <= lmax
// MODE 1: row m of U, zero-padded to n1, inverse -> T[m][a], a in the band
// MODE 2: band row a = (row0 + blockIdx.x) mod n1: c_m dec[m] T[m][a], zero beyond lmax, inverse, real part -> grid[a][.]
template <int MODE>
__global__ __launch_bounds__(512) void k_nufft_fft_syn(NufftSyn a)
{
    extern __shared__ double2 buf[];
    __shared__ double2 tw_hi[TW_HI_MAX], tw_lo[64];
    const TwFactored twf = load_tw_factored(tw_hi, tw_lo, a.tw, a.twN);
    const int n = a.n;
    const int R = n > NUFFT_LDS_MAX ? n / NUFFT_LDS_MAX : 1, ns = n / R, p = ilog2(ns);
    const int row = MODE == 2 ? (a.row0 + (int)blockIdx.x) & (a.n1 - 1) : (int)blockIdx.x;
    auto input = [&](int e) -> double2 {
        if (MODE == 0) {
            const bool second = 2 * e >= a.N;          // theta_e = 2 pi - theta_j
            const int j = second ? a.N - 1 - e : e;
            const bool south = 4 * j >= a.N;           // theta_j = pi - theta_rp
            const int rp = south ? a.N / 2 - 1 - j : j;
            const double2 v = reinterpret_cast<const double2 *>(a.Fv + (long long)row * a.mstride + (long long)rp * a.nv + a.comp4)[south ? 1 : 0];
            return (second && ((row + a.parity) & 1)) ? mk(-v.x, -v.y) : v;
        } else if (MODE == 1) {
            if (e <= a.lmax) return cconj(a.src[(long long)row * a.N + e]);
            if (e >= n - a.lmax) return cconj(a.src[(long long)row * a.N + (e - n + a.N)]);
            return mk(0.0, 0.0);
        } else {
            if (e > a.lmax) return mk(0.0, 0.0);
            return cconj(cscale(a.src[(long long)e * a.n1 + row], (e ? 2.0 : 1.0) * a.dec[e]));
        }
    };
    for (int r = 0; r < R; ++r) {
        __syncthreads();  // twiddle tables written / previous sub-transform read out
        for (int j = threadIdx.x; j < ns; j += blockDim.x) {
            double2 t = mk(0.0, 0.0);
            for (int q = 0; q < R; ++q) t = cadd(t, rot4(input(j + q * ns), (4 / R) * q * r));
            if (r && j) t = cmul(t, expipi(-2.0 * (double)(((long long)j * r) % n) / (double)n));
            buf[lds_slot(j)] = t;
        }
        __syncthreads();
        lds_fft_dif(buf, ns, twf, a.twN);
        for (int k = threadIdx.x; k < ns; k += blockDim.x) {
            const int idx = R * k + r;
            const double2 v = buf[lds_slot(bitrev(k, p))];
            if (MODE == 0) {
                int kk;
                if (idx <= a.lmax) kk = idx;
                else if (idx >= n - a.lmax) kk = idx - n;
                else continue;
                a.dst[(long long)row * a.N + idx] = cscale(cmul(v, cconj(a.fac[kk + a.lmax])), 1.0 / a.N);
            } else if (MODE == 1) {
                if (((idx - a.row0) & (a.n1 - 1)) < a.band) a.dst[(long long)row * a.n1 + idx] = cconj(v);
            } else {
                a.grid[(long long)row * a.n1 + idx] = v.x;
            }
        }
    }
}

// One thread per point: 2 W kernel values, W x W reads of the grid.  A point outside the sphere is counted and reads NaN.
__global__ __launch_bounds__(256) void k_nufft_gather(long long npts, const double2 *__restrict__ loc, const double *__restrict__ grid,
                                                      double *__restrict__ val, int n1, int W, double beta,
                                                      unsigned long long *__restrict__ nbad)
{
    const double inv_hw = 2.0 / W;
    const int mask = n1 - 1;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npts; p += (long long)gridDim.x * blockDim.x) {
        double x, y;
        long long i0, j0;
        if (!nufft_corner(loc[p], n1, W, x, y, i0, j0)) {
            atomicAdd(nbad, 1ULL);
            val[p] = __builtin_nan("");
            continue;
        }
        double wj[NUFFT_WMAX];
        int jj[NUFFT_WMAX];
#pragma unroll
        for (int b = 0; b < NUFFT_WMAX; ++b) {
            wj[b] = b < W ? es_kernel((double)(j0 + b) - y, inv_hw, beta) : 0.0;
            jj[b] = (int)(j0 + b) & mask;
        }
        double s = 0.0;
        for (int a = 0; a < W; ++a) {
            const double wa = es_kernel((double)(i0 + a) - x, inv_hw, beta);
            const double *row = grid + (long long)((int)(i0 + a) & mask) * n1;
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < NUFFT_WMAX; ++b)
                if (b < W) t = fma(wj[b], row[jj[b]], t);
            s = fma(wa, t, s);
        }
        val[p] = s;
    }
}

// Points in the tile order of pointsht_order (the keys and the sort of the spread): one work-group per occupied 64 x 64 tile loads the
// (64 + 15)-row window its points read into LDS with coalesced row reads (50 KB) and gathers from there; block `ntiles` writes NaN for
// the invalid points, which sort behind every tile (k_nufft_keys has counted them).  A tile of at most NUFFT_TSPARSE points skips the
// window (10^6 points at lmax 6144 are 8 per tile: loading 131 000 windows took 5.2 ms where one thread per point takes 2.1).  All
// three ways form the same sums in the same order: a point's value does not depend on the path or on its neighbours.
constexpr int NUFFT_TSPARSE = 256 / NUFFT_WMAX;  // one (point, window row) per thread of the group
__global__ __launch_bounds__(256) void k_nufft_gather_tiles(long long npts, const double2 *__restrict__ loc, const unsigned *__restrict__ key,
                                                            const unsigned *__restrict__ idx, const double *__restrict__ grid,
                                                            double *__restrict__ val, int n1, int W, double beta, int ntx, unsigned ntiles)
{
    __shared__ double tile[NUFFT_TW * NUFFT_TLD];
    __shared__ long long seg[2];
    const unsigned me = blockIdx.x;
    const bool bad = me == ntiles;
    if (threadIdx.x < 2) {  // first sorted position with key >= me (+ 1)
        const unsigned want = bad ? 0xffffffffu : me + threadIdx.x;
        long long lo = 0, hi = npts;
        if (bad && threadIdx.x) lo = npts;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (key[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        seg[threadIdx.x] = lo;
    }
    __syncthreads();
    const long long p0 = seg[0], p1 = seg[1];
    if (p0 == p1) return;
    if (bad) {
        for (long long q = p0 + threadIdx.x; q < p1; q += blockDim.x) val[idx[q]] = __builtin_nan("");
        return;
    }
    const int mask = n1 - 1;
    const int ti0 = (int)(me / ntx) * NUFFT_TS - NUFFT_TPAD, tj0 = (int)(me % ntx) * NUFFT_TS - NUFFT_TPAD;
    const double inv_hw = 2.0 / W;
    if (p1 - p0 <= NUFFT_TSPARSE) {
        // a sparse tile reads the grid itself, W^2 cells per point against the 79 x 79 of the window: thread (point q, c) of the 16 x 16
        // forms the kernel values psi(j0 + c - y), psi(i0 + c - x) once, then the sum of window row c, and thread (q, 0) adds the rows
        double *wjs = tile, *was = tile + NUFFT_TSPARSE * NUFFT_WMAX, *ts = tile + 2 * NUFFT_TSPARSE * NUFFT_WMAX;
        const int q = threadIdx.x / NUFFT_WMAX, c = threadIdx.x % NUFFT_WMAX, o = q * NUFFT_WMAX;
        const bool live = q < (int)(p1 - p0);
        const unsigned p = live ? idx[p0 + q] : 0u;
        double x = 0.0, y = 0.0;
        long long i0 = 0, j0 = 0;
        if (live) {
            nufft_corner(loc[p], n1, W, x, y, i0, j0);
            wjs[o + c] = c < W ? es_kernel((double)(j0 + c) - y, inv_hw, beta) : 0.0;
            was[o + c] = c < W ? es_kernel((double)(i0 + c) - x, inv_hw, beta) : 0.0;
        }
        __syncthreads();
        if (live && c < W) {
            const double *row = grid + (long long)((int)(i0 + c) & mask) * n1;
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < NUFFT_WMAX; ++b)
                if (b < W) t = fma(wjs[o + b], row[(int)(j0 + b) & mask], t);
            ts[o + c] = t;
        }
        __syncthreads();
        if (live && c == 0) {
            double s = 0.0;
            for (int a = 0; a < W; ++a) s = fma(was[o + a], ts[o + a], s);
            val[p] = s;
        }
        return;
    }
    for (int c = threadIdx.x; c < NUFFT_TW * NUFFT_TLD; c += blockDim.x) {
        const int r = c / NUFFT_TLD, cc = c % NUFFT_TLD;
        tile[c] = cc < NUFFT_TW ? grid[(long long)((ti0 + r) & mask) * n1 + ((tj0 + cc) & mask)] : 0.0;
    }
    __syncthreads();
    for (long long q = p0 + threadIdx.x; q < p1; q += blockDim.x) {
        const unsigned p = idx[q];
        double x, y;
        long long i0, j0;
        nufft_corner(loc[p], n1, W, x, y, i0, j0);
        double wj[NUFFT_WMAX];
#pragma unroll
        for (int b = 0; b < NUFFT_WMAX; ++b) wj[b] = b < W ? es_kernel((double)(j0 + b) - y, inv_hw, beta) : 0.0;
        const double *base = tile + ((int)i0 - ti0) * NUFFT_TLD + ((int)j0 - tj0);
        double s = 0.0;
        for (int a = 0; a < W; ++a) {  // (the same sums in the same order on both branches, and in k_nufft_gather)
            const double wa = es_kernel((double)(i0 + a) - x, inv_hw, beta);
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < NUFFT_WMAX; ++b)
                if (b < W) t = fma(wj[b], base[a * NUFFT_TLD + b], t);
            s = fma(wa, t, s);
        }
        val[p] = s;
    }
}

// ---- ring modes next to the poles ------------------------------------------------------------------------------------------------------
// The Legendre sweeps run their three-term recursion through x = cos(theta) in float64.  On a ring next to a pole that x fixes theta to
// 1.1e-16 / sin(theta) only, and the error is the same at every l: l * 1.1e-16 / sin(theta_ring) of a value, 4e-11 of the largest value
// at lmax 4200 (theta_0 = pi / N = 1.9e-4) for a point that lies among those rings.  The adjoint lives with it (its tests give such points a
// wider bound); here the modes of the NUFFT_POLAR_K ring pairs next to the poles are formed again from Wigner-d tables built in
// double-double at the nodes x + xlo (wigner_table_build, hx_wigner.hip: the tables of the mixing matrices), for the orders m <=
// NUFFT_POLAR_M, and overwrite what the sweep left:
//     (+-s)lambda_lm(theta) = (-1)^m N_l d^l_{m,-+s}(theta),  N_l = sqrt((2l+1)/4pi)     (s = 0: lambda_lm = (-1)^m N_l d^l_{m0}),
//     P+ = -(-1)^m sum_l N_l d^l_{m,-s} (E + iB),  P- = -(-1)^(m+s) sum_l N_l d^l_{m,+s} (E - iB),  Q = (P+ + P-) / 2,  U = (P+ - P-) / 2i,
// with the tables' d^l_{ab} (seed d^A_{AB} > 0 for A >= |B|: (-1)^(a-b) times the d^j_{m'm} of the textbooks) and the convention of the
// sweeps for (E, B) -> (Q, U) (tests/spin_synthesis_reference.py writes it out).  Ring pair r >= K carries at most 1 / (2K + 1) of the
// first ring's error; on these rings l theta <= pi (K - 1/2) = 23.6 (N > 2 lmax), where an order beyond 48 is below 2e-10 of the largest
// value (lambda_lm ~ J_m(l theta) <= (l theta / 2)^m / m!), and the sweep's relative error of 1e-9 of that is nothing.  The table of a weight is built when the weight is first
// used: 2 (M + 1) (lmax + 1) 2K doubles, 71 MB at lmax 6144.  One wave per (order, ring, map / field): lane j adds the l = l0 + j mod 64,
// the lanes are added in a fixed order.
// Weights beyond NUFFT_POLAR_SMAX keep the sweep's modes: the seeds of those tables take a binomial the host forms in 128 bits.
constexpr int NUFFT_POLAR_K = 8, NUFFT_POLAR_M = 48, NUFFT_POLAR_SMAX = 56;
struct PolarModes {
    const double *tab;    // [m][1 or 2][lmax + 1][2K]: d^l_{m,-s}, then (s > 0) d^l_{m,+s}, at the nodes k < K north, K + r south
    const double2 *alm;   // first component of the sweep
    double *Fv;
    long long nlm, mstride;
    int lmax, s, K, nv;
};
__global__ __launch_bounds__(64) void k_polar_modes(PolarModes a)
{
    const int m = blockIdx.x, k = blockIdx.y, u = blockIdx.z, lane = threadIdx.x;
    const int s = a.s, n2 = 2 * a.K, l0 = max(m, s);
    const long long cb = (long long)m * (2 * a.lmax + 1 - m) / 2, tsize = (long long)(a.lmax + 1) * n2;
    const double *tp = a.tab + (long long)m * (s ? 2 : 1) * tsize + k, *tm = tp + tsize;
    const double2 *E = a.alm + (long long)(s ? 2 * u : u) * a.nlm + cb, *B = E + a.nlm;
    double pr = 0.0, pi = 0.0, mr = 0.0, mi = 0.0;
    for (int l = l0 + lane; l <= a.lmax; l += 64) {
        const double nl = sqrt((2.0 * l + 1.0) * (0.25 / M_PI));
        const double2 e = E[l];
        if (s == 0) {
            const double d = nl * tp[(long long)l * n2];
            pr = fma(d, e.x, pr);
            pi = fma(d, e.y, pi);
        } else {
            const double2 b = B[l];
            const double dp = nl * tp[(long long)l * n2], dm = nl * tm[(long long)l * n2];
            pr = fma(dp, e.x - b.y, pr);  // E + iB
            pi = fma(dp, e.y + b.x, pi);
            mr = fma(dm, e.x + b.y, mr);  // E - iB
            mi = fma(dm, e.y - b.x, mi);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        pr += __shfl_xor(pr, o);
        pi += __shfl_xor(pi, o);
        mr += __shfl_xor(mr, o);
        mi += __shfl_xor(mi, o);
    }
    if (lane) return;
    const bool south = k >= a.K;
    double *row = a.Fv + (long long)m * a.mstride + (long long)(south ? k - a.K : k) * a.nv + (south ? 2 : 0);
    const double sgm = (m & 1) ? -1.0 : 1.0;
    if (s == 0) {
        row[4 * u] = sgm * pr;
        row[4 * u + 1] = sgm * pi;
        return;
    }
    const double sgs = (s & 1) ? sgm : -sgm;  // -(-1)^(m + s)
    const double ppr = -sgm * pr, ppi = -sgm * pi, pmr = sgs * mr, pmi = sgs * mi;
    row[8 * u] = 0.5 * (ppr + pmr);
    row[8 * u + 1] = 0.5 * (ppi + pmi);
    row[8 * u + 4] = 0.5 * (ppi - pmi);
    row[8 * u + 5] = -0.5 * (ppr - pmr);
}

// Gauss-Legendre nodes on [-1, 1] (host, Newton on P_n)
static void gl_nodes(int n, std::vector<double> &x, std::vector<double> &w)
{
    x.resize(n); w.resize(n);
    for (int i = 0; i < (n + 1) / 2; ++i) {
        long double z = cosl(3.141592653589793238462643383279502884L * (i + 0.75L) / (n + 0.5L)), pp = 0.0L;
        for (int it = 0; it < 100; ++it) {
            long double p1 = 1.0L, p2 = 0.0L;
            for (int j = 1; j <= n; ++j) {
                const long double p3 = p2;
                p2 = p1;
                p1 = ((2.0L * j - 1.0L) * z * p2 - (j - 1.0L) * p3) / j;
            }
            pp = n * (z * p1 - p2) / (z * z - 1.0L);
            const long double dz = p1 / pp;
            z -= dz;
            if (fabsl(dz) < 1e-19L) break;
        }
        x[i] = (double)-z; x[n - 1 - i] = (double)z;
        w[i] = w[n - 1 - i] = (double)(2.0L / ((1.0L - z * z) * pp * pp));
    }
}

}  // namespace hx

extern "C" hx_pointsht *hx_pointsht_create(int lmax, double epsilon)
{
    if (ensure_ready() != HX_OK) return nullptr;
    if (lmax < 0 || lmax > 8191 || !(epsilon > 0.0) || !(epsilon < 1.0)) {
        set_error("hx_pointsht_create: lmax in [0, 8191] and 0 < epsilon < 1");
        return nullptr;
    }
    hx_pointsht *ps = new hx_pointsht;
    ps->lmax = lmax;
    ps->epsilon = epsilon;
    int N = 16;
    while (N < 2 * lmax + 2) N *= 2;
    ps->N = N;
    ps->n1 = 2 * N;
    ps->W = std::max(4, std::min(NUFFT_WMAX, (int)ceil(-log10(epsilon)) + 3));
    ps->beta = 2.30 * ps->W;
    ps->twN = std::min(ps->n1, NUFFT_LDS_MAX);
    ps->eq = plan_create_equiangular(N, lmax);
    if (!ps->eq) { delete ps; return nullptr; }
    // psi^(k) = int psi(u) cos(k h u) du, h = 2 pi / n1, by Gauss-Legendre quadrature (the integrand is smooth; 2 W + 32 nodes)
    std::vector<double> xg, wg;
    gl_nodes(2 * ps->W + 32, xg, wg);
    const double hgrid = 2.0 * M_PI / ps->n1, hw = 0.5 * ps->W;
    auto khat = [&](int k) {
        long double s = 0.0L;
        for (size_t i = 0; i < xg.size(); ++i) s += (long double)(wg[i] * hw * es_kernel(xg[i] * hw, 1.0 / hw, ps->beta)) * cosl((long double)k * hgrid * xg[i] * hw);
        return (double)s;
    };
    std::vector<double> dec(lmax + 1);
    std::vector<double2> fac(2 * lmax + 1), tw(std::max(ps->twN / 2, 64));
    for (int m = 0; m <= lmax; ++m) dec[m] = 1.0 / khat(m);
    for (int k = -lmax; k <= lmax; ++k) {
        const double f = dec[k < 0 ? -k : k], ang = M_PI * k / N;
        fac[k + lmax].x = f * cos(ang); fac[k + lmax].y = f * sin(ang);
    }
    for (int k = 0; k < (int)tw.size(); ++k) {
        const long double ang = -2.0L * 3.141592653589793238462643383279502884L * k / ps->twN;
        tw[k].x = (double)cosl(ang); tw[k].y = (double)sinl(ang);
    }
    if (upload(ps->dec_phi, dec) != HX_OK || upload(ps->fac_theta, fac) != HX_OK || upload(ps->tw, tw) != HX_OK || ps->nbad.alloc(8) != HX_OK) {
        hx_plan_destroy(ps->eq);
        delete ps;
        return nullptr;
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_nufft_fft<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_nufft_fft<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_nufft_fft<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_nufft_fft_syn<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_nufft_fft_syn<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_nufft_fft_syn<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    return ps;
}

extern "C" void hx_pointsht_destroy(hx_pointsht *ps)
{
    if (!ps) return;
    if (rt().ready) (void)hipStreamSynchronize(rt().stream);
    if (ps->eq) hx_plan_destroy(ps->eq);
    delete ps;
}

extern "C" int hx_pointsht_info(const hx_pointsht *ps, int *info4)
{
    if (!ps || !info4) return fail(HX_ERR_ARG, "hx_pointsht_info: null argument");
    info4[0] = ps->lmax; info4[1] = ps->N; info4[2] = ps->n1; info4[3] = ps->W;
    return HX_OK;
}

namespace hx {

// ---- the two halves of the transform (hx_common.h) -------------------------------------------------------------------
// Half one: points -> grid.  pointsht_order decides the spreading path for n points and, for the tile path, sorts them once (the order is
// shared by every component spread from these points); pointsht_spread_one ADDS one component to a grid (no memset: a caller that
// keeps the grid resident accumulates page after page -- spreading is additive in the points).
int pointsht_order(hx_pointsht *ps, int64_t npoints, const double2 *loc, PointOrder *o)
{
    const int n1 = ps->n1, W = ps->W;
    hipStream_t st = rt().stream;
    // large catalogues are spread through LDS tiles (one sort per call); HX_NUFFT_TILES = 0 / 1 forces the choice
    bool tiles = npoints >= 300000;  // measured cross-over at lmax 6144 (tools/time_pointsht.py)
    if (const char *e = getenv("HX_NUFFT_TILES")) tiles = atoi(e) != 0;
    if (npoints == 0 || npoints > 0xfffffff0ll) tiles = false;
    o->tiles = tiles;
    o->key = o->idx = nullptr;
    if (!tiles) return HX_OK;
    const int ntx = n1 / NUFFT_TS + 1;
    ProfScope pf("nufft_sort");
    HX_TRY(ps->key.alloc(sizeof(unsigned) * (size_t)npoints));
    HX_TRY(ps->key2.alloc(sizeof(unsigned) * (size_t)npoints));
    HX_TRY(ps->idx.alloc(sizeof(unsigned) * (size_t)npoints));
    HX_TRY(ps->idx2.alloc(sizeof(unsigned) * (size_t)npoints));
    const long long nblk = std::min<long long>((npoints + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(k_nufft_keys, dim3((unsigned)nblk), dim3(256), 0, st, (long long)npoints, loc, n1, W, ntx,
                       ps->key.as<unsigned>(), ps->idx.as<unsigned>(), ps->nbad.as<unsigned long long>());
    // all 32 bits: invalid points carry the key 0xffffffff
    HX_TRY(rsort::radix_sort_pairs<unsigned>(ps->key.as<unsigned>(), ps->idx.as<unsigned>(), ps->key2.as<unsigned>(), ps->idx2.as<unsigned>(),
                                             (unsigned long long)npoints, 32, ps->sort_tmp, st, &o->key, &o->idx));
    return HX_OK;
}

int pointsht_spread_one(hx_pointsht *ps, const PointOrder &o, int64_t npoints, const double2 *loc, const double *val, double *grid)
{
    const int n1 = ps->n1, W = ps->W;
    hipStream_t st = rt().stream;
    if (o.tiles) {
        const int ntx = n1 / NUFFT_TS + 1, nty = (n1 / 2 + W + NUFFT_TPAD) / NUFFT_TS + 1;
        hipLaunchKernelGGL(k_nufft_spread_tiles, dim3((unsigned)(ntx * nty)), dim3(256), 0, st, (long long)npoints, loc, val, o.key, o.idx,
                           grid, n1, W, ps->beta, ntx, ps->nbad.as<unsigned long long>());
    } else if (npoints > 0) {
        const long long nblk = std::min<long long>((npoints + 255) / 256, 1 << 20);
        hipLaunchKernelGGL(k_nufft_spread, dim3((unsigned)nblk), dim3(256), 0, st, (long long)npoints, loc, val, grid, n1, W, ps->beta,
                           ps->nbad.as<unsigned long long>());
    }
    HX_HIP(hipGetLastError());
    return HX_OK;
}

// Half two: grids -> alm.  Component c's grid comes from grid_of(c) right before its three FFT stages (a caller with one grid refills it
// there); the ring spectra of a batch then go through the Legendre analysis.  d_alm: [ncomp][nlm] on the device.
int pointsht_grids_to_alm(hx_pointsht *ps, int spin, int ncomp, const GridOf &grid_of, double2 *d_alm)
{
    hx_plan *eq = ps->eq;
    const int lmax = ps->lmax, N = ps->N, n1 = ps->n1, W = ps->W;
    hipStream_t st = rt().stream;
    const size_t hrow = (size_t)(lmax + 1) * N;
    HX_TRY(ps->T.alloc(sizeof(double2) * (size_t)(lmax + 1) * n1));
    HX_TRY(ps->U.alloc(sizeof(double2) * hrow));
    const bool generic = analysis_generic_spin(spin);  // a spin weight other than 0 and 2: one field per Legendre sweep
    const int maxb = generic ? 2 : analysis_max_comp(spin);
    HX_TRY(ps->h.alloc(sizeof(double2) * hrow * std::min(ncomp, maxb)));
    NufftFft a;
    a.dec = ps->dec_phi.as<double>(); a.fac = ps->fac_theta.as<double2>(); a.tw = ps->tw.as<double2>();
    a.lmax = lmax; a.N = N; a.n1 = n1; a.twN = ps->twN;
    const int band = std::min(n1, n1 / 2 + W + 4);  // rows a point with 0 <= theta <= pi can touch
    a.row0 = (n1 - W / 2 - 2) % n1;
    auto launch = [&](int mode, int n, int rows) {
        const int ns = std::min(n, NUFFT_LDS_MAX), threads = std::min(512, std::max(64, ns / 16));  // one radix-16 butterfly per thread and pass
        a.n = n;
        const size_t lds = (size_t)lds_fft_slots(ns) * sizeof(double2);
        if (mode == 0) hipLaunchKernelGGL(k_nufft_fft<0>, dim3(rows), dim3(threads), lds, st, a);
        else if (mode == 1) hipLaunchKernelGGL(k_nufft_fft<1>, dim3(rows), dim3(threads), lds, st, a);
        else hipLaunchKernelGGL(k_nufft_fft<2>, dim3(rows), dim3(threads), lds, st, a);
    };
    for (int c0 = 0, nb = 0; c0 < ncomp; c0 += nb) {
        nb = generic ? std::min(2, ncomp - c0) : analysis_next_batch(spin, ncomp - c0);
        if (nb <= 0) return fail(HX_ERR_ARG, "point transform: %d components of spin %d", ncomp, spin);
        for (int c = 0; c < nb; ++c) {
            const double *grid = nullptr;
            HX_TRY(grid_of(c0 + c, &grid));
            ProfScope pf("nufft_fft");
            HX_HIP(hipMemsetAsync(ps->T.p, 0, sizeof(double2) * (size_t)(lmax + 1) * n1, st));
            HX_HIP(hipMemsetAsync(ps->U.p, 0, sizeof(double2) * hrow, st));
            a.src_real = grid;
            a.dst = ps->T.as<double2>();
            launch(0, n1, band);
            a.src = ps->T.as<double2>(); a.dst = ps->U.as<double2>();
            launch(1, n1, lmax + 1);
            a.src = ps->U.as<double2>(); a.dst = ps->h.as<double2>() + hrow * c;
            launch(2, N, lmax + 1);
            HX_HIP(hipGetLastError());
        }
        eq->hsrc = ps->h.as<double2>();
        eq->hsrc_stride = (long long)hrow;
        const int rc = analysis_batch(eq, spin, nb, nullptr, d_alm + (size_t)c0 * eq->nlm, nullptr, nullptr, nullptr, 0);
        eq->hsrc = nullptr;
        HX_TRY(rc);
    }
    return HX_OK;
}

// ---- the forward direction: its two halves (hx_common.h) ------------------------------------------------------------------------------
// Half one: alm -> grids.  One sweep of the vector-unit synthesis per four maps / two spin-2 fields / one field of any other weight
// (the sweeps of alm2map, on the equiangular plan; their ring modes live in the plan's operand buffer F, idle here as there), then per
// component the three transposed FFT stages through the object's U and T.  Every cell a later stage reads is written by the stage
// before it, so no buffer is cleared and an adjoint call in between (which clears what it uses) changes nothing.
// The Wigner-d table of k_polar_modes for one spin weight, built on first use and kept by the object (only a complete table stays).
static int polar_table(hx_pointsht *ps, int spin, const double **tab)
{
    const int lmax = ps->lmax;
    if (!ps->polar_x.p || !ps->polar_xlo.p) {
        const int K = std::min(NUFFT_POLAR_K, ps->N / 4);
        std::vector<double> x(2 * K), xlo(2 * K);
        for (int r = 0; r < K; ++r) {
            const long double c = cosl(2.0L * 3.141592653589793238462643383279502884L * (r + 0.5L) / ps->N);
            x[r] = (double)c; xlo[r] = (double)(c - (long double)x[r]);
            x[K + r] = -x[r]; xlo[K + r] = -xlo[r];
        }
        HX_TRY(upload(ps->polar_x, x));
        HX_TRY(upload(ps->polar_xlo, xlo));
        ps->polar_K = K;
        ps->polar_M = std::min(lmax, NUFFT_POLAR_M);
    }
    std::unique_ptr<DevBuf> &slot = ps->polar_tab[spin];
    if (!slot) {
        std::unique_ptr<DevBuf> buf(new DevBuf);
        const int nt = spin ? 2 : 1, n2 = 2 * ps->polar_K;
        const size_t tsize = (size_t)(lmax + 1) * n2;
        HX_TRY(buf->alloc(sizeof(double) * tsize * nt * (ps->polar_M + 1)));
        for (int m = 0; m <= ps->polar_M; ++m)
            for (int t = 0; t < nt; ++t)
                HX_TRY(wigner_table_build(lmax, m, t == 0 ? -spin : spin, n2, ps->polar_x.as<double>(), ps->polar_xlo.as<double>(),
                                          buf->as<double>() + tsize * ((size_t)m * nt + t), n2, 1));
        slot = std::move(buf);
    }
    *tab = slot->as<double>();
    return HX_OK;
}

int pointsht_alm_to_grids(hx_pointsht *ps, int spin, int ncomp, const double2 *d_alm, const GridFor &grid_for, const GridDone &grid_done)
{
    hx_plan *eq = ps->eq;
    const int lmax = ps->lmax, N = ps->N, n1 = ps->n1, W = ps->W;
    hipStream_t st = rt().stream;
    const int cpu = spin ? 2 : 1;
    if (spin < 0 || ncomp < 1 || ncomp % cpu) return fail(HX_ERR_ARG, "point transform: %d components of spin %d", ncomp, spin);
    if (spin > lmax) {  // no l >= s below the band limit: zero fields
        for (int c = 0; c < ncomp; ++c) {
            double *grid = nullptr;
            HX_TRY(grid_for(c, &grid));
            HX_HIP(hipMemsetAsync(grid, 0, sizeof(double) * (size_t)n1 * n1, st));
            if (grid_done) HX_TRY(grid_done(c, grid));
        }
        return HX_OK;
    }
    const bool generic = analysis_generic_spin(spin);  // a spin weight other than 0 and 2 (HX_SPIN_GENERIC=1: 2 as well)
    const int umax = generic ? 1 : synth_valu_max_units(spin);
    HX_TRY(ps->T.alloc(sizeof(double2) * (size_t)(lmax + 1) * n1));
    HX_TRY(ps->U.alloc(sizeof(double2) * (size_t)(lmax + 1) * N));
    HX_TRY(eq->F.alloc(sizeof(double) * (size_t)(lmax + 1) * eq->nrp_pad * 4 * std::min(umax * cpu, ncomp)));
    const double *polar = nullptr;
    if (spin <= NUFFT_POLAR_SMAX) HX_TRY(polar_table(ps, spin, &polar));
    NufftSyn a;
    a.Fv = eq->F.as<double>(); a.grid = nullptr; a.src = nullptr; a.dst = nullptr;
    a.dec = ps->dec_phi.as<double>(); a.fac = ps->fac_theta.as<double2>(); a.tw = ps->tw.as<double2>();
    a.parity = spin & 1;
    a.lmax = lmax; a.N = N; a.n1 = n1; a.twN = ps->twN;
    a.band = std::min(n1, n1 / 2 + W + 4);  // rows a point with 0 <= theta <= pi can read
    a.row0 = (n1 - W / 2 - 2) % n1;
    auto launch = [&](int mode, int n, int rows) {
        const int ns = std::min(n, NUFFT_LDS_MAX), threads = std::min(512, std::max(64, ns / 16));
        a.n = n;
        const size_t lds = (size_t)lds_fft_slots(ns) * sizeof(double2);
        if (mode == 0) hipLaunchKernelGGL(k_nufft_fft_syn<0>, dim3(rows), dim3(threads), lds, st, a);
        else if (mode == 1) hipLaunchKernelGGL(k_nufft_fft_syn<1>, dim3(rows), dim3(threads), lds, st, a);
        else hipLaunchKernelGGL(k_nufft_fft_syn<2>, dim3(rows), dim3(threads), lds, st, a);
    };
    for (int c0 = 0; c0 < ncomp;) {
        int units = umax;
        while (units * cpu > ncomp - c0) units >>= 1;
        const int nc = units * cpu;
        hx_plan::SpinData *sd = nullptr;
        hx_plan::TaskSet *ts = nullptr;
        HX_TRY(spin_data(eq, spin, generic, &sd));
        HX_TRY(task_set(eq, spin, generic, synth_valu_task_blocks(spin, units), &ts));
        HX_TRY(launch_synth_valu(eq, spin, units, *sd, *ts, d_alm + (size_t)c0 * eq->nlm, eq->F.as<double>(), generic));
        a.nv = 4 * nc;
        a.mstride = (long long)eq->nrp_pad * a.nv;
        if (polar) {
            ProfScope pf("polar_modes");
            PolarModes pm;
            pm.tab = polar; pm.alm = d_alm + (size_t)c0 * eq->nlm; pm.Fv = eq->F.as<double>();
            pm.nlm = eq->nlm; pm.mstride = a.mstride;
            pm.lmax = lmax; pm.s = spin; pm.K = ps->polar_K; pm.nv = a.nv;
            hipLaunchKernelGGL(k_polar_modes, dim3(ps->polar_M + 1, 2 * ps->polar_K, units), dim3(64), 0, st, pm);
        }
        for (int c = 0; c < nc; ++c) {
            double *grid = nullptr;
            HX_TRY(grid_for(c0 + c, &grid));
            {
                ProfScope pf("nufft_fft_syn");
                a.comp4 = 4 * c;
                a.dst = ps->U.as<double2>();
                launch(0, N, lmax + 1);
                a.src = ps->U.as<double2>(); a.dst = ps->T.as<double2>();
                launch(1, n1, lmax + 1);
                a.src = ps->T.as<double2>(); a.grid = grid;
                launch(2, n1, a.band);
                HX_HIP(hipGetLastError());
            }
            if (grid_done) HX_TRY(grid_done(c0 + c, grid));
        }
        c0 += nc;
    }
    return HX_OK;
}

// Half two: one component of a grid at n points.  The path is the spread's (pointsht_order): one thread per point below 300000
// points, LDS tiles from there on.  That cross-over was measured for the spread (tools/time_pointsht.py) and is kept, so that both
// directions share one order per call.  Measured for the gather at lmax 6144 (HX_NUFFT_TILES=0 / 1, DIRECTION=both
// tools/time_pointsht.py; ms per component, one thread per point / tiles):
// 10^5 0.2 / 0.9, 3 10^5 1.0 / 1.3, 10^6 2.1 / 2.1, 3 10^6 6.4 / 4.5, 10^7 19.1 / 5.6 -- its own cross-over lies near 10^6.  (With a
// window loaded for every occupied tile the tiles took 3.2 / 4.6 / 5.2 / 5.5 / 5.9: hence the sparse branch of k_nufft_gather_tiles.)
int pointsht_gather_one(hx_pointsht *ps, const PointOrder &o, int64_t npoints, const double2 *loc, const double *grid, double *val)
{
    const int n1 = ps->n1, W = ps->W;
    hipStream_t st = rt().stream;
    ProfScope pf("nufft_gather");
    if (o.tiles) {
        const int ntx = n1 / NUFFT_TS + 1, nty = (n1 / 2 + W + NUFFT_TPAD) / NUFFT_TS + 1;
        hipLaunchKernelGGL(k_nufft_gather_tiles, dim3((unsigned)(ntx * nty) + 1), dim3(256), 0, st, (long long)npoints, loc, o.key, o.idx, grid,
                           val, n1, W, ps->beta, ntx, (unsigned)(ntx * nty));
    } else if (npoints > 0) {
        const long long nblk = std::min<long long>((npoints + 255) / 256, 1 << 20);
        hipLaunchKernelGGL(k_nufft_gather, dim3((unsigned)nblk), dim3(256), 0, st, (long long)npoints, loc, grid, val, n1, W, ps->beta,
                           ps->nbad.as<unsigned long long>());
    }
    HX_HIP(hipGetLastError());
    return HX_OK;
}

}  // namespace hx

// A resident set of grids: the field of `ncomp` components of one hx_pointsht_grids call, to be read at any number of point sets.
struct hx_pointgrid {
    hx_pointsht *ps = nullptr;  // borrowed: tables, sort buffers, the counter of bad points
    int ncomp = 0;
    hx::DevBuf grids;           // [ncomp][n1][n1]
};

static int pointsht_check_bad(hx_pointsht *ps, const char *who)
{
    unsigned long long nbad = 0;
    hipStream_t st = rt().stream;
    HX_HIP(hipMemcpyAsync(&nbad, ps->nbad.p, 8, hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (nbad) return fail(HX_ERR_ARG, "%s: %llu points with colatitude outside [0, pi] or non-finite coordinates", who, nbad);
    return HX_OK;
}

extern "C" int hx_pointsht_synthesis(hx_pointsht *ps, int spin, int ncomp, int64_t npoints, const double *loc, const double *alm,
                                     double *map)
{
    HX_TRY(ensure_ready());
    if (!ps || !alm || (npoints > 0 && (!loc || !map))) return fail(HX_ERR_ARG, "hx_pointsht_synthesis: null argument");
    if (spin < 0) return fail(HX_ERR_ARG, "hx_pointsht_synthesis: negative spin weight %d", spin);
    if (ncomp < 1 || (spin > 0 && (ncomp & 1)) || npoints < 0) return fail(HX_ERR_ARG, "hx_pointsht_synthesis: bad component or point count");
    if (npoints == 0) return HX_OK;
    const int n1 = ps->n1;
    InView vloc, valm;
    OutView vmap;
    HX_TRY(vloc.bind(loc, sizeof(double) * 2 * (size_t)npoints));
    HX_TRY(valm.bind(alm, sizeof(double2) * (size_t)ncomp * ps->eq->nlm));
    HX_TRY(vmap.bind(map, sizeof(double) * (size_t)ncomp * npoints));
    hipStream_t st = rt().stream;
    HX_TRY(ps->grid.alloc(sizeof(double) * (size_t)n1 * n1));
    HX_HIP(hipMemsetAsync(ps->nbad.p, 0, 8, st));
    PointOrder order;
    HX_TRY(pointsht_order(ps, npoints, vloc.as<double2>(), &order));
    // one grid serves every component: filled by the component's FFT stages and read right behind them
    const GridFor one = [&](int, double **grid) -> int {
        *grid = ps->grid.as<double>();
        return HX_OK;
    };
    const GridDone read = [&](int c, const double *grid) -> int {
        return pointsht_gather_one(ps, order, npoints, vloc.as<double2>(), grid, vmap.as<double>() + (size_t)c * npoints);
    };
    HX_TRY(pointsht_alm_to_grids(ps, spin, ncomp, valm.as<double2>(), one, read));
    HX_TRY(pointsht_check_bad(ps, "hx_pointsht_synthesis"));
    HX_TRY(vmap.finish());
    return HX_OK;
}

extern "C" hx_pointgrid *hx_pointsht_grids(hx_pointsht *ps, int spin, int ncomp, const double *alm)
{
    if (ensure_ready() != HX_OK) return nullptr;
    if (!ps || !alm || spin < 0 || ncomp < 1 || (spin > 0 && (ncomp & 1))) {
        fail(HX_ERR_ARG, "hx_pointsht_grids: null argument, negative spin weight or bad component count");
        return nullptr;
    }
    const size_t cells = (size_t)ps->n1 * ps->n1;
    hx_pointgrid *g = new hx_pointgrid;
    g->ps = ps;
    g->ncomp = ncomp;
    InView valm;
    const GridFor resident = [&](int c, double **grid) -> int {
        *grid = g->grids.as<double>() + cells * c;
        return HX_OK;
    };
    if (g->grids.alloc(sizeof(double) * cells * ncomp) != HX_OK || valm.bind(alm, sizeof(double2) * (size_t)ncomp * ps->eq->nlm) != HX_OK ||
        pointsht_alm_to_grids(ps, spin, ncomp, valm.as<double2>(), resident, GridDone()) != HX_OK ||
        hipStreamSynchronize(rt().stream) != hipSuccess) {
        delete g;
        return nullptr;
    }
    return g;
}

extern "C" int hx_pointgrid_gather(hx_pointgrid *g, int64_t npoints, const double *loc, double *map)
{
    HX_TRY(ensure_ready());
    if (!g || npoints < 0 || (npoints > 0 && (!loc || !map))) return fail(HX_ERR_ARG, "hx_pointgrid_gather: null argument or negative point count");
    if (npoints == 0) return HX_OK;
    hx_pointsht *ps = g->ps;
    const size_t cells = (size_t)ps->n1 * ps->n1;
    InView vloc;
    OutView vmap;
    HX_TRY(vloc.bind(loc, sizeof(double) * 2 * (size_t)npoints));
    HX_TRY(vmap.bind(map, sizeof(double) * (size_t)g->ncomp * npoints));
    HX_HIP(hipMemsetAsync(ps->nbad.p, 0, 8, rt().stream));
    PointOrder order;
    HX_TRY(pointsht_order(ps, npoints, vloc.as<double2>(), &order));
    for (int c = 0; c < g->ncomp; ++c)
        HX_TRY(pointsht_gather_one(ps, order, npoints, vloc.as<double2>(), g->grids.as<double>() + cells * c, vmap.as<double>() + (size_t)c * npoints));
    HX_TRY(pointsht_check_bad(ps, "hx_pointgrid_gather"));
    HX_TRY(vmap.finish());
    return HX_OK;
}

extern "C" void hx_pointgrid_destroy(hx_pointgrid *g)
{
    if (!g) return;
    if (rt().ready) (void)hipStreamSynchronize(rt().stream);
    delete g;
}

extern "C" int hx_pointsht_adjoint(hx_pointsht *ps, int spin, int ncomp, int64_t npoints, const double *loc, const double *map,
                                   double *alm)
{
    HX_TRY(ensure_ready());
    if (!ps || !alm || (npoints > 0 && (!loc || !map))) return fail(HX_ERR_ARG, "hx_pointsht_adjoint: null argument");
    if (spin < 0) return fail(HX_ERR_ARG, "hx_pointsht_adjoint: negative spin weight %d", spin);
    if (ncomp < 1 || (spin > 0 && (ncomp & 1)) || npoints < 0) return fail(HX_ERR_ARG, "hx_pointsht_adjoint: bad component or point count");
    const int n1 = ps->n1;
    InView vloc, vmap;
    OutView valm;
    HX_TRY(vloc.bind(loc, sizeof(double) * 2 * (size_t)npoints));
    HX_TRY(vmap.bind(map, sizeof(double) * (size_t)ncomp * npoints));
    HX_TRY(valm.bind(alm, sizeof(double2) * (size_t)ncomp * ps->eq->nlm));
    hipStream_t st = rt().stream;
    HX_TRY(ps->grid.alloc(sizeof(double) * (size_t)n1 * n1));
    HX_HIP(hipMemsetAsync(ps->nbad.p, 0, 8, st));
    PointOrder order;
    HX_TRY(pointsht_order(ps, npoints, vloc.as<double2>(), &order));
    // one grid serves every component: cleared and filled right before the component's FFT stages
    const GridOf fill = [&](int c, const double **grid) -> int {
        ProfScope pf("nufft_spread");
        HX_HIP(hipMemsetAsync(ps->grid.p, 0, sizeof(double) * (size_t)n1 * n1, st));
        HX_TRY(pointsht_spread_one(ps, order, npoints, vloc.as<double2>(), vmap.as<double>() + (size_t)c * npoints, ps->grid.as<double>()));
        *grid = ps->grid.as<double>();
        return HX_OK;
    };
    HX_TRY(pointsht_grids_to_alm(ps, spin, ncomp, fill, valm.as<double2>()));
    unsigned long long nbad = 0;
    HX_HIP(hipMemcpyAsync(&nbad, ps->nbad.p, 8, hipMemcpyDeviceToHost, st));
    HX_HIP(hipStreamSynchronize(st));
    if (nbad) return fail(HX_ERR_ARG, "hx_pointsht_adjoint: %llu points with colatitude outside [0, pi] or non-finite values", nbad);
    HX_TRY(valm.finish());
    return HX_OK;
}
