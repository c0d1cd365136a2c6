// hx_pixwin.hip -- the HEALPix pixel window function of any spin weight, computed from the pixel shapes (hx_pixel_window,
// hx_pixel_window_rings): what healpy.pixwin reads out of its data files (heracles/healpy.py:68-115, deconvolve=True), without a file.
//
// Quantity.  A_lm(p) = (1 / Omega) int_p sY_lm dOmega, Omega = 4 pi / (12 N^2): the average of sY_lm over pixel p in the local
// (theta, phi) basis.  W_l^2 = 4 pi / ((2l+1) 12 N^2) sum_p sum_{m=-l..l} |A_lm(p)|^2 for l >= s, W_l = 1 below.
//
// Reduction to one dimension (face coordinates of hxpix::xyf2lonlat): z depends on jr = jrll - x - y only -- z = 1 - jr^2 / 3, nr = jr
// in the north cap (jr < 1), z = (2 - jr) 2 / 3, nr = 1 in the belt -- and phi = (pi/4)(jpll + (x - y) / nr).  The pixel of ring r spans
// jr N in [r - 1, r + 1]; at a given jr its x - y runs over d0 +- h, h = (jr N - (r - 1)) / N above the ring centre, ((r + 1) - jr N) / N
// below.  The phi integral is closed:
//     A_lm = (1 / Omega) int djr (2/3) nr (s)lambda_lm(z) e^{-i m (pi/4) d0 / nr} G_m,   G_0 = 2 D, G_m = 2 sin(m D) / m, D = (pi/4) h / nr,
// and each half of the pixel gets a 12-node Gauss-Legendre rule in jr (the integrand is analytic on a half; the cap/belt change at
// jr = 1 is the centre of ring N).  With node t in [0, 1], weight w: the factor of lambda at a node is (2 w nrN / pi) G_m, nrN = nr N.
//
// Shapes.  Belt rings N < r <= 2N: one shape (the phase is constant), 4N pixels.  Rings r <= N: d0 N in {-(r-1), -(r-3), .., r-1} on
// each of 4 faces; d0 -> -d0 conjugates A, so ceil(r / 2) shapes of 8 pixels (4 where d0 = 0).  South mirrors north.
//
// Kernel k_pixwin_shapes: one wave per (shape, group of m-chunks).  A chunk is 32 orders; an order has two lanes, one per half of the
// pixel, each with its 12 nodes in registers: chain values, node weights, scale exponents.  ALL lanes of a chunk start their chains
// together -- lane (m) is at l = l0(m) + k in step k, l0 = max(m, s) -- so that no step is predicated; spin 0 runs the two-step
// recursion of the plan (tables of k_init_norm0: both parities per step pair), s >= 1 the one-step recursion of k_init_norm_s for the
// pair (+s, -s), seeds from spin_seeds.  The values are scaled as everywhere (hx_sht_common.h): a chain below 2^-300 counts as zero,
// chains are promoted every 32 steps; a block of 32 steps in which no chain of the wave is live runs recursions only.  Per l the two
// halves are added (one DPP exchange) and |A|^2 goes to an LDS tile [l mod 64][order]; after a block its 32 complete rows are summed
// over the orders in a fixed order by the lane l mod 32, which adds them to the wave's own row of the partial buffer.  k_pixwin_rows
// adds the partial rows of a ring, shape by shape, group by group: no atomics, the same bits every time.
#include <algorithm>
#include <cmath>
#include <vector>

#include "hx_sht_common.h"

namespace hx {

namespace {

constexpr int PW_NODES = 12;  // Gauss-Legendre nodes per half pixel
constexpr int PW_MS = 32;     // orders per chunk (two lanes each)
constexpr int PW_LB = 32;     // l per block
constexpr int PW_TS = 33;     // row stride of the LDS tile [64][PW_MS]
constexpr int PW_ITEMS = 4096;  // shapes per launch: bounds the partial buffer, never below one ring (<= 4096 shapes at nside 8192)
constexpr int PW_WAVES = 2048;  // waves a launch aims for: small rings split their m-chunks over groups

struct PwRule {
    double t[PW_NODES], w[PW_NODES];  // nodes and weights on [0, 1]
};
struct PwItem {
    int ring, d, mlim, pad;  // ring 1..2N, |d0| N, highest order that contributes on the ring (the plan's rule)
};
struct PwParams {
    int nside, spin, lmax, groups, nchunk;
    const PwItem *items;
    const double *mfac, *kf;
    double *partial;  // [item][group][lmax + 1]
    PwRule rule;
};

template <bool S0>
__global__ __launch_bounds__(64) void k_pixwin_shapes(PwParams A, const double2 *__restrict__ coefn, const double *__restrict__ alphan)
{
    constexpr int NN = PW_NODES;
    __shared__ double tile[64 * PW_TS];
    const int lane = threadIdx.x, half = lane & 1, slot = lane >> 1;
    const PwItem it = A.items[blockIdx.x / A.groups];
    const int g = blockIdx.x % A.groups;
    const int N = A.nside, lmax = A.lmax, s = A.spin;
    double *__restrict__ prow = A.partial + (long long)blockIdx.x * (lmax + 1);

    double xx[NN], wre[NN], wim[NN], vc[NN][2], vp[NN][2];
    int sc[NN][2];

    auto promote = [&](int j, int c) __attribute__((always_inline)) {
        const int hc = __double2hiint(vc[j][c]), hp = __double2hiint(vp[j][c]);
        const bool up = sc[j][c] < 0 && (hc & 0x7ff00000) >= 0x3ff00000;
        const int sub = up ? (300 << 20) : 0;
        const bool pz = up && (hp & 0x7ff00000) <= (300 << 20);
        vc[j][c] = __hiloint2double(hc - sub, __double2loint(vc[j][c]));
        vp[j][c] = pz ? 0.0 : __hiloint2double(hp - sub, __double2loint(vp[j][c]));
        sc[j][c] += up ? 1 : 0;
    };

    for (int c = g; c < A.nchunk && c * PW_MS <= it.mlim; c += A.groups) {
        const int m = c * PW_MS + slot;
        const bool valid = m <= lmax;
        const int mm = valid ? m : lmax;
        const int l0 = S0 ? mm : (mm > s ? mm : s);
        const int base = S0 ? c * PW_MS : (c * PW_MS > s ? c * PW_MS : s);
        const int off = l0 - base;  // 0 .. 31
        const long long cb = almidx(lmax, 0, mm);
        const double m2 = m == 0 ? 1.0 : 2.0;  // spin 0: the orders -m and m have the same |A|

        for (int i = lane; i < 64 * PW_TS; i += 64) tile[i] = 0.0;

        // ---- nodes of this lane's half: geometry, weight, seeds ----
#pragma unroll
        for (int j = 0; j < NN; ++j) {
            const double t = A.rule.t[j];
            const double jrN = (double)(it.ring - 1 + half) + t, hN = half ? 1.0 - t : t;
            const bool cap = jrN < (double)N;
            const double jr = jrN / (double)N, nrN = cap ? jrN : (double)N;
            double z, om, st;
            if (cap) {
                om = jr * jr * (1.0 / 3.0);
                z = 1.0 - om;
                st = sqrt(om * (2.0 - om));
            } else {
                z = (2.0 - jr) * (2.0 / 3.0);
                om = 1.0 - z;
                st = sqrt((1.0 - z) * (1.0 + z));
            }
            xx[j] = S0 ? z * z : z;
            // (2 w nrN / pi) G_m e^{-i m (pi/4) d0 / nr}
            const double q = 0.25 / nrN;
            double amp;
            if (m == 0) amp = A.rule.w[j] * hN;
            else amp = A.rule.w[j] * nrN * (4.0 / M_PI) * sinpi((double)m * hN * q) / (double)m;
            double ps, pc;
            sincospi((double)m * (double)it.d * q, &ps, &pc);
            wre[j] = valid ? amp * pc : 0.0;
            wim[j] = valid ? -amp * ps : 0.0;
            SVal a, b;
            if (S0) {
                a = spow(st, mm);
                a.v *= A.mfac[mm];
                b = a;
                b.v *= sqrt(2.0 * mm + 3.0) * z;  // lambda_{m+1,m} = sqrt(2m+3) x lambda_mm
                snorm_small(a);
                snorm_small(b);
            } else {
                spin_seeds(s, mm, st, om, A.kf[mm], a, b);
            }
            // (a lane past lmax carries zeros: live, and nothing to add)
            vc[j][0] = valid ? a.v : 0.0; sc[j][0] = valid ? a.e : 0;
            vc[j][1] = valid ? b.v : 0.0; sc[j][1] = valid ? b.e : 0;
            vp[j][0] = vp[j][1] = 0.0;
            __builtin_amdgcn_sched_barrier(0);  // node by node: interleaved, the twelve set-ups hold far more values than registers
        }
        __syncthreads();

        // one block of 32 l.  ACC: the values enter the sums; STEADY: every chain of the wave is live (no masks)
        auto block = [&](auto ACCC, auto STEADYC, int kb) __attribute__((always_inline)) {
            constexpr bool ACC = decltype(ACCC)::value, STEADY = decltype(STEADYC)::value;
            const long long ib = cb + l0 + kb;
            // four l per trip (the two registers of a chain swap roles from step to step: an even number of steps per trip); the
            // coefficients of the next trip are requested before this one runs
            constexpr int TR = 4, CO = S0 ? 0 : 1;  // (the one-step coefficients are indexed by the target l)
            double2 ncf[TR];
            double nal[TR];
#pragma unroll
            for (int t = 0; t < TR; ++t) {
                ncf[t] = coefn[ib + t + CO];
                nal[t] = ACC ? alphan[ib + t] : 0.0;
            }
#pragma unroll 1
            for (int k0 = 0; k0 < PW_LB; k0 += TR) {
                double2 cf[TR];
                double al[TR];
#pragma unroll
                for (int t = 0; t < TR; ++t) {
                    cf[t] = ncf[t];
                    al[t] = nal[t];
                    ncf[t] = coefn[ib + k0 + TR + t + CO];  // (past the block: the next block's, or the padding of the tables)
                    nal[t] = ACC ? alphan[ib + k0 + TR + t] : 0.0;
                }
                if (S0) {
#pragma unroll
                    for (int t = 0; t < TR; t += 2) {
                        const bool odd = (t >> 1) & 1;
                        const double2 c0 = cf[t], c1 = cf[t + 1];
                        double a0r = 0.0, a0i = 0.0, a1r = 0.0, a1i = 0.0;
#pragma unroll
                        for (int j = 0; j < NN; ++j) {
                            double &u0 = odd ? vp[j][0] : vc[j][0], &o0 = odd ? vc[j][0] : vp[j][0];
                            double &u1 = odd ? vp[j][1] : vc[j][1], &o1 = odd ? vc[j][1] : vp[j][1];
                            if (ACC) {
                                const double e0 = (STEADY || sc[j][0] == 0) ? u0 : 0.0, e1 = (STEADY || sc[j][1] == 0) ? u1 : 0.0;
                                a0r = fma(e0, wre[j], a0r); a0i = fma(e0, wim[j], a0i);
                                a1r = fma(e1, wre[j], a1r); a1i = fma(e1, wim[j], a1i);
                            }
                            o0 = fma(fma(c0.x, xx[j], c0.y), u0, -o0);
                            o1 = fma(fma(c1.x, xx[j], c1.y), u1, -o1);
                        }
                        if (ACC) {
                            a0r += __shfl_xor(a0r, 1); a0i += __shfl_xor(a0i, 1);
                            a1r += __shfl_xor(a1r, 1); a1i += __shfl_xor(a1i, 1);
                            if (!half) {
                                const int row = off + kb + k0 + t;
                                tile[(row & 63) * PW_TS + slot] = m2 * (al[t] * al[t]) * (a0r * a0r + a0i * a0i);
                                tile[((row + 1) & 63) * PW_TS + slot] = m2 * (al[t + 1] * al[t + 1]) * (a1r * a1r + a1i * a1i);
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < TR; ++t) {
                        const bool odd = t & 1;
                        const double2 c = cf[t];
                        double apr = 0.0, api = 0.0, amr = 0.0, ami = 0.0;
#pragma unroll
                        for (int j = 0; j < NN; ++j) {
                            double &u0 = odd ? vp[j][0] : vc[j][0], &o0 = odd ? vc[j][0] : vp[j][0];
                            double &u1 = odd ? vp[j][1] : vc[j][1], &o1 = odd ? vc[j][1] : vp[j][1];
                            if (ACC) {
                                const double e0 = (STEADY || sc[j][0] == 0) ? u0 : 0.0, e1 = (STEADY || sc[j][1] == 0) ? u1 : 0.0;
                                apr = fma(e0, wre[j], apr); api = fma(e0, wim[j], api);
                                amr = fma(e1, wre[j], amr); ami = fma(e1, wim[j], ami);
                            }
                            o0 = fma(fma(c.x, xx[j], c.y), u0, -o0);
                            o1 = fma(fma(c.x, xx[j], -c.y), u1, -o1);
                        }
                        if (ACC) {
                            apr += __shfl_xor(apr, 1); api += __shfl_xor(api, 1);
                            amr += __shfl_xor(amr, 1); ami += __shfl_xor(ami, 1);
                            if (!half) {
                                // sum over -l..l: |A_l0|^2 + sum_{m>0} (|A+|^2 + |A-|^2)
                                const double p = (apr * apr + api * api) + (m == 0 ? 0.0 : (amr * amr + ami * ami));
                                tile[((off + kb + k0 + t) & 63) * PW_TS + slot] = (al[t] * al[t]) * p;
                            }
                        }
                    }
                }
            }
        };
        using BT = std::integral_constant<bool, true>;
        using BF = std::integral_constant<bool, false>;

        // rows kb .. kb + 31 of the tile are complete: lane (l mod 32) adds the orders in order, clears the row, adds to its l
        auto consume = [&](int kb) __attribute__((always_inline)) {
            __syncthreads();
            if (lane < 32) {
                const int i = (lane - (base + kb)) & 31, l = base + kb + i;
                double *tr = tile + ((kb + i) & 63) * PW_TS;
                double sum = 0.0;
#pragma unroll
                for (int q = 0; q < PW_MS; ++q) {
                    sum += tr[q];
                    tr[q] = 0.0;
                }
                if (l <= lmax) prow[l] += sum;
            }
            __syncthreads();
        };
        // lead-in: some chain of the wave is still scaled.  A loop of its own, so that the exponents are dead in the steady loop.
        int kb = 0;
        for (; base + kb <= lmax; kb += PW_LB) {
            bool dd = true, live = true;
#pragma unroll
            for (int j = 0; j < NN; ++j) {
                promote(j, 0);
                promote(j, 1);
                dd = dd && sc[j][0] < 0 && sc[j][1] < 0;
                live = live && sc[j][0] == 0 && sc[j][1] == 0;
            }
            if (__all(live)) break;
            if (__all(dd || !valid)) block(BF{}, BF{}, kb);
            else block(BT{}, BF{}, kb);
            consume(kb);
        }
        for (; base + kb <= lmax; kb += PW_LB) {
            block(BT{}, BT{}, kb);
            consume(kb);
        }
    }
}

// rows[ring][l] = 4 pi / (2l+1) sum over the pixels of the ring and over m of |A_lm|^2: shapes in order, groups in order
__global__ __launch_bounds__(256) void k_pixwin_rows(int nside, int spin, int lmax, int groups, const PwItem *__restrict__ items,
                                                      const int *__restrict__ first, const double *__restrict__ partial, double *__restrict__ rows)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x, ri = blockIdx.y;
    if (l > lmax) return;
    double acc = 0.0;
    for (int it = first[ri]; it < first[ri + 1]; ++it) {
        double sa = 0.0;
        for (int g = 0; g < groups; ++g) sa = __dadd_rn(sa, partial[((long long)it * groups + g) * (lmax + 1) + l]);
        const PwItem I = items[it];
        const double mult = I.ring <= nside ? (I.d == 0 ? 4.0 : 8.0) : 4.0 * nside;
        acc = __dadd_rn(acc, __dmul_rn(mult, sa));
    }
    rows[(long long)ri * (lmax + 1) + l] = l < spin ? 0.0 : __dmul_rn(acc, 4.0 * M_PI / (2.0 * l + 1.0));
}

// w2[l] += mult(ring) rows[ring][l], ring by ring: the southern twin counts with the northern ring, the equator once
__global__ __launch_bounds__(256) void k_pixwin_accumulate(int nside, int lmax, int ring0, int nrings, const double *__restrict__ rows, double *__restrict__ w2)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > lmax) return;
    double acc = w2[l];
    for (int ri = 0; ri < nrings; ++ri)
        acc = __dadd_rn(acc, __dmul_rn(ring0 + ri == 2 * nside ? 1.0 : 2.0, rows[(long long)ri * (lmax + 1) + l]));
    w2[l] = acc;
}

__global__ __launch_bounds__(256) void k_pixwin_finish(int nside, int spin, int lmax, const double *__restrict__ w2, double *__restrict__ out)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > lmax) return;
    out[l] = l < spin ? 1.0 : __dsqrt_rn(__ddiv_rn(w2[l], 12.0 * (double)nside * (double)nside));
}

// Gauss-Legendre rule of PW_NODES points on [0, 1]
PwRule pixwin_rule()
{
    PwRule R;
    const int n = PW_NODES;
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int i = 0; i < n; ++i) {
        long double x = cosl(pi * (i + 0.75L) / (n + 0.5L)), dp = 1.0L;
        for (int itn = 0; itn < 100; ++itn) {
            long double p0 = 1.0L, p1 = x;
            for (int k = 2; k <= n; ++k) {
                const long double p2 = ((2 * k - 1) * x * p1 - (k - 1) * p0) / k;
                p0 = p1;
                p1 = p2;
            }
            dp = n * (x * p1 - p0) / (x * x - 1.0L);
            const long double dx = p1 / dp;
            x -= dx;
            if (fabsl(dx) < 1e-19L) break;
        }
        // (one more evaluation for the derivative at the converged node)
        long double p0 = 1.0L, p1 = x;
        for (int k = 2; k <= n; ++k) {
            const long double p2 = ((2 * k - 1) * x * p1 - (k - 1) * p0) / k;
            p0 = p1;
            p1 = p2;
        }
        dp = n * (x * p1 - p0) / (x * x - 1.0L);
        R.t[n - 1 - i] = (double)(0.5L * (1.0L + x));
        R.w[n - 1 - i] = (double)(1.0L / ((1.0L - x * x) * dp * dp));
    }
    return R;
}

int pixwin_check(const char *who, int nside, int spin, int lmax)
{
    if (nside < 1 || nside > 8192) return fail(HX_ERR_ARG, "%s: nside %d is outside 1..8192", who, nside);
    if (lmax < 0) return fail(HX_ERR_ARG, "%s: lmax %d", who, lmax);
    if (spin < 0 || spin > lmax) return fail(HX_ERR_ARG, "%s: spin %d is outside 0..lmax = %d", who, spin, lmax);
    if (lmax > 4 * nside)
        return fail(HX_ERR_ARG, "%s: lmax %d: the window of NSIDE=%d is computed up to lmax = 4 nside = %d (the quadrature rule is validated up to there)",
                    who, lmax, nside, 4 * nside);
    return HX_OK;
}

struct PlanHold {
    hx_plan *pl = nullptr;
    ~PlanHold() { if (pl) hx_plan_destroy(pl); }
};

// the rows of the northern rings ring0 .. ring0 + count - 1 into d_rows [count][lmax + 1] (if given), and / or their weighted sum
// added to d_w2 [lmax + 1] (if given), launch by launch of whole rings
int pixwin_run(int nside, int spin, int lmax, int ring0, int count, double *d_rows, double *d_w2)
{
    // the recursion tables depend on the band limit only: those of an equiangular plan, which has no ring Fourier stage to set up
    PlanHold hold;
    hold.pl = plan_create_equiangular(((2 * lmax + 2) / 4 + 1) * 4, lmax);
    if (!hold.pl) return HX_ERR_HIP;
    hx_plan *pl = hold.pl;
    hx_plan::SpinData *sd = nullptr;
    HX_TRY(spin_data(pl, spin, spin != 0, &sd));
    hipStream_t st = rt().stream;
    PwParams A;
    A.nside = nside; A.spin = spin; A.lmax = lmax;
    A.nchunk = lmax / PW_MS + 1;
    A.mfac = pl->mfac.as<double>();
    A.kf = sd->kf.as<double>();
    A.rule = pixwin_rule();
    const size_t rowlen = (size_t)lmax + 1;
    const unsigned lblocks = (unsigned)((rowlen + 255) / 256);
    DevBuf d_items, d_first, d_partial, d_rowbuf;
    std::vector<PwItem> items;
    std::vector<int> first;
    ProfScope ps("pixel_window");
    for (int ra = ring0; ra < ring0 + count;) {
        items.clear();
        first.assign(1, 0);
        int rb = ra;
        while (rb < ring0 + count) {
            const int ns = rb <= nside ? (rb + 1) / 2 : 1;
            if (!items.empty() && (int)items.size() + ns > PW_ITEMS) break;
            // the largest sin(theta) of the ring's pixels is at their lower corner, jr = (r + 1) / N (the equator at most)
            const double jr = std::min((double)(rb + 1) / nside, 2.0);
            const double z = jr < 1.0 ? 1.0 - jr * jr / 3.0 : (2.0 - jr) * (2.0 / 3.0);
            const int mlim = ring_mlim(lmax, spin, std::sqrt((1.0 - z) * (1.0 + z)), z);
            for (int j = 0; j < ns; ++j) items.push_back(PwItem{rb, rb <= nside ? rb - 1 - 2 * j : 0, mlim, 0});
            first.push_back((int)items.size());
            ++rb;
        }
        const int nit = (int)items.size(), nr = rb - ra;
        A.groups = nit >= PW_WAVES ? 1 : std::min(A.nchunk, (PW_WAVES + nit - 1) / nit);
        const size_t pbytes = sizeof(double) * rowlen * (size_t)nit * A.groups;
        HX_TRY(upload(d_items, items));
        HX_TRY(upload(d_first, first));
        HX_TRY(d_partial.alloc(pbytes));
        HX_HIP(hipMemsetAsync(d_partial.p, 0, pbytes, st));
        A.items = d_items.as<PwItem>();
        A.partial = d_partial.as<double>();
        if (spin == 0)
            hipLaunchKernelGGL(k_pixwin_shapes<true>, dim3((unsigned)nit * A.groups), dim3(64), 0, st, A, sd->cn.as<double2>(), sd->al.as<double>());
        else
            hipLaunchKernelGGL(k_pixwin_shapes<false>, dim3((unsigned)nit * A.groups), dim3(64), 0, st, A, sd->cn.as<double2>(), sd->al.as<double>());
        HX_HIP(hipGetLastError());
        double *rows = d_rows ? d_rows + (size_t)(ra - ring0) * rowlen : nullptr;
        if (!rows) {
            HX_TRY(d_rowbuf.alloc(sizeof(double) * rowlen * nr));
            rows = d_rowbuf.as<double>();
        }
        hipLaunchKernelGGL(k_pixwin_rows, dim3(lblocks, nr), dim3(256), 0, st, nside, spin, lmax, A.groups, A.items, d_first.as<int>(), A.partial, rows);
        if (d_w2) hipLaunchKernelGGL(k_pixwin_accumulate, dim3(lblocks), dim3(256), 0, st, nside, lmax, ra, nr, rows, d_w2);
        HX_HIP(hipGetLastError());
        HX_HIP(hipStreamSynchronize(st));  // the item tables are rewritten, the buffers may be reallocated for the next launch
        ra = rb;
    }
    return HX_OK;
}

}  // namespace

}  // namespace hx

using namespace hx;

extern "C" int hx_pixel_window_rings(int nside, int spin, int lmax, int ring_first, int ring_count, double *out)
{
    HX_TRY(ensure_ready());
    HX_TRY(pixwin_check("hx_pixel_window_rings", nside, spin, lmax));
    if (!out) return fail(HX_ERR_ARG, "hx_pixel_window_rings: null output");
    if (ring_first < 1 || ring_count < 0 || ring_count > 2 * nside || ring_first + ring_count - 1 > 2 * nside)
        return fail(HX_ERR_ARG, "hx_pixel_window_rings: rings %d .. %d are not northern rings 1 .. 2 nside = %d", ring_first, ring_first + ring_count - 1, 2 * nside);
    if (ring_count == 0) return HX_OK;
    OutView vout;
    HX_TRY(vout.bind(out, sizeof(double) * ((size_t)lmax + 1) * ring_count));
    HX_TRY(pixwin_run(nside, spin, lmax, ring_first, ring_count, vout.as<double>(), nullptr));
    HX_TRY(vout.finish());
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}

extern "C" int hx_pixel_window(int nside, int spin, int lmax, double *window)
{
    HX_TRY(ensure_ready());
    HX_TRY(pixwin_check("hx_pixel_window", nside, spin, lmax));
    if (!window) return fail(HX_ERR_ARG, "hx_pixel_window: null output");
    OutView vout;
    HX_TRY(vout.bind(window, sizeof(double) * ((size_t)lmax + 1)));
    DevBuf d_w2;
    HX_TRY(d_w2.alloc(sizeof(double) * ((size_t)lmax + 1)));
    hipStream_t st = rt().stream;
    HX_HIP(hipMemsetAsync(d_w2.p, 0, sizeof(double) * ((size_t)lmax + 1), st));
    HX_TRY(pixwin_run(nside, spin, lmax, 1, 2 * nside, nullptr, d_w2.as<double>()));
    hipLaunchKernelGGL(k_pixwin_finish, dim3((unsigned)((lmax + 256) / 256)), dim3(256), 0, st, nside, spin, lmax, d_w2.as<double>(), vout.as<double>());
    HX_HIP(hipGetLastError());
    HX_TRY(vout.finish());
    HX_HIP(hipStreamSynchronize(st));  // d_w2 dies with this scope
    return HX_OK;
}
