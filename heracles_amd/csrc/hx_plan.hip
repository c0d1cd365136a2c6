// hx_plan.hip -- the plan of the HEALPix transforms (and of the equiangular rings of the point transform): ring geometry,
// the tables that depend on the band limit only (twiddles, seeds and coefficients of the normalised recursions) and the
// plan's scratch.  What the ring Fourier stage needs of a plan -- FFT classes, Bluestein filters, kernel attributes -- is set
// up by ring_fft_plan_init (hx_ring_fft.hip).  Pipeline overview: hx_sht_common.h.
#include <algorithm>
#include <cmath>

#include "hx_sht_common.h"

namespace hx {
// =====================================================================================
// table initialisation kernels
// =====================================================================================
// Normalised recursions used by the analysis kernel (two FMAs per new value, after the
// scheme of libsharp/ducc's Ylmgen): with lambda_l = alpha_l mu_l,
//   spin 0 (two-step):  mu_{l+2} = (A' x^2 + B') mu_l - mu_{l-2}
//       A = a_{l+1} a_{l+2},  B = -(a_{l+2}/a_{l+1} + a_{l+2} a_{l+1}/a_l^2),  a_l = sqrt((4l^2-1)/(l^2-m^2)),
//       alpha_{l+2} alpha_l = a_{l+2} a_{l+1} / 4,   A' = A alpha_l/alpha_{l+2},  B' likewise;
//       coef[idx(l,m)] = (A', B') is indexed by the SOURCE l, alpha[idx(l,m)] = alpha_l.
//   spin 2 (one-step):  mu_{l+1} = (p' x +- q') mu_l - mu_{l-1}   (+ for d^l_{m,-2}, - for d^l_{m,+2})
//       alpha_{l+1} = r_l alpha_{l-1},  p' = p alpha_l/alpha_{l+1},  q' likewise;
//       coef[idx(l+1,m)] = (p', q') is indexed by the TARGET l.
// One thread per (m, chain): the alpha recursion is sequential in l.
__global__ void k_init_norm0(int lmax, double2 *__restrict__ coef, double *__restrict__ alpha)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int m = t >> 1, par = t & 1;
    if (m > lmax) return;
    const double dm = m;
    auto a = [dm](double l) { return sqrt((4.0 * l * l - 1.0) / (l * l - dm * dm)); };
    double al = 1.0;
    for (int l = m + par; l <= lmax; l += 2) {
        const double dl = l;
        const double a1 = a(dl + 1.0), a2 = a(dl + 2.0);
        const double A = a1 * a2;
        double B = -a2 / a1;
        if (l > m) {
            const double a0 = a(dl);
            B -= a2 * a1 / (a0 * a0);
        }
        const double an = 0.25 * a2 * a1 / al;
        coef[almidx(lmax, l, m)] = make_double2(A * al / an, B * al / an);
        alpha[almidx(lmax, l, m)] = al;
        al = an;
    }
}

__global__ void k_init_norm2(int lmax, double2 *__restrict__ coef, double *__restrict__ alpha)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m > lmax) return;
    const int l0 = m > 2 ? m : 2;
    double am1 = 1.0, a0 = 1.0;  // alpha_{l-1}, alpha_l
    for (int l = l0; l <= lmax; ++l) {
        alpha[almidx(lmax, l, m)] = a0;
        if (l == lmax) break;
        // coefficients of the step l -> l+1 (n = -2)
        const double k = l, lp = l + 1.0, dm = m, dn = -2.0;
        const double den = k * sqrt((lp * lp - dm * dm) * (lp * lp - dn * dn));
        const double r1 = sqrt((2.0 * k + 3.0) / (2.0 * k + 1.0));
        const double p = r1 * (2.0 * k + 1.0) * k * lp / den;
        const double q = -r1 * (2.0 * k + 1.0) * dm * dn / den;
        double a1 = 1.0;
        if (l > l0) {
            const double r2 = sqrt((2.0 * k + 3.0) / (2.0 * k - 1.0));
            const double r = r2 * lp * sqrt((k * k - dm * dm) * (k * k - dn * dn)) / den;
            a1 = r * am1;
        }
        coef[almidx(lmax, l + 1, m)] = make_double2(p * a0 / a1, q * a0 / a1);
        am1 = a0;
        a0 = a1;
    }
}

// k_init_norm2 for a spin weight s >= 1: the same one-step recursion with n = -s in place of -2, from l0 = max(m, s).  The (+s)
// chain runs with (p', +q'), the (-s) chain with (p', -q'): one table serves both.
__global__ void k_init_norm_s(int lmax, int s, double2 *__restrict__ coef, double *__restrict__ alpha)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m > lmax) return;
    const int l0 = m > s ? m : s;
    double am1 = 1.0, a0 = 1.0;  // alpha_{l-1}, alpha_l
    for (int l = l0; l <= lmax; ++l) {
        alpha[almidx(lmax, l, m)] = a0;
        if (l == lmax) break;
        // coefficients of the step l -> l+1 (n = -s)
        const double k = l, lp = l + 1.0, dm = m, dn = -(double)s;
        const double den = k * sqrt((lp * lp - dm * dm) * (lp * lp - dn * dn));
        const double r1 = sqrt((2.0 * k + 3.0) / (2.0 * k + 1.0));
        const double p = r1 * (2.0 * k + 1.0) * k * lp / den;
        const double q = -r1 * (2.0 * k + 1.0) * dm * dn / den;
        double a1 = 1.0;
        if (l > l0) {
            const double r2 = sqrt((2.0 * k + 3.0) / (2.0 * k - 1.0));
            const double r = r2 * lp * sqrt((k * k - dm * dm) * (k * k - dn * dn)) / den;
            a1 = r * am1;
        }
        coef[almidx(lmax, l + 1, m)] = make_double2(p * a0 / a1, q * a0 / a1);
        am1 = a0;
        a0 = a1;
    }
}
}  // namespace hx

using namespace hx;

// =====================================================================================
// plan
// =====================================================================================
PlanDev hx_plan::dev() const
{
    PlanDev P;
    P.nside = nside; P.lmax = lmax; P.nrp = nrp; P.nrp_pad = nrp_pad; P.twN = twN;
    P.npix = npix; P.ny = ny;
    P.z = z.as<double>(); P.omz = omz.as<double>(); P.sth = sth.as<double>(); P.rwdef = rwdef.as<double>();
    P.nsub = nsub.as<int>(); P.shifted = shifted.as<int>();
    P.startN = startN.as<long long>(); P.startS = startS.as<long long>(); P.bhat_off = bhat_off.as<long long>();
    P.tw = tw.as<double2>(); P.bhat = bhat.as<double2>();
    P.mfac = mfac.as<double>(); P.kfac2 = kfac2.as<double>();
    P.rec0 = nullptr; P.rec2 = nullptr;
    P.wnorm = wnorm; P.hsrc = hsrc; P.hsrc_stride = hsrc_stride; P.hN = eqN;
    P.nssrc = nssrc; P.ns_m0 = ns_m0; P.ns_ms = m_step;
    return P;
}

// Tables that depend on the band limit only (twiddles of the in-LDS FFT, seeds and coefficients of the recursions): shared by
// the HEALPix plan and the equiangular plan of the point transform (hx_nufft.hip).
static int plan_tables(hx_plan *pl)
{
    const int lmax = pl->lmax;
    std::vector<double2> tw(std::max(pl->twN / 2, 64));  // load_tw_factored copies 64 entries whatever twN
    for (int k = 0; k < (int)tw.size(); ++k) {
        long double a = -2.0L * 3.141592653589793238462643383279502884L * k / pl->twN;
        tw[k].x = (double)cosl(a); tw[k].y = (double)sinl(a);
    }
    // mfac[m] = (-1)^m sqrt((2m+1)/(4pi) prod_{k<=m} (2k-1)/(2k));  kfac2[m] = K_m 2^-(m-2)
    std::vector<double> mfac(lmax + 1), kfac2(lmax + 3, 0.0);
    {
        long double p = 1.0L;
        for (int m = 0; m <= lmax; ++m) {
            if (m > 0) p *= (2.0L * m - 1.0L) / (2.0L * m);
            long double v = sqrtl((2.0L * m + 1.0L) / (4.0L * 3.141592653589793238462643383279502884L) * p);
            mfac[m] = (double)((m & 1) ? -v : v);
        }
        long double k = 1.0L;
        for (int m = 2; m <= lmax + 2; ++m) {
            if (m > 2) k *= sqrtl((2.0L * m) * (2.0L * m - 1.0L) / ((m - 2.0L) * (m + 2.0L))) / 2.0L;
            kfac2[m] = (double)k;
        }
    }
    HX_TRY(upload(pl->tw, tw));
    HX_TRY(upload(pl->mfac, mfac));
    HX_TRY(upload(pl->kfac2, kfac2));
    hipStream_t st = rt().stream;
    HX_TRY(pl->cn0.alloc(sizeof(double2) * (pl->nlm + TABLE_PAD)));
    HX_TRY(pl->al0.alloc(sizeof(double) * (pl->nlm + TABLE_PAD)));
    HX_HIP(hipMemsetAsync(pl->cn0.p, 0, sizeof(double2) * (pl->nlm + TABLE_PAD), st));
    HX_HIP(hipMemsetAsync(pl->al0.p, 0, sizeof(double) * (pl->nlm + TABLE_PAD), st));
    hipLaunchKernelGGL(k_init_norm0, dim3((2 * (lmax + 1) + 63) / 64), dim3(64), 0, st, lmax, pl->cn0.as<double2>(), pl->al0.as<double>());
    HX_HIP(hipGetLastError());
    return HX_OK;
}

extern "C" hx_plan *hx_plan_create(int nside, int lmax, int max_comp)
{
    if (ensure_ready() != HX_OK) return nullptr;
    if (nside < 1 || lmax < 0 || max_comp < 1) {
        set_error("hx_plan_create: bad argument");
        return nullptr;
    }
    hx_plan *pl = new hx_plan;
    pl->nside = nside; pl->lmax = lmax; pl->max_comp = max_comp;
    pl->npix = 12LL * nside * nside;
    pl->nrp = 2 * nside;
    pl->nrp_pad = (pl->nrp + 63) / 64 * 64;
    pl->nlm = (long long)(lmax + 1) * (lmax + 2) / 2;
    pl->wnorm = 4.0 * M_PI / (double)pl->npix;
    const long long ns = nside, ncap = 2 * ns * (ns - 1);
    std::vector<double> z(pl->nrp), omz(pl->nrp), sth(pl->nrp), rw(pl->nrp, 1.0);
    std::vector<int> nsub(pl->nrp), shifted(pl->nrp);
    std::vector<long long> sN(pl->nrp), sS(pl->nrp);
    const double fact2 = 4.0 / (double)pl->npix, fact1 = (double)(2 * ns) * fact2;
    int maxM = 1;
    for (int rp = 0; rp < pl->nrp; ++rp) {
        const int i = rp + 1;
        if (i < nside) {
            double tmp = (double)i * (double)i * fact2;
            z[rp] = 1.0 - tmp; omz[rp] = tmp; sth[rp] = sqrt(tmp * (2.0 - tmp));
            nsub[rp] = i; sN[rp] = 2LL * i * (i - 1); shifted[rp] = 1;
        } else {
            z[rp] = (double)(2 * nside - i) * fact1; omz[rp] = 1.0 - z[rp];
            sth[rp] = sqrt((1.0 - z[rp]) * (1.0 + z[rp]));
            nsub[rp] = nside; sN[rp] = ncap + (long long)(i - nside) * 4 * ns;
            shifted[rp] = ((i - nside) & 1) == 0;
        }
        sS[rp] = i == 2 * nside ? -1 : pl->npix - sN[rp] - 4LL * nsub[rp];
        maxM = std::max(maxM, fft_size_for(nsub[rp]));
    }
    pl->ny = sN[pl->nrp - 1] + 4LL * nsub[pl->nrp - 1];
    pl->twN = std::max(maxM, 2);
    pl->h_sth = sth; pl->h_z = z; pl->h_nsub = nsub; pl->h_startN = sN; pl->h_startS = sS;
    int rc = HX_OK;
    auto chk = [&](int r) { if (rc == HX_OK) rc = r; };
    chk(upload(pl->z, z)); chk(upload(pl->omz, omz)); chk(upload(pl->sth, sth)); chk(upload(pl->rwdef, rw));
    chk(upload(pl->nsub, nsub)); chk(upload(pl->shifted, shifted));
    chk(upload(pl->startN, sN)); chk(upload(pl->startS, sS));
    // (the ring Fourier stage comes last: its Bluestein filters are transformed with the twiddles of plan_tables)
    if (rc != HX_OK || plan_tables(pl) != HX_OK || ring_fft_plan_init(pl, nsub, sN, sS) != HX_OK) { delete pl; return nullptr; }
    if (hipStreamSynchronize(rt().stream) != hipSuccess || hipGetLastError() != hipSuccess) {
        set_error("hx_plan_create: table initialisation failed");
        delete pl;
        return nullptr;
    }
    return pl;
}

// Plan of the Legendre stages on N / 2 equidistant rings theta_j = 2 pi (j + 1/2) / N, j < N / 2 (N a multiple of 4): ring pair
// r < N / 4 = (theta_r, pi - theta_r), pole -> equator like the HEALPix pairs.  It has no pixels: its ring spectra h_m(theta_j)
// come from the non-uniform Fourier stage of the point transform (hx_nufft.hip), which owns the plan.
hx_plan *hx::plan_create_equiangular(int N, int lmax)
{
    if (N < 4 || (N & 3) || lmax < 0 || 2 * lmax + 1 >= N) {
        set_error("equiangular plan: N=%d lmax=%d", N, lmax);
        return nullptr;
    }
    hx_plan *pl = new hx_plan;
    pl->nside = 0; pl->lmax = lmax; pl->max_comp = 16;
    pl->npix = 0; pl->ny = 0;
    pl->eqN = N;
    pl->wnorm = 1.0 / N;
    pl->nrp = N / 4;
    pl->nrp_pad = (pl->nrp + 63) / 64 * 64;
    pl->nlm = (long long)(lmax + 1) * (lmax + 2) / 2;
    std::vector<double> z(pl->nrp), omz(pl->nrp), sth(pl->nrp), rw(pl->nrp, 1.0);
    for (int r = 0; r < pl->nrp; ++r) {
        const long double t = 2.0L * 3.141592653589793238462643383279502884L * (r + 0.5L) / N;
        const long double sh = sinl(0.5L * t);
        z[r] = (double)cosl(t); omz[r] = (double)(2.0L * sh * sh); sth[r] = (double)sinl(t);
    }
    pl->h_sth = sth; pl->h_z = z;
    pl->twN = 2;
    int rc = HX_OK;
    auto chk = [&](int r) { if (rc == HX_OK) rc = r; };
    chk(upload(pl->z, z)); chk(upload(pl->omz, omz)); chk(upload(pl->sth, sth)); chk(upload(pl->rwdef, rw));
    if (rc != HX_OK || plan_tables(pl) != HX_OK || hipStreamSynchronize(rt().stream) != hipSuccess) { delete pl; return nullptr; }
    return pl;
}

extern "C" void hx_plan_destroy(hx_plan *plan)
{
    if (!plan) return;
    if (rt().ready) (void)hipStreamSynchronize(rt().stream);
    for (int i = 0; i < hx_plan::NSTAGE; ++i) {
        if (plan->stage_done[i]) (void)hipEventDestroy(plan->stage_done[i]);
    }
    for (int i = 0; i < hx_plan::NUNIT_EV; ++i)
        if (plan->unit_up[i]) (void)hipEventDestroy(plan->unit_up[i]);
    delete plan;
}

extern "C" int hx_plan_release_scratch(hx_plan *pl)
{
    if (!pl) return fail(HX_ERR_ARG, "hx_plan_release_scratch: null plan");
    if (rt().ready) {
        HX_HIP(hipStreamSynchronize(rt().stream));
        if (rt().copy) HX_HIP(hipStreamSynchronize(rt().copy));
    }
    for (int i = 0; i < hx_plan::NSTAGE; ++i) pl->stage[i].release();
    pl->resid_maps.release();
    pl->Y.release();
    pl->F.release();
    pl->partial.release();
    pl->syn_tab.release();
    return HX_OK;
}

extern "C" int64_t hx_plan_scratch_bytes(const hx_plan *pl)
{
    if (!pl) return 0;
    size_t spin_tables = 0;
    for (const auto &kv : pl->spin_sets) spin_tables += kv.second.cn.bytes + kv.second.al.bytes;
    return (int64_t)(pl->stage[0].bytes + pl->stage[1].bytes + pl->stage[2].bytes + pl->resid_maps.bytes + pl->Y.bytes + pl->F.bytes + pl->partial.bytes + pl->rec0.bytes + pl->rec2.bytes + pl->cn0.bytes + pl->al0.bytes + pl->cn2.bytes + pl->al2.bytes +
                     pl->bhat.bytes + pl->syn_tab.bytes + spin_tables);
}

extern "C" int hx_plan_last_chunks(const hx_plan *pl) { return pl ? pl->last_chunks : 0; }

namespace hx {
int ensure_rec2(hx_plan *pl)
{
    if (pl->cn2.p) return HX_OK;
    HX_TRY(pl->cn2.alloc(sizeof(double2) * (pl->nlm + TABLE_PAD)));
    HX_TRY(pl->al2.alloc(sizeof(double) * (pl->nlm + TABLE_PAD)));
    HX_HIP(hipMemsetAsync(pl->cn2.p, 0, sizeof(double2) * (pl->nlm + TABLE_PAD), rt().stream));
    HX_HIP(hipMemsetAsync(pl->al2.p, 0, sizeof(double) * (pl->nlm + TABLE_PAD), rt().stream));
    hipLaunchKernelGGL(k_init_norm2, dim3((pl->lmax + 64) / 64), dim3(64), 0, rt().stream, pl->lmax, pl->cn2.as<double2>(), pl->al2.as<double>());
    HX_HIP(hipGetLastError());
    return HX_OK;
}

int ensure_rec_s(hx_plan *pl, int s, hx_plan::SpinSet **out)
{
    const int lmax = pl->lmax;
    if (s < 1 || s > lmax) return fail(HX_ERR_ARG, "ensure_rec_s: spin %d at lmax %d", s, lmax);
    hx_plan::SpinSet &set = pl->spin_sets[s];
    *out = &set;
    if (set.cn.p && set.al.p && set.kf.p) return HX_OK;
    // seed factors of spin_seeds, by incremental products like kfac2 (upwards and downwards from m = s, where the factorial ratio is 1):
    //   m >= s: (-1)^m sqrt((2m+1)/4pi) sqrt((2m)!/((m+s)!(m-s)!)) 2^-(m-s);   m < s: sqrt((2s+1)/4pi) sqrt((2s)!/((s+m)!(s-m)!)) 2^-(s-m)
    std::vector<double> kf(lmax + 1);
    {
        const long double fourpi = 4.0L * 3.141592653589793238462643383279502884L;
        long double k = 1.0L;
        for (int m = s; m <= lmax; ++m) {
            if (m > s) k *= sqrtl((2.0L * m) * (2.0L * m - 1.0L) / ((long double)(m - s) * (m + s))) / 2.0L;
            const long double v = k * sqrtl((2.0L * m + 1.0L) / fourpi);
            kf[m] = (double)((m & 1) ? -v : v);
        }
        k = sqrtl((2.0L * s + 1.0L) / fourpi);
        for (int m = s - 1; m >= 0; --m) {
            k *= sqrtl((long double)(s + m + 1) / (s - m)) / 2.0L;
            kf[m] = (double)k;
        }
    }
    for (double v : kf)
        if (!std::isfinite(v)) return fail(HX_ERR_UNSUPPORTED, "spin-%d values: the seeds of the recursion leave the range of a double", s);
    HX_TRY(upload(set.kf, kf));
    HX_TRY(set.cn.alloc(sizeof(double2) * (pl->nlm + TABLE_PAD)));
    HX_TRY(set.al.alloc(sizeof(double) * (pl->nlm + TABLE_PAD)));
    HX_HIP(hipMemsetAsync(set.cn.p, 0, sizeof(double2) * (pl->nlm + TABLE_PAD), rt().stream));
    HX_HIP(hipMemsetAsync(set.al.p, 0, sizeof(double) * (pl->nlm + TABLE_PAD), rt().stream));
    hipLaunchKernelGGL(k_init_norm_s, dim3((lmax + 64) / 64), dim3(64), 0, rt().stream, lmax, s, set.cn.as<double2>(), set.al.as<double>());
    HX_HIP(hipGetLastError());
    return HX_OK;
}
}  // namespace hx
