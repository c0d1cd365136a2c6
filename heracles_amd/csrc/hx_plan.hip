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
    hx_plan::SpinData *sd = nullptr;
    return spin_data(pl, 0, false, &sd);  // (the spin-0 tables are part of every plan)
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
    for (auto &sp : pl->spins)
        for (auto &kv : sp.second.tasks) {  // lead-in tables: rebuilt by the next sweep that wants one
            kv.second.d_leadin.release();
            kv.second.leadin_skip = false;
        }
    return HX_OK;
}

extern "C" int hx_plan_set_leadin_resume(hx_plan *pl, int on)
{
    if (!pl) return fail(HX_ERR_ARG, "hx_plan_set_leadin_resume: null plan");
    pl->leadin_resume = on < 0 ? 0 : (on > 2 ? 2 : on);
    return HX_OK;
}

extern "C" int hx_plan_set_leadin_cap(hx_plan *pl, int64_t bytes)
{
    if (!pl || bytes < 0) return fail(HX_ERR_ARG, "hx_plan_set_leadin_cap: null plan or negative cap");
    pl->leadin_cap = bytes;
    for (auto &sp : pl->spins)
        for (auto &kv : sp.second.tasks) kv.second.leadin_skip = false;  // (asked again under the new cap)
    return HX_OK;
}

extern "C" int64_t hx_plan_scratch_bytes(const hx_plan *pl)
{
    if (!pl) return 0;
    size_t spin_tables = 0;
    for (const auto &kv : pl->spins) {
        spin_tables += kv.second.cn.bytes + kv.second.al.bytes;
        for (const auto &ts : kv.second.tasks) spin_tables += ts.second.d_leadin.bytes;
    }
    return (int64_t)(pl->stage[0].bytes + pl->stage[1].bytes + pl->stage[2].bytes + pl->resid_maps.bytes + pl->Y.bytes + pl->F.bytes + pl->partial.bytes +
                     pl->bhat.bytes + pl->syn_tab.bytes + spin_tables);
}

extern "C" int hx_plan_last_chunks(const hx_plan *pl) { return pl ? pl->last_chunks : 0; }

// =====================================================================================
// per-spin state: recursion tables, seed factors, task sets
// =====================================================================================
namespace hx {
int spin_data(hx_plan *pl, int spin, bool generic, hx_plan::SpinData **out)
{
    const int lmax = pl->lmax, s = spin;
    if (generic ? (s < 1 || s > lmax) : (s != 0 && s != 2)) return fail(HX_ERR_ARG, "spin_data: spin %d at lmax %d", s, lmax);
    hx_plan::SpinData &sd = pl->spins[{s, generic}];
    *out = &sd;
    if (sd.cn.p && sd.al.p && (sd.kf.p || !generic)) return HX_OK;
    if (generic) {
        // seed factors of spin_seeds, by incremental products like kfac2 (upwards and downwards from m = s, where the factorial ratio is 1):
        //   m >= s: (-1)^m sqrt((2m+1)/4pi) sqrt((2m)!/((m+s)!(m-s)!)) 2^-(m-s);   m < s: sqrt((2s+1)/4pi) sqrt((2s)!/((s+m)!(s-m)!)) 2^-(s-m)
        std::vector<double> kf(lmax + 1);
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
        for (double v : kf)
            if (!std::isfinite(v)) return fail(HX_ERR_UNSUPPORTED, "spin-%d values: the seeds of the recursion leave the range of a double", s);
        HX_TRY(upload(sd.kf, kf));
    }
    hipStream_t st = rt().stream;
    HX_TRY(sd.cn.alloc(sizeof(double2) * (pl->nlm + TABLE_PAD)));
    HX_TRY(sd.al.alloc(sizeof(double) * (pl->nlm + TABLE_PAD)));
    HX_HIP(hipMemsetAsync(sd.cn.p, 0, sizeof(double2) * (pl->nlm + TABLE_PAD), st));
    HX_HIP(hipMemsetAsync(sd.al.p, 0, sizeof(double) * (pl->nlm + TABLE_PAD), st));
    double2 *cn = sd.cn.as<double2>();
    double *al = sd.al.as<double>();
    if (generic) hipLaunchKernelGGL(k_init_norm_s, dim3((lmax + 64) / 64), dim3(64), 0, st, lmax, s, cn, al);
    else if (s == 2) hipLaunchKernelGGL(k_init_norm2, dim3((lmax + 64) / 64), dim3(64), 0, st, lmax, cn, al);
    else hipLaunchKernelGGL(k_init_norm0, dim3((2 * (lmax + 1) + 63) / 64), dim3(64), 0, st, lmax, cn, al);
    HX_HIP(hipGetLastError());
    return HX_OK;
}

// libsharp's published heuristic for the largest m that contributes on a ring
// (sharp_get_mlim): rings with m > mlim are skipped.
int ring_mlim(int lmax, int spin, double sth, double cth)
{
    double ofs = lmax * 0.01;
    if (ofs < 100.) ofs = 100.;
    double b = -2 * spin * fabs(cth);
    double t1 = lmax * sth + ofs;
    double c = (double)spin * spin - t1 * t1;
    double discr = b * b - 4 * c;
    if (discr <= 0) return lmax;
    double res = (-b + sqrt(discr)) / 2.;
    if (res > lmax) res = lmax;
    return (int)(res + 0.5);
}

// The task set of `blocks` ring blocks per task of a spin weight and family, built and uploaded when it is first asked for (the tables are
// not: the flop accounting and hx_ring_modes read task sets only).  Which kernel wants which block count is the kernels' business:
// valu_task_blocks, synth_valu_task_blocks (hx_legendre_valu.hip), one_set_task_blocks, flop_task_blocks (hx_analysis.hip).
int task_set(hx_plan *pl, int spin, bool generic, int blocks, hx_plan::TaskSet **out)
{
    if (spin < 0 || blocks < 1) return fail(HX_ERR_ARG, "task_set: %d ring blocks per task of spin %d", blocks, spin);
    std::map<int, hx_plan::TaskSet> &store = pl->spins[{spin, generic}].tasks;
    const auto it = store.find(blocks);
    if (it != store.end()) {
        *out = &it->second;
        return HX_OK;
    }
    hx_plan::TaskSet &ts = store[blocks];
    const int lmax = pl->lmax;
    const int nrb = (pl->nrp + RBLK - 1) / RBLK;
    ts.of_m.assign(lmax + 1, MTasks{0, 0});
    ts.rows_before_m.assign(lmax + 2, 0);
    ts.arow.assign(lmax + 2, 0);
    long long rows = 0, arows = 0;
    // mlim is monotone in the ring index (pole -> equator): first active ring by bisection
    std::vector<int> mlim(pl->nrp);
    for (int rp = 0; rp < pl->nrp; ++rp) mlim[rp] = ring_mlim(lmax, spin, pl->h_sth[rp], pl->h_z[rp]);
    for (int m = 0; m <= lmax; ++m) {
        ts.rows_before_m[m] = rows;
        ts.arow[m] = arows;
        const int l0 = std::max(m, spin);
        if (l0 <= lmax) arows += (long long)LBLK * ((lmax - l0) / LBLK + 1);
        ts.of_m[m].first = (int)ts.tasks.size();
        if (l0 <= lmax) {
            int first = (int)(std::lower_bound(mlim.begin(), mlim.end(), m) - mlim.begin());
            if (first >= pl->nrp) first = pl->nrp - 1;
            for (int rb = first / RBLK; rb < nrb; rb += blocks) {
                LegTask t;
                t.m = m; t.rb0 = rb; t.nrb = std::min(blocks, nrb - rb); t.pad = 0; t.pout = rows;
                rows += (long long)LBLK * ((lmax - l0) / LBLK + 1);  // padded to whole 32-l blocks (the pipelined kernel stores unconditionally)
                ts.tasks.push_back(t);
            }
        }
        ts.of_m[m].count = (int)ts.tasks.size() - ts.of_m[m].first;
    }
    ts.rows_before_m[lmax + 1] = rows;
    ts.arow[lmax + 1] = arows;
    int rc = upload(ts.d_tasks, ts.tasks);
    if (rc == HX_OK) rc = upload(ts.d_of_m, ts.of_m);
    if (rc == HX_OK) rc = upload(ts.d_arow, ts.arow);
    if (rc != HX_OK) store.erase(blocks);  // (only a complete set stays in the store)
    *out = rc == HX_OK ? &ts : nullptr;
    return rc;
}

// The highest order every ring pair is synthesised for by the batched synthesis: the tasks of an order m start at the 32-ring-pair block
// that holds the first ring with mlim >= m (task_set), so ring pair rp is covered for m <= the largest mlim of its block; the rows beyond
// are never written and the spectrum pass does not read them (no 32 GB memset per sweep of ten fields)
int synth_mlim(hx_plan *pl, int spin, const int **mlim)
{
    hx_plan::SpinData *sd = nullptr;
    HX_TRY(spin_data(pl, spin, false, &sd));
    if (!sd->syn_mlim.p) {
        std::vector<int> h(pl->nrp_pad, -1);
        for (int rp = 0; rp < pl->nrp; ++rp) {
            const int last = std::min(rp / RBLK * RBLK + RBLK - 1, pl->nrp - 1);
            h[rp] = std::min(pl->lmax, ring_mlim(pl->lmax, spin, pl->h_sth[last], pl->h_z[last]));
        }
        HX_TRY(upload(sd->syn_mlim, h));
    }
    *mlim = sd->syn_mlim.as<int>();
    return HX_OK;
}
}  // namespace hx
