// hx_rotate.hip -- rotation of spherical-harmonic coefficients by any Euler angles: a'_lm = sum_m' exp(-i m phi) d^l_mm'(theta)
// exp(-i m' psi) a_lm', d^l(theta) = exp(-i theta J_y) in the Condon-Shortley basis.  gfx950 only.
//
//   k_rotate_alm    the hot path.  A work-group is ROT_MO waves and owns ROT_MO consecutive output columns m >= 0 for up to ROT_CB
//                   components.  It walks the input orders in blocks of ROT_MB pairs (+m', -m'), m' = |m'| ascending, and each block
//                   in tiles of ROT_LB multipoles:
//                     generate    wave = column, lane = pair.  Both chains d^l_{m,+m'} and d^l_{m,-m'} advance ROT_LB steps of the upward three-term
//                                 recurrence in l from l0 = max(m, m'); they share sqrt((l^2 - m^2)(l^2 - m'^2)), computed on the fly
//                                 as one rsqrt per step.  A chain is (mantissa, binary exponent): the seed
//                                 sqrt(C(2A, A+B)) cos^(A+B)(theta/2) sin^(A-B)(theta/2) comes from a log2 sum in double-double
//                                 (host tables of log2 k!, log2 cos, log2 sin), is split into exp2(fraction) and an integer, and the
//                                 pair is renormalised at every tile end.  What the tile gets is ldexp(mantissa, exponent): zero
//                                 while the chain is below the range of a double.  The pair is stored combined,
//                                 e = d+ + (-1)^m' d-, f = d+ - (-1)^m' d-, so that with c = exp(-i m' psi) a_lm'
//                                 b_lm += e Re c + i f Im c covers a_lm' and a_l,-m' = (-1)^m' conj(a_lm').
//                     accumulate  lane = (quarter of the pairs, l of the tile); a wave serves one component and the columns dealt to
//                                 it, so that an input coefficient is read once for all of them.  The tiles are read transposed
//                                 from LDS, the psi phase is folded into (e, f), a (column, component) takes four fmas per pair; the
//                                 four quarters are added by two xor shuffles (a fixed tree), multiplied by exp(-i m phi) and added
//                                 to the output column by the lane that owns that l in every tile.
//                   One work-group adds the contributions of a column in one order and one thread owns an output coefficient
//                   throughout: no atomics on the data, the same bits every call, and a (column, component) pair gets the same
//                   operations whatever batch it sits in.
//   Below sin(theta) = ROT_SPLIT_SIN the entry point rotates twice, by (psi, pi/2, 0) and (0, theta - pi/2, phi), through a scratch
//   alm: d^l(theta) = d^l(pi/2) d^l(theta - pi/2), and FP64 chains lose 1 / sin(theta) of their accuracy.
//   k_rotate_phase  theta = 0 and theta = pi: d = delta_mm' and d^l_mm'(pi) = (-1)^(l-m') delta_m,-m' leave one phase per order.
#include <climits>
#include <cmath>

#include "hx_common.h"
#include "hx_dd.h"

namespace hx {

constexpr int ROT_CB = 4;   // components per block of a work-group (blockIdx.y)
constexpr int ROT_MO = 4;   // output columns m per work-group: its waves
constexpr int ROT_MB = 64;  // pairs (+m', -m') per block: the lanes of the generate phase
constexpr int ROT_LB = 16;  // multipoles per tile
constexpr int ROT_LMAX = 32000;  // (l + 1 - m)(l + 1 + m) is formed in 32-bit integers
// below this sin(theta) a rotation is done as two, by pi/2 and theta - pi/2 (where the FP64 chains of one pass keep a
// quarter of the 1e-12 contract at lmax 6144)
constexpr long double ROT_SPLIT_SIN = 0.1L;
// flops of one pair step of the recurrence (two chains: coefficient 5, fma and product 3, scale 1 each; shared: the products for the
// square root's argument, its carry and the second coefficient 3, the combination (e, f) 4; the rsqrt itself is not counted) and of
// one (pair, l, component) of the accumulation (four fmas)
constexpr int ROT_FLOPS_STEP = 25;
constexpr int ROT_FLOPS_ACC = 8;

__device__ unsigned long long g_rot_flops;

namespace {

struct RotParams {
    int lmax;
    double xh, xl;         // cos(theta) = xh + xl
    DD lc, ls;              // log2 cos(theta/2), log2 sin(theta/2)
    const double2 *lf;      // log2 k! as (hi, lo), k = 0 .. 2 lmax
    const double2 *ppsi;    // exp(-i m' psi), m' = 0 .. lmax
    const double2 *pphi;    // exp(-i m phi)
};

__device__ __forceinline__ long long alm_idx(int lmax, int l, int m) { return (long long)m * (2 * lmax + 1 - m) / 2 + l; }

// a log2 value (hi + lo) as a mantissa in [1, 2] and an integer exponent
__device__ __forceinline__ double split_log2(DD lg, int *e)
{
    const double n = floor(lg.h);
    *e = (int)n;
    return exp2((lg.h - n) + lg.l);
}

// A work-group is ROT_MO waves and owns ROT_MO consecutive output columns m0 .. m0 + ROT_MO - 1 for nc <= ROT_CB components (in, out:
// the first of them).  Generate: wave w runs the chains of column m0 + w into its own tile.  Accumulate: the (column, component)
// pairs are dealt to the waves so that a wave reads each input coefficient once for all the columns it serves: with four components
// wave w takes component w for all four columns, with two it takes component w & 1 for two columns, with one it takes column w.  A
// (column, component) pair goes through the same operations whatever nc is.
__global__ __launch_bounds__(ROT_MO * ROT_MB) void k_rotate_alm(RotParams P, int ncomp, const double2 *__restrict__ in, double2 *out)
{
    // (e, f) of (column, l of the tile, pair); the pair index is xor-ed with the row so that the transposed read is free of bank conflicts
    __shared__ double2 tile[ROT_MO][ROT_LB][ROT_MB];
    const int lane = threadIdx.x & (ROT_MB - 1), w = threadIdx.x / ROT_MB;
    const int m0 = blockIdx.x * ROT_MO, c0 = blockIdx.y * ROT_CB, nc = min(ROT_CB, ncomp - c0);
    const int lmax = P.lmax, m = m0 + w;  // this wave's column of the generate phase (none if m > lmax)
    const long long nlm = (long long)(lmax + 1) * (lmax + 2) / 2;
    const int j = lane & (ROT_LB - 1), q = lane / ROT_LB;  // accumulate: multipole of the tile, quarter of the pairs
    constexpr int NQ = ROT_MB / ROT_LB, QP = ROT_MB / NQ;   // quarters, pairs per quarter
    static_assert(NQ == 4 && ROT_MO == 4 && ROT_CB == 4, "the shuffle tree and the deal of (column, component) pairs are written for fours");
    // accumulate: component cw, columns [i0, i1) of the group
    const int cw = nc == 1 ? 0 : nc == 2 ? (w & 1) : w;
    const int i0 = nc == 1 ? w : nc == 2 ? 2 * (w >> 1) : 0;
    const int i1 = nc == 1 ? w + 1 : nc == 2 ? i0 + 2 : (w < nc ? ROT_MO : 0);
    unsigned long long nstep = 0, nacc = 0;

    for (int p0 = 0; p0 <= lmax; p0 += ROT_MB) {
        const int p = p0 + lane;  // |m'| of this lane's pair
        const bool live = p <= lmax && m <= lmax;
        const int l0 = live ? max(m, p) : INT_MAX;
        double sdp = 0.0, sdm = 0.0;  // seeds: mantissas with sign
        int sep = 0, sem = 0;         // and exponents
        if (live) {
            const int ia = m + p, ib = abs(m - p);
            const double2 f2 = P.lf[2 * l0], fa = P.lf[ia], fb = P.lf[ib];
            DD bin = dd_add(DD{f2.x, f2.y}, dd_neg(dd_add(DD{fa.x, fa.y}, DD{fb.x, fb.y})));
            bin.h *= 0.5;
            bin.l *= 0.5;
            const DD da = DD{(double)ia, 0.0}, db = DD{(double)ib, 0.0};
            sdp = split_log2(dd_add(bin, dd_add(dd_mul(da, P.lc), dd_mul(db, P.ls))), &sep);
            if (p <= m && ((m - p) & 1)) sdp = -sdp;
            if (p > 0) {
                sdm = split_log2(dd_add(bin, dd_add(dd_mul(db, P.lc), dd_mul(da, P.ls))), &sem);
                if ((m + p) & 1) sdm = -sdm;
            }
        }
        const double mp = (double)m * (double)p, sg = (p & 1) ? -1.0 : 1.0;
        double dcp = 0.0, dpp = 0.0, dcm = 0.0, dpm = 0.0, sl = 0.0;  // d^l and d^(l-1) of both chains, sqrt((l^2-m^2)(l^2-m'^2))
        int ep = 0, em = 0;
        const int lfirst = p0 > m0 ? m0 + (p0 - m0) / ROT_LB * ROT_LB : m0;  // tiles are aligned to m0: one lane owns an output l throughout

        for (int lb = lfirst; lb <= lmax; lb += ROT_LB) {
            const double rl_mine = lb + j > 0 ? 1.0 / (double)(lb + j) : 0.0;  // 1 / l of the tile's multipoles, handed round by shuffles
            __syncthreads();  // (the tiles are free: every wave has read what it needed of the last ones)
            // ---- generate: ROT_LB steps of both chains, (e, f) into the tile (unrolled by 4: the full unroll spills scalar registers)
#pragma unroll 4
            for (int t = 0; t < ROT_LB; ++t) {
                const int l = lb + t;
                if (l == l0) {
                    dcp = sdp; dcm = sdm; ep = sep; em = sem;
                }
                const double vp = ldexp(dcp, ep), vm = ldexp(dcm, em);
                tile[w][t][lane ^ t] = make_double2(fma(sg, vm, vp), fma(-sg, vm, vp));
                // l -> l + 1:  s_(l+1) d^(l+1) = ((2l+1)/l) (l(l+1) x - m m') d^l - ((l+1)/l) s_l d^(l-1),  s_l^2 = (l^2 - m^2)(l^2 - m'^2).
                // l(l+1) x - m m' cancels to a small remainder for m ~ m' ~ l at small theta.  x = xh + xl with xh a multiple of 2^-22
                // (the host's split): the inner fma is exact, the outer rounds the difference once (at l = 0, m = m' = 0: d^1 = x d^0)
                const bool on = l >= l0;
                const double rl = __shfl(rl_mine, t), lp1 = (double)(l + 1);
                const double nn = l > 0 ? (double)l * lp1 : 1.0, h2 = l > 0 ? (double)(2 * l + 1) * rl : 1.0, g3 = lp1 * rl;
                const double p1 = on ? (double)((l + 1 - m) * (l + 1 + m)) * (double)((l + 1 - p) * (l + 1 + p)) : 1.0;
                const double r1 = rsqrt(p1);
                const double g3s = g3 * sl;
                const double ap = h2 * fma(nn, P.xl, fma(nn, P.xh, -mp)), am = h2 * fma(nn, P.xl, fma(nn, P.xh, mp));
                const double np = r1 * fma(ap, dcp, -g3s * dpp);
                const double nm = r1 * fma(am, dcm, -g3s * dpm);
                dpp = dcp; dcp = np;
                dpm = dcm; dcm = nm;
                sl = on ? p1 * r1 : 0.0;
                nstep += on && l < lmax ? 1 : 0;
            }
            {   // renormalise: at most 2^15 of growth per step, so a tile stays far inside the range
                int kp, km;
                (void)frexp(fmax(fabs(dcp), fabs(dpp)), &kp);
                (void)frexp(fmax(fabs(dcm), fabs(dpm)), &km);
                dcp = ldexp(dcp, -kp); dpp = ldexp(dpp, -kp); ep += kp;
                dcm = ldexp(dcm, -km); dpm = ldexp(dpm, -km); em += km;
            }
            __syncthreads();
            // ---- accumulate: this lane's l, its quarter of the pairs, component cw into the columns [i0, i1).
            // No branch on the lane in the loop, so that the loads of several pairs are in flight together: where m' > l the chains
            // have not begun and the tiles hold zeros, so the address is clamped to a valid one (m' = l) and the term adds nothing;
            // lanes past lmax work on l = lmax and store nothing.
            if (i0 < i1) {
                const int l = lb + j, lc = min(l, lmax), pq = p0 + q * QP;
                const double2 *src = in + (long long)(c0 + cw) * nlm;
                double ar[ROT_MO], ai[ROT_MO];
#pragma unroll
                for (int i = 0; i < ROT_MO; ++i) ar[i] = ai[i] = 0.0;
#pragma unroll 4
                for (int k = 0; k < QP; ++k) {
                    const int pm = min(pq + k, lc);  // m' of the pair
                    const double2 ph = P.ppsi[pm];
                    double2 a = src[alm_idx(lmax, lc, pm)];
                    if (pm == 0) a.y = 0.0;  // a_l0 of a real field
#pragma unroll
                    for (int i = 0; i < ROT_MO; ++i) {
                        if (i >= i0 && i < i1) {
                            const double2 ef = tile[i][j][(q * QP + k) ^ j];
                            const double er = ef.x * ph.x, ei = ef.x * ph.y, fr = ef.y * ph.x, fi = ef.y * ph.y;
                            // c = ph a;  b += e Re c + i f Im c
                            ar[i] = fma(-ei, a.y, fma(er, a.x, ar[i]));
                            ai[i] = fma(fi, a.x, fma(fr, a.y, ai[i]));
                        }
                    }
                }
                nacc += l <= lmax ? (unsigned)(min(max(l - pq + 1, 0), QP) * (i1 - i0)) : 0u;
#pragma unroll
                for (int i = 0; i < ROT_MO; ++i) {
                    if (i >= i0 && i < i1) {
                        ar[i] += __shfl_xor(ar[i], ROT_LB);
                        ai[i] += __shfl_xor(ai[i], ROT_LB);
                        ar[i] += __shfl_xor(ar[i], 2 * ROT_LB);
                        ai[i] += __shfl_xor(ai[i], 2 * ROT_LB);
                        const int mo = m0 + i;  // the output column
                        if (q == 0 && l <= lmax && mo <= l) {
                            const double2 phm = P.pphi[mo];
                            double2 *o = out + (long long)(c0 + cw) * nlm + alm_idx(lmax, l, mo);
                            const double br = ar[i], bi = mo == 0 ? 0.0 : ai[i];
                            double2 v = make_double2(fma(-bi, phm.y, br * phm.x), fma(bi, phm.x, br * phm.y));
                            if (p0 > 0) {  // the first block of pairs reaches every l of the column and starts the sum
                                const double2 prev = *o;
                                v.x += prev.x;
                                v.y += prev.y;
                            }
                            if (mo == 0) v.y = 0.0;
                            *o = v;
                        }
                    }
                }
            }
        }
    }
    // executed flops: one integer atomic per wave
    unsigned long long fl = nstep * ROT_FLOPS_STEP + nacc * (unsigned long long)(4 + ROT_FLOPS_ACC);
    for (int s = 32; s > 0; s >>= 1) fl += __shfl_xor(fl, s);
    if (lane == 0) atomicAdd(&g_rot_flops, fl);
}

// out = (-1)^l? conj? of a_lm times ph[m]: theta = 0 (flip = 0) and theta = pi (flip = 1: (-1)^l conj(a_lm))
__global__ __launch_bounds__(256) void k_rotate_phase(int lmax, int flip, const double2 *__restrict__ ph, const double2 *__restrict__ in,
                                                      double2 *__restrict__ out)
{
    const int m = blockIdx.y, l = m + blockIdx.x * 256 + threadIdx.x;
    if (l > lmax) return;
    const long long at = (long long)blockIdx.z * ((long long)(lmax + 1) * (lmax + 2) / 2) + alm_idx(lmax, l, m);
    double2 a = in[at];
    if (m == 0) a.y = 0.0;
    if (flip) {
        a.y = -a.y;
        if (l & 1) a = make_double2(-a.x, -a.y);
    }
    const double2 w = ph[m];
    double2 o = make_double2(fma(-a.y, w.y, a.x * w.x), fma(a.y, w.x, a.x * w.y));
    if (m == 0) o.y = 0.0;
    out[at] = o;
}

const long double PI_L = 3.141592653589793238462643383279502884L;

// exp(-i m alpha), m = 0 .. lmax, from the host's long doubles (m alpha in a double loses 1e-16 m |alpha| of the phase)
std::vector<double2> phase_table(int lmax, long double alpha)
{
    std::vector<double2> t((size_t)lmax + 1);
    for (int m = 0; m <= lmax; ++m) t[m] = make_double2((double)cosl(m * alpha), (double)-sinl(m * alpha));
    t[0] = make_double2(1.0, 0.0);
    return t;
}

double2 split_ld(long double v)
{
    const double h = (double)v;
    return make_double2(h, (double)(v - h));
}

// The tables and parameters of one launch of k_rotate_alm: a rotation by long-double angles, theta in [-pi, pi] (a negative theta
// is folded as in the entry point).  The buffers live until the caller's call is over.
struct RotTables {
    DevBuf psi, phi, lf;
    RotParams P;

    // share: another launch of the same lmax whose log2 k! table is used instead of building a second one
    int build(int lmax, long double ps, long double th, long double ph, const RotTables *share = nullptr)
    {
        if (th < 0) {
            th = -th;
            ps -= PI_L;
            ph += PI_L;
        }
        const size_t nl = (size_t)lmax + 1;
        if (!share) {
            std::vector<double2> t(2 * nl);
            long double sum = 0, comp = 0;  // log2 k!, compensated
            t[0] = make_double2(0.0, 0.0);
            for (size_t k = 1; k < t.size(); ++k) {
                const long double y = log2l((long double)k) - comp, s = sum + y;
                comp = (s - sum) - y;
                sum = s;
                t[k] = split_ld(sum - comp);
            }
            HX_TRY(upload_vec(lf, t));
        }
        HX_TRY(upload_vec(psi, phase_table(lmax, ps)));
        HX_TRY(upload_vec(phi, phase_table(lmax, ph)));
        P.lmax = lmax;
        // cos(theta) = xh + xl with xh a multiple of 2^-22: l(l+1) xh - m m' (below 2^31) is then exact in the kernel's inner fma and
        // the outer one rounds l(l+1) x - m m' once.  With xh the nearest double the inner fma rounded away what xl was to add wherever
        // the two terms do not cancel: cos(theta) was a double in effect, theta off by up to 1.1e-16 / tan(theta), times lmax in d^l
        const long double cx = cosl(th);
        const double2 lc = split_ld(log2l(cosl(th / 2))), ls = split_ld(log2l(sinl(th / 2)));
        P.xh = (double)ldexpl(rintl(ldexpl(cx, 22)), -22);
        P.xl = (double)(cx - (long double)P.xh);
        P.lc = DD{lc.x, lc.y};
        P.ls = DD{ls.x, ls.y};
        P.lf = (share ? share->lf : lf).as<double2>();
        P.ppsi = psi.as<double2>();
        P.pphi = phi.as<double2>();
        return HX_OK;
    }

    void launch(int ncomp, const double2 *in, double2 *out, hipStream_t st) const
    {
        const dim3 grid((unsigned)((P.lmax + 1 + ROT_MO - 1) / ROT_MO), (unsigned)((ncomp + ROT_CB - 1) / ROT_CB));
        hipLaunchKernelGGL(k_rotate_alm, grid, dim3(ROT_MO * ROT_MB), 0, st, P, ncomp, in, out);
    }
};

}  // namespace

int rotate_exec_flops(unsigned long long *v, bool reset)
{
    HX_HIP(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_rot_flops), sizeof(*v)));
    const unsigned long long z = 0;
    if (reset) HX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_rot_flops), &z, sizeof(z)));
    return HX_OK;
}

}  // namespace hx

using namespace hx;

extern "C" int hx_rotate_alm(int lmax, int ncomp, const double _Complex *alm_in, double _Complex *alm_out, double psi, double theta, double phi)
{
    HX_TRY(ensure_ready());
    if (lmax < 0) return fail(HX_ERR_ARG, "hx_rotate_alm: lmax = %d", lmax);
    if (lmax > ROT_LMAX) return fail(HX_ERR_UNSUPPORTED, "hx_rotate_alm: lmax = %d, at most %d (32-bit products of l +- m)", lmax, ROT_LMAX);
    if (ncomp < 1) return fail(HX_ERR_ARG, "hx_rotate_alm: ncomp = %d", ncomp);
    if ((ncomp + ROT_CB - 1) / ROT_CB > 65535) return fail(HX_ERR_ARG, "hx_rotate_alm: ncomp = %d, at most %d components in one call", ncomp, 65535 * ROT_CB);
    if (!alm_in || !alm_out) return fail(HX_ERR_ARG, "hx_rotate_alm: null pointer");
    if (!std::isfinite(psi) || !std::isfinite(theta) || !std::isfinite(phi))
        return fail(HX_ERR_ARG, "hx_rotate_alm: the angles (%g, %g, %g) are not finite", psi, theta, phi);
    const size_t nl = (size_t)lmax + 1, nlm = nl * (nl + 1) / 2, bytes = sizeof(double2) * nlm * (size_t)ncomp;
    {
        const uintptr_t a = (uintptr_t)alm_in, b = (uintptr_t)alm_out;
        if (a < b + bytes && b < a + bytes)
            return fail(HX_ERR_ARG, "hx_rotate_alm: alm_in and alm_out overlap (every output order needs every input order: there is no in-place rotation)");
    }
    // theta into [0, pi] through its half angle: cosl and sinl reduce any argument exactly (theta mod a 64-bit 2 pi is off by 3e-19 per
    // turn, times lmax in the phase of d), theta and theta + 2 pi give the same d^l, and cos(theta/2) sin(theta/2) < 0 is a theta in
    // (pi, 2 pi): Ry(-theta) = Rz(pi) Ry(theta) Rz(-pi)
    long double ps = psi, ph = phi;
    const long double hc = cosl((long double)theta / 2), hs = sinl((long double)theta / 2);
    if ((hc < 0) != (hs < 0) && hc != 0 && hs != 0) {
        ps -= PI_L;
        ph += PI_L;
    }
    const long double th = 2 * atan2l(fabsl(hs), fabsl(hc));
    ps = fmodl(ps, 2 * PI_L);
    ph = fmodl(ph, 2 * PI_L);
    const bool at_zero = th == 0, at_pi = (double)th == (double)PI_L;

    InView vin;
    HX_TRY(vin.bind(alm_in, bytes));
    OutView vout;
    HX_TRY(vout.bind(alm_out, bytes));
    hipStream_t st = rt().stream;
    DevBuf b_phi, b_mid;
    RotTables t1, t2;
    if (at_zero || at_pi) {
        // a'_lm = exp(-i m (phi + psi)) a_lm;  at pi: (-1)^l exp(-i m (phi - psi)) conj(a_lm)
        HX_TRY(upload_vec(b_phi, phase_table(lmax, at_zero ? ph + ps : ph - ps)));
        ProfScope prof("rotate_alm");
        hipLaunchKernelGGL(k_rotate_phase, dim3((unsigned)((nl + 255) / 256), (unsigned)nl, (unsigned)ncomp), dim3(256), 0, st, lmax, at_pi ? 1 : 0,
                           b_phi.as<double2>(), vin.as<double2>(), vout.as<double2>());
    } else if (sinl(th) < ROT_SPLIT_SIN) {
        // d^l(theta) = d^l(pi/2) d^l(theta - pi/2): two rotations by angles of order one through a scratch alm, since the FP64 chains
        // lose 1 / sin(theta).  theta - pi/2 stays a long double: rounded to a double it is lmax 1e-16 of phase
        HX_TRY(b_mid.alloc(bytes));
        HX_TRY(t1.build(lmax, ps, PI_L / 2, 0));
        HX_TRY(t2.build(lmax, 0, th - PI_L / 2, ph, &t1));
        ProfScope prof("rotate_alm");
        t1.launch(ncomp, vin.as<double2>(), b_mid.as<double2>(), st);
        t2.launch(ncomp, b_mid.as<double2>(), vout.as<double2>(), st);
    } else {
        HX_TRY(t1.build(lmax, ps, th, ph));
        ProfScope prof("rotate_alm");
        t1.launch(ncomp, vin.as<double2>(), vout.as<double2>(), st);
    }
    HX_HIP(hipGetLastError());
    HX_TRY(vout.finish());
    return finish_call();
}
