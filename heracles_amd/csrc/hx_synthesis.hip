// hx_synthesis.hip -- alm2map: ring modes of the Legendre synthesis (hx_legendre_valu.hip, hx_synth_duo.hip) -> ring spectra ->
// pixels.  The inverse sub-DFTs that write the pixels are those of the ring Fourier stage (hx_ring_fft.hip).
#include <algorithm>

#include "hx_sht_common.h"

namespace hx {
// =====================================================================================
// synthesis: Fv -> ring spectra -> pixels (the Legendre part lives in hx_legendre_valu.hip)
// =====================================================================================
// Fv[m][rp][4 nc] -> conj(Z) spectra of the packed ring pair z = f_N + i f_S.  Fv is the output of the vector-unit synthesis
// (hx_legendre_valu.hip) for ONE map (nc = 1) or (Q, U) field (nc = 2), component c = (N_re, N_im, S_re, S_im) at 4 c.
// X[k] = sum_{m == k mod nphi} (c_m/2) Ft_m + sum_{m == -k} (c_m/2) conj(Ft_m), Ft = F e^{i m phi0};  output
// Zc[c][startN + k] = conj(X_N + i X_S).  The values of four consecutive ring pairs at one m share a 128-byte line: a group
// takes four ring pairs (thread = (ring pair, component, k)).
__global__ __launch_bounds__(256) void k_synth_spectrum_v(PlanDev P, const double *__restrict__ Fv, int nc, int lmax,
                                                          double2 *__restrict__ Zc, const int *__restrict__ mlim, int rp_hi)
{
    const int rp = blockIdx.x * 4 + (threadIdx.x & 3), rest = threadIdx.x >> 2;
    if (rp >= P.nrp || rp >= rp_hi) return;  // (ring pairs from rp_hi on: k_synth_spectrum_t)
    // nc <= 64 components side by side (nc need not divide 64: the threads left over have nothing to do)
    const int c = rest % nc, kk = rest / nc, kstep = (int)(blockDim.x >> 2) / nc;
    if (kk >= kstep) return;
    const int n = P.nsub[rp], nphi = 4 * n;
    const bool shifted = P.shifted[rp] != 0;
    const long long mstride = (long long)P.nrp_pad * 4 * nc;
    const double *row = Fv + (long long)rp * 4 * nc + 4 * c;
    // mlim (batched matrix-unit synthesis): rows of this ring pair exist for m <= mlim[rp] only (pruned beyond: zero, and not written)
    const int mtop = mlim ? min(lmax, mlim[rp]) : lmax;
    // One pass serves the bins k and nphi - k: A = sum_{m == k} (c_m / 2) Ft_m, B = sum_{m == -k} (c_m / 2) Ft_m;
    // X[k] = A + conj(B), X[nphi - k] = B + conj(A) -- every value of Fv is read once (round 5; two passes before)
    for (int k = kk; 2 * k <= nphi; k += kstep) {
        const int k2 = (nphi - k) % nphi;
        double2 an = make_double2(0.0, 0.0), as = an, bn = an, bs = an;
        for (int m = k; m <= mtop; m += nphi) {  // m == k (mod nphi)
            const double2 *b = reinterpret_cast<const double2 *>(row + m * mstride);
            double2 ph = make_double2(1.0, 0.0);
            if (shifted) ph = expipi((double)(m % (2 * nphi)) / (double)nphi);
            const double sc = m == 0 ? 0.5 : 1.0;  // c_m / 2
            an = cadd(an, cscale(cmul(b[0], ph), sc));
            as = cadd(as, cscale(cmul(b[1], ph), sc));
        }
        if (k2 != k) {
            for (int m = k2; m <= mtop; m += nphi) {  // m == -k (mod nphi)
                const double2 *b = reinterpret_cast<const double2 *>(row + m * mstride);
                double2 ph = make_double2(1.0, 0.0);
                if (shifted) ph = expipi((double)(m % (2 * nphi)) / (double)nphi);
                const double sc = m == 0 ? 0.5 : 1.0;
                bn = cadd(bn, cscale(cmul(b[0], ph), sc));
                bs = cadd(bs, cscale(cmul(b[1], ph), sc));
            }
        } else {
            bn = an;
            bs = as;
        }
        double2 *z = Zc + (long long)c * P.ny + P.startN[rp];
        z[k] = cconj(cadd(cadd(an, cconj(bn)), mul_pi(cadd(as, cconj(bs)))));
        if (k2 != k) z[k2] = cconj(cadd(cadd(bn, cconj(an)), mul_pi(cadd(bs, cconj(as)))));
    }
}

// The same for ring pairs with 4 n >= 2 lmax + 2 pixels per ring (round 5; at nside 4096 / lmax 6144: 5120 of the 8192 ring pairs, 73 % of
// the pixels): no two orders fall on one bin, so the pass is a TRANSPOSITION -- bin m = conj(Ft_N + i Ft_S), bin nphi - m =
// conj(conj Ft_N + i conj Ft_S), zeros between lmax and nphi - lmax -- and goes through LDS: a block takes one ring pair and 64
// orders, reads their rows of Fv (nc x 32 contiguous bytes each), and writes, per component, two runs of 64 consecutive bins.  The
// gather above walks the orders per bin with one or two 32-byte reads in flight per thread and scatters 16-byte writes: 48 ms for the
// twenty components of ten fields against ~16 ms of traffic at copy rate.
constexpr int SPT_M = 64;
__global__ __launch_bounds__(256) void k_synth_spectrum_t(PlanDev P, const double *__restrict__ Fv, int nc, int lmax, double2 *__restrict__ Zc,
                                                          const int *__restrict__ mlim, int rp_lo)
{
    extern __shared__ double2 spt[];  // [2][nc][SPT_M]: the bins m and nphi - m of the block's orders
    const int rp = rp_lo + blockIdx.x;
    const int n = P.nsub[rp], nphi = 4 * n, m0 = blockIdx.y * SPT_M;
    if (2 * m0 > nphi) return;  // (orders beyond nphi / 2 belong to the mirrored run of another block)
    const bool shifted = P.shifted[rp] != 0;
    const int mtop = mlim ? min(lmax, mlim[rp]) : lmax;
    const long long mstride = (long long)P.nrp_pad * 4 * nc;
    const double *row = Fv + (long long)rp * 4 * nc;
    // element e = (order j of the tile, component c): 32 contiguous bytes; consecutive threads take consecutive components of an order
    for (int e = threadIdx.x; e < SPT_M * nc; e += blockDim.x) {
        const int j = e / nc, c = e % nc, m = m0 + j;
        double2 z1 = make_double2(0.0, 0.0), z2 = z1;
        if (m <= mtop) {
            const double2 *b = reinterpret_cast<const double2 *>(row + m * mstride + 4 * c);
            double2 fn = b[0], fs = b[1];
            if (shifted) {
                const double2 ph = expipi((double)(m % (2 * nphi)) / (double)nphi);
                fn = cmul(fn, ph);
                fs = cmul(fs, ph);
            }
            if (m == 0) {  // c_0 / 2 = 1 / 2 and both sums meet in bin 0
                z1 = cconj(cadd(make_double2(fn.x, 0.0), mul_pi(make_double2(fs.x, 0.0))));
            } else {
                z1 = cconj(cadd(fn, mul_pi(fs)));
                z2 = cconj(cadd(cconj(fn), mul_pi(cconj(fs))));
            }
        }
        spt[c * SPT_M + j] = z1;
        spt[(nc + c) * SPT_M + j] = z2;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SPT_M * nc; e += blockDim.x) {
        const int c = e / SPT_M, j = e % SPT_M, m = m0 + j;
        double2 *z = Zc + (long long)c * P.ny + P.startN[rp];
        if (2 * m <= nphi) z[m] = spt[c * SPT_M + j];
        if (m > 0 && 2 * m < nphi) z[nphi - m] = spt[(nc + c) * SPT_M + j];
    }
}

// (Until round 6 the inverse sub-DFTs wrote their spectra to Y and a pass of its own, k_synth_scatter, turned Y_r[k] = conj(z[4k + r]) into
// pixels: 20 ms per ten fields.  The read-out of the sub-DFT kernels writes the pixels itself now -- MODE 1 with `pixout`: ten fields
// 62.7 -> 52.7 ms of ring stage, ten maps 31.0 -> 25.9, same device -- and a synthesis holds no Y buffer.)
}  // namespace hx

using namespace hx;

// ---- one synthesis pass over a batch (device pointers): one sweep of the vector-unit kernel per map / field (the round-1 matrix
// kernel it replaces took 100 / 217 ms for one spin-0 map / spin-2 field at nside 4096 against 19 / 57, and 201 / 653 ms for ten
// against 187 / 570).  If d_ref != NULL the output is the residual ref - synth (Jacobi iteration). ----
// small batches: one sweep of the vector-unit kernel per four maps / two fields (they share the recursion), then the rest
// generic: one field per sweep of the run-time-spin instantiation, with the tables and the task set of its weight
static int synthesis_batch_valu(hx_plan *pl, int spin, int nb, const double2 *d_alms, double *d_maps, const double *d_ref, bool generic = false)
{
    hipStream_t st = rt().stream;
    const int cpu = spin ? 2 : 1;
    PlanDev P = pl->dev();
    const int umax = generic ? 1 : synth_valu_max_units(spin);
    // ring modes and ring spectra live in the analysis' operand buffer F, as in the batched path (F is idle during a synthesis, and a plan
    // that has run a batched synthesis holds most of the HBM in it already: separate buffers failed to allocate at nside 8192)
    const size_t fv_pad = (sizeof(double) * (size_t)(pl->lmax + 1) * pl->nrp_pad * 4 * cpu * umax + 255) & ~(size_t)255;
    HX_TRY(pl->F.alloc(fv_pad + sizeof(double2) * (size_t)pl->ny * cpu * umax));
    double *fsyn = pl->F.as<double>();
    double2 *zc = reinterpret_cast<double2 *>(reinterpret_cast<char *>(pl->F.p) + fv_pad);
    for (int c0 = 0; c0 < nb;) {
        int units = umax;
        while (units * cpu > nb - c0) units >>= 1;
        const int nc = units * cpu;
        hx_plan::SpinData *sd = nullptr;
        hx_plan::TaskSet *ts = nullptr;
        HX_TRY(spin_data(pl, spin, generic, &sd));
        HX_TRY(task_set(pl, spin, generic, synth_valu_task_blocks(spin, units), &ts));
        HX_TRY(launch_synth_valu(pl, spin, units, *sd, *ts, d_alms + (size_t)c0 * pl->nlm, fsyn, generic));
        ProfScope ps("ring_fft");
        hipLaunchKernelGGL(k_synth_spectrum_v, dim3((pl->nrp + 3) / 4), dim3(256), 0, st, P, fsyn, nc, pl->lmax, zc, (const int *)nullptr, pl->nrp);
        // inverse sub-DFTs whose read-out writes the pixels (or the residual ref - synthesised of a Jacobi iteration) itself
        HX_TRY(launch_ring_subdft_spectra(pl, nc, zc, d_maps + (size_t)c0 * pl->npix, d_ref ? d_ref + (size_t)c0 * pl->npix : nullptr));
        c0 += nc;
    }
    HX_HIP(hipGetLastError());
    return HX_OK;
}

int hx::synthesis_batch(hx_plan *pl, int spin, int nb, const double2 *d_alms, double *d_maps, const double *d_ref)
{
    hipStream_t st = rt().stream;
    const int cpu = spin ? 2 : 1;  // components per unit (map / field)
    const bool generic = plan_generic_spin(pl, spin);
    if (generic || (spin != 0 && spin != 2)) {
        // a spin weight other than 0 and 2 (HX_SPIN_GENERIC=1: 2 as well): one sweep of the run-time-spin kernel per field
        if (!generic || pl->hsrc) return fail(HX_ERR_UNSUPPORTED, "spin-%d maps not yet supported", spin);
        if (spin < 0 || nb < 2 || (nb & 1)) return fail(HX_ERR_ARG, "synthesis_batch: %d components of spin %d", nb, spin);
        if (spin > pl->lmax) {  // no l >= s below the band limit: zero maps, i.e. the residual is the reference
            const size_t bytes = sizeof(double) * (size_t)pl->npix * nb;
            if (d_ref) HX_HIP(hipMemcpyAsync(d_maps, d_ref, bytes, hipMemcpyDeviceToDevice, st));
            else HX_HIP(hipMemsetAsync(d_maps, 0, bytes, st));
            return HX_OK;
        }
        return synthesis_batch_valu(pl, spin, nb, d_alms, d_maps, d_ref, true);
    }
    PlanDev P = pl->dev();
    // batches of >= 5 maps / >= 3 fields: sweeps of up to 20 maps / 10 fields on the matrix unit (hx_synth_duo.hip).  Their ring
    // modes (Fv) and ring spectra (conj Z) live in the analysis' operand buffer F, which is idle during a synthesis: a Jacobi iteration
    // of ten fields needs no HBM beyond what its analysis passes hold (F 64 GB >= 32 + 32).
    const int nunits_all = nb / cpu;
    const int umin = synth_duo_min_units(spin);
    if (nunits_all >= umin) {
        const int umax = synth_duo_max_units(spin);
        hx_plan::SpinData *sd = nullptr;
        hx_plan::TaskSet *ts = nullptr;
        const int *ml = nullptr;  // rows of Fv beyond ml[rp] are neither written nor read
        HX_TRY(spin_data(pl, spin, false, &sd));
        HX_TRY(task_set(pl, spin, false, one_set_task_blocks(spin), &ts));
        HX_TRY(synth_mlim(pl, spin, &ml));
        // what a sweep of `units` holds: ring modes + ring spectra (in F), the B-operand table
        auto sweep_bytes = [&](int units) {
            const double nc = (double)units * cpu;
            return sizeof(double) * (double)(pl->lmax + 1) * pl->nrp_pad * synth_duo_rowlen(spin, units) + sizeof(double2) * (double)pl->ny * nc +
                   (double)synth_duo_table_bytes(pl, spin, units);
        };
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = 0; }
        double avail = 0.92 * ((double)fr + (double)pl->F.bytes + (double)pl->Y.bytes + (double)pl->syn_tab.bytes);
        if (scratch_budget_bytes() > 0.0) avail = std::min(avail, scratch_budget_bytes());  // (hx_set_scratch_budget bounds this scratch too)
        for (int u0 = 0; u0 < nunits_all;) {
            int units = std::min(umax, nunits_all - u0);
            // (a remainder of one or two units would run a whole sweep of the matrix kernel for 4-8 columns: split the tail evenly instead)
            if (nunits_all - u0 > umax && nunits_all - u0 < umax + umin) units = (nunits_all - u0 + 1) / 2;
            // a sweep that does not fit the free HBM (nside 8192: 213 + 129 GB for ten fields) is cut down; below the matrix kernel's
            // smallest useful batch the rest goes to the vector-unit kernel's sweeps of four maps / two fields
            while (units > 1 && sweep_bytes(units) > avail) --units;
            if (units < umin && sweep_bytes(units) > avail) units = 0;
            if (units < umin && (units == 0 || nunits_all - u0 >= umin)) {
                HX_TRY(synthesis_batch_valu(pl, spin, (nunits_all - u0) * cpu, d_alms + (size_t)u0 * cpu * pl->nlm, d_maps + (size_t)u0 * cpu * pl->npix,
                                            d_ref ? d_ref + (size_t)u0 * cpu * pl->npix : nullptr));
                break;
            }
            const int nc = units * cpu, rowlen = synth_duo_rowlen(spin, units);
            const size_t fv_bytes = sizeof(double) * (size_t)(pl->lmax + 1) * pl->nrp_pad * rowlen;
            const size_t zc_bytes = sizeof(double2) * (size_t)pl->ny * nc;
            const size_t fv_pad = (fv_bytes + 255) & ~(size_t)255;
            HX_TRY(pl->F.alloc(fv_pad + zc_bytes));
            HX_TRY(pl->syn_tab.alloc(synth_duo_table_bytes(pl, spin, units)));
            double *fv = pl->F.as<double>();
            double2 *zc = reinterpret_cast<double2 *>(reinterpret_cast<char *>(pl->F.p) + fv_pad);
            HX_TRY(launch_synth_duo(pl, spin, units, *sd, *ts, d_alms + (size_t)u0 * cpu * pl->nlm, pl->syn_tab.as<double>(), fv));
            ProfScope ps("ring_fft");
            {
                // ring pairs whose rings hold every order in a bin of its own go through the transposing pass, the polar ones through the gather
                int rp_t = pl->nrp;
                while (rp_t > 0 && 4 * pl->h_nsub[rp_t - 1] >= 2 * pl->lmax + 2) --rp_t;
                if (rp_t > 0)
                    hipLaunchKernelGGL(k_synth_spectrum_v, dim3((rp_t + 3) / 4), dim3(256), 0, st, P, fv, nc, pl->lmax, zc, ml, rp_t);
                if (rp_t < pl->nrp) {
                    const int nphi_max = 4 * pl->h_nsub[pl->nrp - 1];
                    const dim3 grid(pl->nrp - rp_t, (nphi_max / 2 + SPT_M) / SPT_M);
                    hipLaunchKernelGGL(k_synth_spectrum_t, grid, dim3(256), sizeof(double2) * 2 * nc * SPT_M, st, P, fv, nc, pl->lmax, zc, ml, rp_t);
                }
            }
            HX_TRY(launch_ring_subdft_spectra(pl, nc, zc, d_maps + (size_t)u0 * cpu * pl->npix, d_ref ? d_ref + (size_t)u0 * cpu * pl->npix : nullptr));
            u0 += units;
        }
        HX_HIP(hipGetLastError());
        return HX_OK;
    }
    return synthesis_batch_valu(pl, spin, nb, d_alms, d_maps, d_ref);
}

extern "C" int hx_alm2map(hx_plan *pl, int spin, int ncomp, const double *alms, double *maps)
{
    HX_TRY(ensure_ready());
    HX_TRY(check_sht_args(pl, spin, ncomp, alms, maps, true));
    InView valms;
    OutView vmaps;
    HX_TRY(valms.bind(alms, sizeof(double2) * (size_t)ncomp * pl->nlm));
    HX_TRY(vmaps.bind(maps, sizeof(double) * (size_t)ncomp * pl->npix));
    HX_TRY(synthesis_batch(pl, spin, ncomp, valms.as<double2>(), vmaps.as<double>(), nullptr));
    HX_TRY(vmaps.finish());
    if (valms.tmp.p || vmaps.tmp.p) {
        HX_HIP(hipStreamSynchronize(rt().stream));
        return HX_OK;
    }
    return finish_call();
}
