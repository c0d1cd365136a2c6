// hx_map2alm.hip -- map2alm entry points of the C ABI: hx_map2alm (one batch, Jacobi iterations), and hx_map2alm_multi /
// hx_map2alm_list, whose host maps go through one upload pipeline that the transforms follow (map2alm_multi_impl; how a call is
// cut into sweeps: hx_sweep_plan.h).  Pipeline of one sweep: hx_sht_common.h.
#include <algorithm>
#include <chrono>
#include <cstdlib>

#include "hx_sht_common.h"
#include "hx_sweep_plan.h"

using namespace hx;

int hx::check_sht_args(hx_plan *pl, int spin, int ncomp, const void *a, const void *b, bool any_spin)
{
    if (!pl || !a || !b) return fail(HX_ERR_ARG, "null plan or buffer");
    if (pl->nside < 1) return fail(HX_ERR_ARG, "not a HEALPix plan");
    if (spin < 0 && any_spin) return fail(HX_ERR_ARG, "negative spin weight %d", spin);
    if (spin != 0 && spin != 2 && !any_spin) return fail(HX_ERR_UNSUPPORTED, "spin-%d maps not yet supported", spin);
    if (ncomp < 1 || (spin >= 1 && (ncomp & 1))) return fail(HX_ERR_ARG, "bad component count %d for spin %d", ncomp, spin);
    return HX_OK;
}

namespace hx {
__global__ void k_apply_fl(int lmax, int ncomp, long long nlm, const double *__restrict__ fl, double2 *__restrict__ alm)
{
    const int m = blockIdx.x;
    for (int i = threadIdx.x; i < (lmax - m + 1) * ncomp; i += blockDim.x) {
        const int c = i / (lmax - m + 1), l = m + i % (lmax - m + 1);
        double2 *p = alm + c * nlm + almidx(lmax, l, m);
        p->x *= fl[l];
        p->y *= fl[l];
    }
}
}  // namespace hx

static int apply_fl(hx_plan *pl, int nb, double2 *alm, const double *fl)
{
    hipLaunchKernelGGL(k_apply_fl, dim3(pl->lmax + 1), dim3(256), 0, rt().stream, pl->lmax, nb, pl->nlm, fl, alm);
    HX_HIP(hipGetLastError());
    return HX_OK;
}

// one array, on the host (through the pinned pipeline) or on the device, into device memory, ordered on `on` (nullptr: the library stream)
static int push(void *dst, const double *src, size_t bytes, hipStream_t on)
{
    if (is_device_ptr(src)) HX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, on ? on : rt().stream));
    else HX_TRY(copy_h2d(dst, src, bytes, on));
    return HX_OK;
}

// The components src(0) .. src(ncomp - 1) of npix values each gathered into dst: runs of components that lie behind one another
// in memory go as one transfer.
template <class Src>
static int gather_components(double *dst, int ncomp, long long npix, Src src, hipStream_t on)
{
    for (int c = 0, e; c < ncomp; c = e) {
        for (e = c + 1; e < ncomp && src(e) == src(e - 1) + npix; ++e) {}  // [c, e): one run
        HX_TRY(push(dst + (size_t)c * npix, src(c), sizeof(double) * (size_t)(e - c) * npix, on));
    }
    return HX_OK;
}

// Several transforms as ONE call (the loop of heracles/mapping.py:151-172 over the (field, bin) maps of a job): host maps of ALL
// jobs go through one upload pipeline (pageable -> pinned -> HBM, second stream) that the transforms follow, across job boundaries, so
// that the call costs its PCIe time plus very little.  A host job is cut into the sweeps that cost least per map (ten fields / ten maps
// at the bench size) and every such sweep runs as a StreamSweep (hx_sht_common.h): its rings are uploaded slab by slab -- for every
// component the block of northern rings of the slab and the block of their southern partners -- and the slab's ring FFTs, operand rows
// and completed ring groups are queued behind it; what is left behind the last byte is a twelfth of a sweep (21 ms at the bench size:
// 48 GB in 882 ms).  Sweeps that cannot be streamed (the small batches of the vector-unit kernels, HX_STREAM_SLABS=0) are uploaded whole,
// at most 5 spin-2 fields / 8 spin-0 maps at a time with the last one halved until it holds at most two units (round 3's pipeline: 960 ms).
// Callers put their large jobs first.  niter = 0 only (iterations need their maps resident).
// comp_maps (hx_map2alm_list): job j's components are SEPARATE arrays comp_maps[j][c] (maps[j] = the first of them); they are
// gathered into the staging buffer of their sweep -- host arrays through the pinned pipeline, device arrays by copies on the
// upload stream; neighbours in memory go as one transfer.
static int map2alm_multi_impl(hx_plan *pl, int njobs, const int *spins, const int *ncomps, const double *const *maps, const double *const *const *comp_maps,
                              double *const *alms, const double *ring_weights, const double *pix_weights, const double *const *fls)
{
    HX_TRY(ensure_ready());
    if (!pl || njobs < 1 || !spins || !ncomps || !maps || !alms) return fail(HX_ERR_ARG, "hx_map2alm_multi: bad arguments");
    for (int j = 0; j < njobs; ++j) HX_TRY(check_sht_args(pl, spins[j], ncomps[j], maps[j], alms[j]));
    // a job goes through the staging buffers if its maps are on the host, or scattered over separate arrays
    std::vector<bool> staged(njobs);
    InView vrw, vpw;
    HX_TRY(vrw.bind(ring_weights, sizeof(double) * pl->nrp));
    HX_TRY(vpw.bind(pix_weights, sizeof(double) * (size_t)pl->npix));
    HX_TRY(classify_pixel_weights(pl, vpw.as<double>()));
    std::vector<InView> vfl(njobs);
    std::vector<OutView> valm(njobs);
    // HX_STREAM_SLABS: slabs of rings per streamed sweep (default 12; 0 or 1: the sweeps of round 3 -- whole maps, 5 fields / 8 maps at most)
    static int want_slabs = -1;
    if (want_slabs < 0) { const char *e = getenv("HX_STREAM_SLABS"); want_slabs = e ? atoi(e) : 12; }
    bool any_host = false;
    for (int j = 0; j < njobs; ++j) {
        HX_TRY(vfl[j].bind(fls ? fls[j] : nullptr, sizeof(double) * (pl->lmax + 1)));
        HX_TRY(valm[j].bind(alms[j], sizeof(double2) * (size_t)ncomps[j] * pl->nlm));
        staged[j] = !is_device_ptr(maps[j]) || (comp_maps && comp_maps[j]);
        any_host = any_host || staged[j];
    }
    // host maps: the sweep that costs least per map, its rings uploaded and transformed slab by slab (StreamSweep), or, where that
    // is not possible, whole maps in small sweeps (plan_sweeps)
    auto can_stream = [&](int spin, int nb) { return want_slabs > 1 && copy_stream() != nullptr && analysis_can_stream(pl, spin, nb); };
    std::vector<Sweep> sweeps = plan_sweeps(njobs, spins, ncomps, staged, analysis_next_batch, can_stream);
    hipStream_t cs = any_host ? copy_stream() : nullptr;
    size_t stage_bytes = 0;
    for (const Sweep &w : sweeps)
        if (staged[w.job]) stage_bytes = std::max(stage_bytes, (size_t)(sizeof(double) * (size_t)w.nb * (size_t)pl->npix));
    // host sweeps are numbered in upload order; buffer h % NST holds host sweep h.  THREE buffers: the upload of sweep h + 1 waits
    // for the transform of sweep h - 2, not h - 1 -- with two, a 4.8 GB upload sat 130 ms behind the 240 ms transform of the
    // spin-2 sweep before it (tools/time_host_multi.py).  Streamed sweeps are up to 32 GB each and end right behind their upload: two.
    const int NST = 3 * (double)stage_bytes > 64e9 ? 2 : hx_plan::NSTAGE;
    constexpr int NEV = hx_plan::NUNIT_EV;
    hipEvent_t *unit_up = pl->unit_up;
    if (any_host) {
        if (!cs) return fail(HX_ERR_HIP, "hx_map2alm_multi: no copy stream");
        for (int i = 0; i < NST; ++i) {
            HX_TRY(pl->stage[i].alloc(stage_bytes));
            if (!pl->stage_done[i]) HX_HIP(hipEventCreateWithFlags(&pl->stage_done[i], hipEventDisableTiming));
        }
        for (int i = 0; i < NEV; ++i)
            if (!unit_up[i]) HX_HIP(hipEventCreateWithFlags(&unit_up[i], hipEventDisableTiming));
    }
    std::vector<int> hidx(sweeps.size(), -1);
    int nh = 0;
    for (size_t k = 0; k < sweeps.size(); ++k)
        if (staged[sweeps[k].job]) hidx[k] = nh++;
    // streamed sweeps: slab edges, task tables and scratch of ALL of them before anything is queued
    std::vector<StreamSweep> ss(sweeps.size());
    for (size_t k = 0; k < sweeps.size(); ++k) {
        const Sweep &w = sweeps[k];
        if (!w.stream) continue;
        HX_TRY(analysis_stream_plan(pl, spins[w.job], w.nb, want_slabs, ss[k]));
        ss[k].d_maps = pl->stage[hidx[k] % NST].as<double>();
        ss[k].d_alms = valm[w.job].as<double2>() + (size_t)w.c0 * pl->nlm;
        ss[k].d_rw = vrw.as<double>(); ss[k].d_pw = vpw.as<double>(); ss[k].d_fl = vfl[w.job].as<double>();
    }
    for (size_t k = 0; k < sweeps.size(); ++k)
        if (sweeps[k].stream) HX_TRY(analysis_stream_leadin(ss[k]));
    // units of work in order: a whole sweep, or one slab of a streamed sweep; units of host sweeps have an upload in front of them
    struct Unit { size_t k; int slab; };
    std::vector<Unit> units;
    for (size_t k = 0; k < sweeps.size(); ++k) {
        if (sweeps[k].stream)
            for (int q = 0; q < ss[k].nslab; ++q) units.push_back({k, q});
        else
            units.push_back({k, -1});
    }
    std::vector<int> uidx(units.size(), -1);  // number of the unit among those with an upload
    int nu = 0;
    for (size_t u = 0; u < units.size(); ++u)
        if (hidx[units[u].k] >= 0) uidx[u] = nu++;
    // component c of a sweep: its source array and its place in the staging buffer
    auto comp_src = [&](const Sweep &w, int c) -> const double * {
        return (comp_maps && comp_maps[w.job]) ? comp_maps[w.job][w.c0 + c] : maps[w.job] + (size_t)(w.c0 + c) * pl->npix;
    };
    auto upload = [&](size_t u) -> int {
        const Sweep &w = sweeps[units[u].k];
        const int b = hidx[units[u].k] % NST, slab = units[u].slab;
        if (slab <= 0 && hidx[units[u].k] >= NST) HX_HIP(hipEventSynchronize(pl->stage_done[b]));  // host sweep h - NST has read this buffer
        double *stage = pl->stage[b].as<double>();
        if (slab < 0) {
            HX_TRY(gather_components(stage, w.nb, pl->npix, [&](int c) { return comp_src(w, c); }, cs));
        } else {
            // the rings of the slab: a block of northern rings and the block of their southern partners, per component
            const StreamSweep &sw = ss[units[u].k];
            const int r0 = sw.rp_edge[slab], r1 = std::min(sw.rp_edge[slab + 1], pl->nrp) - 1;  // first and last ring pair
            const long long n0 = pl->h_startN[r0], n1 = pl->h_startN[r1] + 4LL * pl->h_nsub[r1];
            const int rs = pl->h_startS[r1] >= 0 ? r1 : r1 - 1;                                  // (the equator has no southern ring)
            const long long s0 = rs >= r0 ? pl->h_startS[rs] : 0, s1 = rs >= r0 ? pl->h_startS[r0] + 4LL * pl->h_nsub[r0] : 0;
            for (int c = 0; c < w.nb; ++c) {
                const double *src = comp_src(w, c);
                double *dst = stage + (size_t)c * pl->npix;
                HX_TRY(push(dst + n0, src + n0, sizeof(double) * (size_t)(n1 - n0), cs));
                if (s1 > s0) HX_TRY(push(dst + s0, src + s0, sizeof(double) * (size_t)(s1 - s0), cs));
            }
        }
        HX_HIP(hipEventRecord(unit_up[uidx[u] % NEV], cs));
        return HX_OK;
    };
    auto next_upload = [&](size_t u) -> size_t {  // first unit after u with an upload
        for (size_t q = u + 1; q < units.size(); ++q)
            if (uidx[q] >= 0) return q;
        return units.size();
    };
    // HX_TRACE=1: host-side timeline of the call on stderr (ms since entry): when each unit's upload was staged and issued
    const bool trace = getenv("HX_TRACE") != nullptr;
    const auto t_entry = std::chrono::steady_clock::now();
    auto now_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count(); };
    auto traced_upload = [&](size_t u) -> int {
        const double t0 = now_ms();
        const int rc = upload(u);
        if (trace) {
            const Sweep &w = sweeps[units[u].k];
            fprintf(stderr, "[hx] multi: sweep %zu (job %d, spin %d, %d comps) slab %d staged %.0f -> %.0f ms\n", units[u].k, w.job, spins[w.job], w.nb, units[u].slab, t0, now_ms());
        }
        return rc;
    };
    const size_t first_up = next_upload((size_t)-1);
    if (first_up < units.size()) HX_TRY(traced_upload(first_up));
    for (size_t u = 0; u < units.size(); ++u) {
        const size_t k = units[u].k;
        const Sweep &w = sweeps[k];
        const int slab = units[u].slab;
        if (uidx[u] >= 0) HX_HIP(hipStreamWaitEvent(rt().stream, unit_up[uidx[u] % NEV], 0));
        bool done = true;
        if (slab < 0) {
            const double *src = hidx[k] >= 0 ? pl->stage[hidx[k] % NST].as<double>() : maps[w.job] + (size_t)w.c0 * pl->npix;
            HX_TRY(analysis_batch(pl, spins[w.job], w.nb, src, valm[w.job].as<double2>() + (size_t)w.c0 * pl->nlm, vrw.as<double>(), vpw.as<double>(),
                                  vfl[w.job].as<double>(), 0));
        } else {
            if (slab == 0) HX_TRY(analysis_stream_start(ss[k]));
            HX_TRY(analysis_stream_slab(ss[k], slab));
            done = slab + 1 == ss[k].nslab;
            if (done) HX_TRY(analysis_stream_end(ss[k]));
        }
        if (done && hidx[k] >= 0) HX_HIP(hipEventRecord(pl->stage_done[hidx[k] % NST], rt().stream));
        if (trace) fprintf(stderr, "[hx] multi: sweep %zu slab %d queued at %.0f ms\n", k, slab, now_ms());
        if (uidx[u] >= 0) {
            const size_t q = next_upload(u);
            if (q < units.size()) HX_TRY(traced_upload(q));  // the host thread stages the next unit while this one is transformed
        }
    }
    for (int j = 0; j < njobs; ++j) HX_TRY(valm[j].finish());
    if (trace) fprintf(stderr, "[hx] multi: everything queued at %.0f ms\n", now_ms());
    HX_HIP(hipStreamSynchronize(rt().stream));  // staging buffers of host arguments are released on return
    if (trace) fprintf(stderr, "[hx] multi: done at %.0f ms\n", now_ms());
    return HX_OK;
}

extern "C" int hx_map2alm(hx_plan *pl, int spin, int ncomp, const double *maps, double *alms,
                          const double *ring_weights, const double *pix_weights, const double *fl, int niter)
{
    HX_TRY(ensure_ready());
    HX_TRY(check_sht_args(pl, spin, ncomp, maps, alms, true));
    if (niter < 0) return fail(HX_ERR_ARG, "niter < 0");
    InView vmaps, vrw, vpw, vfl;
    OutView valms;
    // Host maps without iterations go through the upload pipeline of hx_map2alm_multi (one job): sweep k + 1 is staged (pageable ->
    // pinned -> HBM, second stream, three plan-owned buffers) while the GPU transforms sweep k
    // (a weight on the run-time-spin sweep is uploaded whole and transformed resident: the pipeline's sweeps are not built for it)
    if (niter == 0 && !is_device_ptr(maps) && copy_stream() != nullptr && !analysis_generic_spin(spin))
        return map2alm_multi_impl(pl, 1, &spin, &ncomp, &maps, nullptr, &alms, ring_weights, pix_weights, &fl);
    HX_TRY(vmaps.bind(maps, sizeof(double) * (size_t)ncomp * pl->npix));
    HX_TRY(vrw.bind(ring_weights, sizeof(double) * pl->nrp));
    HX_TRY(vpw.bind(pix_weights, sizeof(double) * (size_t)pl->npix));
    HX_TRY(classify_pixel_weights(pl, vpw.as<double>()));
    HX_TRY(vfl.bind(fl, sizeof(double) * (pl->lmax + 1)));
    HX_TRY(valms.bind(alms, sizeof(double2) * (size_t)ncomp * pl->nlm));
    // residual maps of the Jacobi iterations: plan-owned scratch (no per-call hipMalloc)
    DevBuf &resid = pl->resid_maps;
    // the sweeps are sized by analysis_next_batch(); the synthesis of the Jacobi iterations takes the maps / fields of a sweep in its
    // own sweeps of four maps / two fields
    if (niter > 0) HX_TRY(resid.alloc(sizeof(double) * (size_t)analysis_max_batch(spin, ncomp) * pl->npix));
    for (int c0 = 0, nb = 0; c0 < ncomp; c0 += nb) {
        nb = analysis_next_batch(spin, ncomp - c0);
        const double *dm = vmaps.as<double>() + (size_t)c0 * pl->npix;
        double2 *da = valms.as<double2>() + (size_t)c0 * pl->nlm;
        // the filter fl is applied once, after the last iteration
        HX_TRY(analysis_batch(pl, spin, nb, dm, da, vrw.as<double>(), vpw.as<double>(), niter == 0 ? vfl.as<double>() : nullptr, 0));
        for (int it = 0; it < niter; ++it) {
            HX_TRY(synthesis_batch(pl, spin, nb, da, resid.as<double>(), dm));
            HX_TRY(analysis_batch(pl, spin, nb, resid.as<double>(), da, vrw.as<double>(), vpw.as<double>(), nullptr, 1));
        }
        if (niter > 0 && fl) HX_TRY(apply_fl(pl, nb, da, vfl.as<double>()));
    }
    HX_TRY(valms.finish());
    // staging buffers of host arguments are released on return: only an all-device call may stay asynchronous
    if (vmaps.tmp.p || vrw.tmp.p || vpw.tmp.p || vfl.tmp.p || valms.tmp.p) {
        HX_HIP(hipStreamSynchronize(rt().stream));
        return HX_OK;
    }
    return finish_call();
}

extern "C" int hx_map2alm_multi(hx_plan *pl, int njobs, const int *spins, const int *ncomps, const double *const *maps, double *const *alms,
                                const double *ring_weights, const double *pix_weights, const double *const *fls)
{
    return map2alm_multi_impl(pl, njobs, spins, ncomps, maps, nullptr, alms, ring_weights, pix_weights, fls);
}

// The loop of heracles/mapping.py:151-172 as ONE call over the arrays the reference holds: one array per map -- [npix] for spin 0,
// [2][npix] (Q, U) for spin 2 -- and one output array per map ([nlm] / [2][nlm] complex).  The maps are gathered sweep by sweep
// into the staging buffers of hx_map2alm_multi (no stacked copy on the host: np.stack of the bench's 48 GB costs several seconds),
// spin-2 fields first; the alms are collected in HBM and handed out at the end.  niter > 0 (Jacobi iterations need their maps
// resident): the maps of a spin are gathered into one device array first, then transformed as a batch.
extern "C" int hx_map2alm_list(hx_plan *pl, int nmaps, const int *spins, const double *const *maps, double *const *alms,
                               const double *ring_weights, const double *pix_weights, const double *fl0, const double *fl2, int niter)
{
    HX_TRY(ensure_ready());
    if (!pl || nmaps < 1 || !spins || !maps || !alms || niter < 0) return fail(HX_ERR_ARG, "hx_map2alm_list: bad arguments");
    std::vector<const double *> comps[2];  // [0]: spin 2, [1]: spin 0 (large jobs first)
    std::vector<int> owner[2];
    for (int i = 0; i < nmaps; ++i) {
        if (spins[i] != 0 && spins[i] != 2) return fail(HX_ERR_UNSUPPORTED, "spin-%d maps not yet supported", spins[i]);
        if (!maps[i] || !alms[i]) return fail(HX_ERR_ARG, "hx_map2alm_list: null map or alm %d", i);
        const int g = spins[i] ? 0 : 1;
        comps[g].push_back(maps[i]);
        if (spins[i]) comps[g].push_back(maps[i] + pl->npix);
        owner[g].push_back(i);
    }
    int jspin[2], jn[2], nj = 0;
    const double *jmaps[2], *jfl[2];
    const double *const *jcomp[2];
    double *jalm[2];
    DevBuf out[2];
    for (int g = 0; g < 2; ++g) {
        if (comps[g].empty()) continue;
        HX_TRY(out[g].alloc(sizeof(double2) * comps[g].size() * (size_t)pl->nlm));
        jspin[nj] = g == 0 ? 2 : 0; jn[nj] = (int)comps[g].size(); jmaps[nj] = comps[g][0]; jcomp[nj] = comps[g].data();
        jalm[nj] = out[g].as<double>(); jfl[nj] = g == 0 ? fl2 : fl0;
        ++nj;
    }
    if (niter == 0) {
        HX_TRY(map2alm_multi_impl(pl, nj, jspin, jn, jmaps, jcomp, jalm, ring_weights, pix_weights, jfl));
    } else {
        InView vrw, vpw;  // (bound once: a host weight array is not uploaded per spin)
        HX_TRY(vrw.bind(ring_weights, sizeof(double) * pl->nrp));
        HX_TRY(vpw.bind(pix_weights, sizeof(double) * (size_t)pl->npix));
        for (int j = 0; j < nj; ++j) {
            DevBuf in;
            HX_TRY(in.alloc(sizeof(double) * (size_t)jn[j] * pl->npix));
            HX_TRY(gather_components(in.as<double>(), jn[j], pl->npix, [&](int c) { return jcomp[j][c]; }, nullptr));
            HX_TRY(hx_map2alm(pl, jspin[j], jn[j], in.as<double>(), jalm[j], vrw.as<double>(), vpw.as<double>(), jfl[j], niter));
            HX_HIP(hipStreamSynchronize(rt().stream));  // `in` is released here
        }
    }
    // (the call above has synchronised) alms out: host arrays through the pinned pipeline, device arrays by device copies
    for (int g = 0; g < 2; ++g) {
        const int cpu = g == 0 ? 2 : 1;
        for (size_t u = 0; u < owner[g].size(); ++u) {
            const size_t bytes = sizeof(double2) * (size_t)cpu * pl->nlm;
            const char *src = (const char *)out[g].p + u * bytes;
            double *dst = alms[owner[g][u]];
            if (is_device_ptr(dst)) HX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, rt().stream));
            else HX_TRY(copy_d2h(dst, src, bytes));
        }
    }
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}

