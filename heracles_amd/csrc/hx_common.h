// hx_common.h -- runtime state, error handling and device-buffer helpers shared by the
// translation units of libhxsht.so.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/hxsht.h"

namespace hx {

// ---- error state -------------------------------------------------------------------
void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);

#define HX_HIP(call)                                                                     \
    do {                                                                                 \
        hipError_t _e = (call);                                                          \
        if (_e != hipSuccess)                                                            \
            return ::hx::fail(HX_ERR_HIP, "%s failed: %s (%s:%d)", #call,                \
                              hipGetErrorString(_e), __FILE__, __LINE__);                \
    } while (0)

#define HX_TRY(expr)                                                                     \
    do {                                                                                 \
        int _rc = (expr);                                                                \
        if (_rc != HX_OK) return _rc;                                                    \
    } while (0)

// ---- runtime -----------------------------------------------------------------------
struct Runtime {
    bool ready = false;
    int device = -1;
    int cus = 256;  // compute units of the device (grid size of persistent kernels)
    hipStream_t stream = nullptr;
    hipStream_t copy = nullptr;  // created on first use (copy_stream())
    bool own_stream = false;
    bool async = false;
    bool profiling = false;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    hipEvent_t order_ev = nullptr;  // library stream -> copy stream dependency (hx_mixmat.hip); recreated by hx_init on another device
    struct Prof {
        int launches = 0;
        double ms = 0.0;
        std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    };
    std::map<std::string, Prof> prof;
    std::vector<hipEvent_t> event_pool;
};
Runtime &rt();
int ensure_ready();  // lazily hx_init(current device); HX_ERR_NO_DEVICE if none

// Scoped kernel-family timer: records HIP events on the library stream when profiling.
struct ProfScope {
    const char *name;
    hipEvent_t a = nullptr, b = nullptr;
    explicit ProfScope(const char *n);
    ~ProfScope();
};

// ---- device buffers ----------------------------------------------------------------
bool is_device_ptr(const void *p);
bool is_pinned_host(const void *p);  // page-locked host memory the runtime knows (hipHostMalloc / hipHostRegister)

// Owning device allocation.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int alloc(size_t n);    // (re)allocate exactly n bytes if current capacity < n
    void release();
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// a host vector into a device buffer sized for it (complete on return)
template <class T>
int upload_vec(DevBuf &b, const std::vector<T> &v)
{
    HX_TRY(b.alloc(sizeof(T) * (v.empty() ? 1 : v.size())));
    if (!v.empty()) HX_HIP(hipMemcpy(b.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return HX_OK;
}

// Input view: device pointer as-is, host pointer copied to a temporary device buffer.
struct InView {
    const void *dev = nullptr;
    DevBuf tmp;
    int bind(const void *src, size_t bytes);
    template <class T> const T *as() const { return static_cast<const T *>(dev); }
};

// Output view: device pointer as-is; host pointer -> temporary device buffer, copied back
// by finish().
struct OutView {
    void *dev = nullptr;
    void *host = nullptr;
    size_t bytes = 0;
    DevBuf tmp;
    int bind(void *dst, size_t bytes);
    int finish();
    template <class T> T *as() const { return static_cast<T *>(dev); }
};

// Host <-> device copies on the library stream; large pageable host buffers are staged through
// pinned memory by several host threads.  copy_d2h is complete on return, copy_h2d is stream-ordered.
int copy_h2d(void *dst_dev, const void *src_host, size_t bytes, hipStream_t on = nullptr);  // on: another stream than the library's
void stager_reset_events();  // hx_init on another device: recreate the staging events there
hipStream_t copy_stream();  // second stream of the library (uploads that overlap its kernels); nullptr if it cannot be created
int copy_d2h(void *dst_host, const void *src_dev, size_t bytes, hipStream_t on = nullptr);  // on: another stream than the library's (the caller orders it behind the producer)

int finish_call();  // synchronise unless async

// Scratch budget of one analysis m-chunk in bytes (hx_set_scratch_budget, else HX_SCRATCH_GB); 0 = automatic
double scratch_budget_bytes();

// hx_init on another device: drop the context hx_mixmat / hx_mixmat_eb keep between calls (hx_mixmat.hip)
void mixmat_drop_cache();
void alm2cl_drop_cache();  // hx_twopoint.hip: the buffers hx_alm2cl_pairs keeps between calls
void corr_cache_drop();    // hx_transforms.hip: nodes, weights and Wigner tables hx_cl2corr / hx_corr2cl keep for the last lmax
void synalm_drop_cache();  // hx_synalm.hip: the factor hx_synalm / hx_cl_cholesky keep between calls
void lognormal_drop_cache();  // hx_lognormal.hip: the result, change report, parameters and flag word its calls keep between calls
int rotate_exec_flops(unsigned long long *v, bool reset);  // hx_rotate.hip: FP64 vector flops hx_rotate_alm executed (for hx_executed_flops)
void gausscov_drop_cache();  // hx_gausscov.hip: the folded tables Z and coefficients hx_gauss_cov_accumulate keeps between calls
int gausscov_exec_flops(unsigned long long *v, bool reset);  // hx_gausscov.hip: FP64 vector flops of hx_gauss_cov_accumulate (for hx_executed_flops)

void deproject_drop_cache();  // hx_deproject.hip: the partial tiles and the reduced matrix hx_deproject_gram keeps between calls
int deproject_exec_flops(unsigned long long *v, bool reset);  // hx_deproject.hip: FP64 matrix-instruction flops of hx_deproject_gram (for hx_executed_flops)

int corr_tables_view(int lmax, const double **T, const double **w, int *kpad);  // hx_transforms.hip: those tables, for hx_xi_cols.hip
// hx_transforms.hip: the cached table [lmax + 1][kpad] of the normalised pair (A, B) (wigner_pair_normalise, hx_wigner.h) at the lmax + 1
// Gauss-Legendre nodes and their weights w, for hx_xi_cols.hip (built on first use; see PairCache for how long the pointers hold)
int xi_pair_table_view(int lmax, int A, int B, const double **T, const double **w, int *kpad);

// The two halves of hx_pointsht_adjoint (hx_nufft.hip), for callers that keep grids resident (hx_catalm, hx_catalm.hip).
// Half one: pointsht_order picks the spreading path for n points (tiles from 300000 points, HX_NUFFT_TILES forces it) and sorts them
// by tile when that path is taken -- once for every component spread from these points; pointsht_spread_one ADDS one component
// (val[n] at loc[n] = (theta, phi)) to grid [n1][n1], without clearing it.  The order lives in the buffers of `ps` until its next call.
// Half two: pointsht_grids_to_alm runs the three FFT stages on the grid grid_of(c) hands out for component c, then the Legendre
// analysis: d_alm [ncomp][nlm] on the device.
struct PointOrder {
    bool tiles = false;
    unsigned *key = nullptr, *idx = nullptr;  // sorted (tile, point index) pairs
};
using GridOf = std::function<int(int c, const double **grid)>;
int pointsht_order(hx_pointsht *ps, int64_t npoints, const double2 *loc, PointOrder *o);
int pointsht_spread_one(hx_pointsht *ps, const PointOrder &o, int64_t npoints, const double2 *loc, const double *val, double *grid);
int pointsht_grids_to_alm(hx_pointsht *ps, int spin, int ncomp, const GridOf &grid_of, double2 *d_alm);
// The two halves of hx_pointsht_synthesis, the forward direction (alm -> values at the points), for callers that keep grids resident
// (hx_pointgrid).  Half one does not depend on the points: pointsht_alm_to_grids runs the Legendre synthesis sweeps and the three
// transposed FFT stages; component c's grid [n1][n1] is written where grid_for(c) says, and grid_done(c, grid) (may be empty) is called
// once its stages are queued -- a caller with one grid gathers from it there.  d_alm: [ncomp][nlm] on the device.
// Half two: pointsht_gather_one reads one component at n points, ordered by pointsht_order as for the spread (the same tile rule):
// val[n], NaN at points outside the sphere, which are counted in the object's nbad.
using GridFor = std::function<int(int c, double **grid)>;
using GridDone = std::function<int(int c, const double *grid)>;
int pointsht_alm_to_grids(hx_pointsht *ps, int spin, int ncomp, const double2 *d_alm, const GridFor &grid_for, const GridDone &grid_done);
int pointsht_gather_one(hx_pointsht *ps, const PointOrder &o, int64_t npoints, const double2 *loc, const double *grid, double *val);

}  // namespace hx
