// hx_mixmat.hip -- mode-coupling (mixing) matrices: the context of one (l1max, l2max, l3max), its products and its entry points.
//
// Replaces convolvecl.mixmat / mixmat_eb as called at heracles/twopoint.py:378-388:
//   M_{l1 l2} = (2 l2 + 1)/(4 pi) sum_{l3} (2 l3 + 1) W_{l3} (l1 l2 l3; s1 -s1 0)(l1 l2 l3; s2 -s2 0)
// evaluated in its dense quadrature form:
//   xi(x) = sum_{l3} (2 l3 + 1)/(4 pi) W_{l3} P_{l3}(x)
//   G^{(ab)} = D^{(ab)T} diag(w xi) D^{(ab)} diag((2 l2 + 1)/2),   D^{(ab)}[k][l] = d^l_{ab}(x_k)
// on N >= (l1max + l2max + l3max)/2 + 1 Gauss-Legendre nodes, which is exact.  Fields of any spin weights (s1, s2) are served, and
// their matrices are DEFINED by the quadrature form: G^{(s1,s2)} is (-1)^{s1+s2} times the product of 3j symbols above, so for odd
// s1 + s2 the bare formula gives minus the identity for a full-sky mask and the quadrature form the identity (pseudo-Cl = M Cl).  The
// nodes and the tables D^{(ab)} come from hx_wigner.hip; the (l, l') contraction is a symmetric FP64 GEMM on the matrix unit
// (hx_gemm.hip), its tile order a host function (hx_mix_tiles.h).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hx_dd.h"
#include "hx_gemm.h"
#include "hx_mix_tiles.h"
#include "hx_wigner.h"

namespace hx {

static_assert(sizeof(MixTile) == sizeof(int2) && offsetof(MixTile, x) == offsetof(int2, x) && offsetof(MixTile, y) == offsetof(int2, y),
              "the tile list is uploaded as it stands and read as int2");

// ---- node weights s_k = w_k xi(x_k + xlo_k), xi = sum_l (2 l + 1) / (4 pi) W_l P_l --------------------------------------------------
// (Round 5: k_weight_xi_dd, one thread per node running the P_l recurrence and the sum in double-double: 1.6 ms per mask at L = 6144.)
// As a matrix-vector product over the (0,0) table (round 6): T0[l][k] = P_l(x_k + xlo_k) is in HBM anyway (built in
// double-double, rounded once), so  s_k = w_k sum_l (2 l + 1) / (4 pi) W_l T0[l][k]  needs no recurrence -- that kernel ran ONE
// dependent chain of 6144 double-double steps per node, 1.6 ms per mask at L = 6144 whatever the GPU could do beside it (9217 nodes:
// 145 waves), three quarters of a binned mixing-matrix key.  Here a block takes 64 nodes x a slice of the multipoles (4 sub-slices
// of it across its waves), every partial sum is compensated (two_sum) and the slices are added in fixed order: the rounding of the table
// entries is random from l to l (1e-16 of each term), unlike the node errors the double-double tables exist for.
constexpr int XI_SLICES = 8;
__global__ __launch_bounds__(256) void k_xi_partial(int l3max, int kpad, const double *__restrict__ cl, const double *__restrict__ T0,
                                                    double2 *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double2 red[4][64];
    const int k = blockIdx.x * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6;
    const int nl = l3max + 1, per = (nl + XI_SLICES * 4 - 1) / (XI_SLICES * 4);
    const int l0 = (blockIdx.y * 4 + sub) * per, l1 = min(l0 + per, nl);
    double sum = 0.0, comp = 0.0;
    if (k < kpad) {
        for (int l = l0; l < l1; ++l) {
            const double v = ((2.0 * l + 1.0) / (4.0 * M_PI) * cl[l]) * T0[(long long)l * kpad + k];
            const double t = sum + v, bb = t - sum;
            comp += (sum - (t - bb)) + (v - bb);
            sum = t;
        }
    }
    red[sub][threadIdx.x & 63] = make_double2(sum, comp);
    __syncthreads();
    if (sub == 0 && k < kpad) {
        DD a = dd_quick(red[0][threadIdx.x].x, red[0][threadIdx.x].y);
#pragma unroll
        for (int q = 1; q < 4; ++q) a = dd_add(a, dd_quick(red[q][threadIdx.x].x, red[q][threadIdx.x].y));
        part[(long long)blockIdx.y * kpad + k] = make_double2(a.h, a.l);
    }
}
__global__ void k_xi_finish(int n, int kpad, const double *__restrict__ w, const double2 *__restrict__ part, double *__restrict__ s)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    DD a = DD{part[k].x, part[k].y};
    for (int q = 1; q < XI_SLICES; ++q) a = dd_add(a, DD{part[(long long)q * kpad + k].x, part[(long long)q * kpad + k].y});
    s[k] = w[k] * (a.h + a.l);
}

// out0 = (a + b)/2, out1 = (a - b)/2, out2 = b   (a = G22 in out0, b = G2-2 in out2)
__global__ void k_eb_combine(long long n, double *__restrict__ o0, double *__restrict__ o1,
                             const double *__restrict__ o2)
{
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long st = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += st) {
        const double a = o0[i], b = o2[i];
        o0[i] = 0.5 * (a + b);
        o1[i] = 0.5 * (a - b);
    }
}

// ---- binned rows (heracles.twopoint.mixing_matrices(bins=, weights=): heracles/twopoint.py:391-397 -> heracles/result.py:124-248) ----
// The reference bins the OUTPUT multipole of every matrix on the host, column by column (5 s per (3, 6145, 6145) matrix).  Binning is
// linear in the rows, so with the mask-independent binned tables
//     Tb[b][k] = sum_{l in bin b} w_l d^l(x_k)
// the numerators of the binned matrix are the SKINNY product  sum_k Tb[b][k] s_k T[l2][k] (2 l2 + 1) / 2  --  (nbins x N)(N x L2):
// ~200x fewer flops than the full matrix at 32 bins, one read of the table from HBM (0.46 GB at L = 6144) and nbins x (l2max + 1)
// doubles to the host instead of 0.9 GB.
//
// k_bin_table: one thread per node, the rows of a bin in ascending l with a compensated sum (the terms oscillate in l and cancel).
__global__ __launch_bounds__(256) void k_bin_table(int kpad, const int *__restrict__ start, const int *__restrict__ rows, const double *__restrict__ rw,
                                                   const double *__restrict__ T, double *__restrict__ Tb)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (k >= kpad) return;
    double sum = 0.0, comp = 0.0;
    for (int e = start[b]; e < start[b + 1]; ++e) {
        const double v = rw[e] * T[(long long)rows[e] * kpad + k];
        const double t = sum + v, bb = t - sum;
        comp += (sum - (t - bb)) + (v - bb);  // two_sum
        sum = t;
    }
    Tb[(long long)b * kpad + k] = sum + comp;
}

// partial[ks][b][j] = sum_{k in share ks} A[b][k] B[j][k]:  A = Tb diag(s) [nbpad][kpad], B = T [rows_pad][kpad].
// A wave owns 16 columns j and MT tiles of 16 bins; a lane brings 32 contiguous bytes (4 nodes) of one row of each operand per
// step, so the four matrix instructions of a step contract the nodes k + 4 (lane >> 4) + {0, 1, 2, 3} -- any order is fine as long as
// A and B agree.  B (the big table) streams from HBM once, 128 contiguous bytes per row and step; A stays in L2.  The node range is cut
// into gridDim.y shares (enough work-groups to fill the chip); k_binned_finish adds them in fixed order.
template <int MT>
__global__ __launch_bounds__(256) void k_binned_gemm(const double *__restrict__ A, const double *__restrict__ B, int kpad, int kchunk, int nbpad, int l2pad,
                                                     double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 15, kg = lane >> 4;
    const int c0 = (blockIdx.x * 4 + w) * 16, b0 = blockIdx.z * (MT * 16);
    const int k0 = blockIdx.y * kchunk, k1 = min(k0 + kchunk, kpad);
    const double *pb = B + (long long)(c0 + r) * kpad + kg * 4;
    const double *pa = A + (long long)(b0 + r) * kpad + kg * 4;
    double4_t acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
    int k = k0;
    for (; k + 64 <= k1; k += 64) {  // four steps of B in flight
        double4_t b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = *reinterpret_cast<const double4_t *>(pb + k + 16 * u);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            double4_t a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = *reinterpret_cast<const double4_t *>(pa + (long long)t * 16 * kpad + k + 16 * u);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int h = 0; h < 4; ++h) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][h], b[u][h], acc[t], 0, 0, 0);
        }
    }
    for (; k < k1; k += 16) {
        const double4_t b = *reinterpret_cast<const double4_t *>(pb + k);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const double4_t a = *reinterpret_cast<const double4_t *>(pa + (long long)t * 16 * kpad + k);
#pragma unroll
            for (int h = 0; h < 4; ++h) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[h], b[h], acc[t], 0, 0, 0);
        }
    }
    // D layout: row = (lane >> 4) + 4 * reg, col = lane & 15
    double *po = partial + ((long long)blockIdx.y * nbpad + b0) * l2pad + c0 + r;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) po[(long long)(t * 16 + kg + 4 * q) * l2pad] = acc[t][q];
}

// out[b][j] = ratio(colscale[j] * sum_ks partial[ks][b][j], norm[b]), ratio(n, d) = n / d where n != 0, else 0 (the reference's rule:
// heracles/result.py:132-135).  EB: pa = the (2,2) product, pb = the (2,-2) product -> [0] = (a + b) / 2, [1] = (a - b) / 2, [2] = b.
template <bool EB>
__global__ __launch_bounds__(256) void k_binned_finish(int nbins, int n2, int nbpad, int l2pad, int ksplit, const double *__restrict__ pa,
                                                       const double *__restrict__ pb, const double *__restrict__ colscale,
                                                       const double *__restrict__ norm, double *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= n2) return;
    const long long slab = (long long)nbpad * l2pad, at = (long long)b * l2pad + j;
    double a = 0.0, c = 0.0;
    for (int ks = 0; ks < ksplit; ++ks) {
        a += pa[ks * slab + at];
        if (EB) c += pb[ks * slab + at];
    }
    const double cs = colscale[j], nb = norm[b];
    auto ratio = [nb](double v) { return v != 0.0 ? v / nb : 0.0; };
    const long long o = (long long)b * n2 + j, sz = (long long)nbins * n2;
    if (EB) {
        a *= cs;
        c *= cs;
        out[o] = ratio(0.5 * (a + c));
        out[o + sz] = ratio(0.5 * (a - c));
        out[o + 2 * sz] = ratio(c);
    } else {
        out[o] = ratio(a * cs);
    }
}

// Everything of a mixing-matrix build that does not depend on the mask: Gauss-Legendre nodes, the Wigner-d tables
// T_ab[l][k] = d^l_ab(x_k) of the products asked for, the tile list and the column scaling (2 l2 + 1) / 2.  One context
// serves any number of masks: per mask only the node weights s_k = w_k xi(x_k) and one GEMM per product remain
// (the reference calls convolvecl once per (field pair, bin pair), heracles/twopoint.py:354-397, rebuilding all of it).
typedef WigTable MixTable;  // T: the table [rows_pad][kpad], Tb: its binned rows [nbpad][kpad] (hx_mixctx_set_bins)
struct MixCtx {
    int l1max = -1, l2max = -1, l3max = -1, L = 0, n = 0, kpad = 0, rows_pad = 0;
    GLNodes gl;  // node k = x[k] + xlo[k]
    DevBuf s, d_tiles, d_cs;
    size_t ntiles = 0;
    // Tables by normalised pair (a >= |b|: G^{(ab)} is the same for (a, b), (b, a) and (-b, -a), see wigner_pair_normalise).  (0,0) is
    // pinned and never dropped: the node weights of every mask read it.  Of the others at most max_tabs are kept
    // (HX_MIX_TABLES at creation; 16 holds every pair of a job with spins {0, 1, 2, 3}: three (s, 0) and twelve (s1, +-s2)), the one
    // used longest ago goes first.  A table is rows_pad x kpad doubles: 0.46 GB at L = 6144.
    WigTableSet tabs;
    DevBuf cl;              // the mask spectrum in hand, l3max + 1 values (mix_set_mask)
    DevBuf Ts;              // T diag(s) of the product in hand (k_mixmat_gemm_dma)
    DevBuf xi_part;         // slices of the node weights of the mask in hand (k_xi_partial)
    // binned rows (hx_mixctx_set_bins): bin lists of the output multipole, binned tables Tb_t[nbpad][kpad] per product
    int nbins = 0, nbpad = 0, l2pad = 0, ksplit = 1, kchunk = 0;
    DevBuf b_start, b_rows, b_w, b_norm;
    DevBuf Tbs, part[2], b_out;  // (b_out: device image of a host destination, kept between calls)
    // page-locked landing buffer of a binned result on its way to a pageable destination (the GPU writes it by DMA; the bytes are then
    // copied on by the host): straight into a fresh numpy array, the runtime pins the caller's pages call by call -- 3 ms per 1.5 MB key in
    // a process that holds a plan's scratch, against 0.15 ms this way (tools/exp_mixmat_list_env.py)
    void *b_pin = nullptr;
    size_t b_pin_bytes = 0;
    MixCtx() = default;
    MixCtx(const MixCtx &) = delete;
    MixCtx &operator=(const MixCtx &) = delete;
    ~MixCtx()
    {
        if (b_pin) (void)hipHostFree(b_pin);
    }
};
static int mix_ctx_init(MixCtx &c, int l1max, int l2max, int l3max)
{
    c.l1max = l1max; c.l2max = l2max; c.l3max = l3max;
    c.L = std::max(l1max, l2max);
    c.n = (l1max + l2max + l3max) / 2 + 1;
    c.kpad = (c.n + GK - 1) / GK * GK;
    c.rows_pad = (c.L + 1 + GB - 1) / GB * GB;
    WigTableSet &ts = c.tabs;
    ts.lmax = c.L; ts.rows = c.rows_pad; ts.kpad = c.kpad; ts.max_tabs = 16;
    if (const char *e = getenv("HX_MIX_TABLES")) ts.max_tabs = std::max(1, atoi(e));
    // (the (0,0) table = P_l(x_k) also feeds the node weights xi(x_k) of every mask, a sum over l <= l3max: its rows run that far)
    ts.pin_a = ts.pin_b = 0;
    ts.pin_lmax = std::max(c.L, c.l3max);
    ts.pin_rows = (ts.pin_lmax + 1 + GB - 1) / GB * GB;
    HX_TRY(c.gl.ensure(c.n, true));
    HX_TRY(c.s.alloc(sizeof(double) * c.kpad));
    const std::vector<MixTile> tiles = mix_tile_order(c.rows_pad / GB);
    c.ntiles = tiles.size();
    HX_TRY(upload_vec(c.d_tiles, tiles));
    std::vector<double> cs(c.rows_pad, 0.0);
    for (int l = 0; l <= c.L; ++l) cs[l] = (2.0 * l + 1.0) / 2.0;
    HX_TRY(upload_vec(c.d_cs, cs));
    return HX_OK;
}

// the table of the pair (a, b), built on first use; *out stays valid until the next call of this function
static int mix_ctx_table(MixCtx &c, int a, int b, MixTable **out)
{
    int A, B;
    (void)wigner_pair_normalise(a, b, &A, &B);
    return c.tabs.get(c.gl, A, B, out);
}

// One mask spectrum (host or device, zero-padded / truncated to l3max + 1 values) becomes the mask in hand: its node weights
// s_k = w_k xi(x_k) are a matrix-vector product over the (0,0) table
static int mix_set_mask(MixCtx &c, const double *cl, int ncl)
{
    hipStream_t st = rt().stream;
    const int nl = c.l3max + 1, ncopy = std::min(ncl, nl);
    HX_TRY(c.cl.alloc(sizeof(double) * nl));
    if (is_device_ptr(cl)) {
        HX_HIP(hipMemsetAsync(c.cl.p, 0, sizeof(double) * nl, st));
        HX_HIP(hipMemcpyAsync(c.cl.p, cl, sizeof(double) * ncopy, hipMemcpyDeviceToDevice, st));
    } else {
        std::vector<double> h(nl, 0.0);
        std::copy(cl, cl + ncopy, h.begin());
        HX_HIP(hipMemcpy(c.cl.p, h.data(), sizeof(double) * nl, hipMemcpyHostToDevice));
    }
    MixTable *t0 = nullptr;
    HX_TRY(mix_ctx_table(c, 0, 0, &t0));
    HX_TRY(c.xi_part.alloc(sizeof(double2) * (size_t)XI_SLICES * c.kpad));
    HX_HIP(hipMemsetAsync(c.s.p, 0, sizeof(double) * c.kpad, st));
    ProfScope ps("weight_xi");
    hipLaunchKernelGGL(k_xi_partial, dim3((c.kpad + 63) / 64, XI_SLICES), dim3(256), 0, st, c.l3max, c.kpad, c.cl.as<double>(), t0->T.as<double>(), c.xi_part.as<double2>());
    hipLaunchKernelGGL(k_xi_finish, dim3((c.n + 255) / 256), dim3(256), 0, st, c.n, c.kpad, c.gl.w.as<double>(), c.xi_part.as<double2>(), c.s.as<double>());
    HX_HIP(hipGetLastError());
    return HX_OK;
}

// G^{(ab)} of the mask in hand into d_out (device, (l1max + 1) x (l2max + 1), ld = l2max + 1)
static int mix_ctx_product(MixCtx &c, int a, int b, double *d_out)
{
    MixTable *t = nullptr;
    HX_TRY(mix_ctx_table(c, a, b, &t));
    if (!c.Ts.p) HX_TRY(c.Ts.alloc(sizeof(double) * (size_t)c.rows_pad * c.kpad));
    return launch_gemm_sym(t->T.as<double>(), c.rows_pad, c.kpad, c.s.as<double>(), c.Ts.as<double>(), c.d_tiles.as<int2>(), c.ntiles, c.l1max + 1,
                           c.l2max + 1, c.d_cs.as<double>(), d_out, (long long)(c.l2max + 1));
}

// ---- the context and the staging buffer of the one-shot entry points, kept between calls ------------------------------------------
// hx_mixmat / hx_mixmat_eb / hx_mixmat_batch used to build and free a context per call: nodes, two or three 0.46 GB tables, the 0.46 GB
// scaled table and -- for a host destination -- a 0.9 GB staging buffer at L = 6144, i.e. ~3 GB of hipMalloc / hipFree per build.  Every
// second or third build of a row then took 0.12-0.18 s instead of 0.031 (BENCH_r04 seconds_all; round 5's first run: builds 2, 5 and 8 of a
// row, whatever the destination's kind, never with a device destination): the driver's unmapping of the freed blocks catching up.  The
// tables do not depend on the mask, so the last context is kept (one (l1max, l2max, l3max) at a time, as hx_mixctx_* keeps its own), and
// so is the staging buffer: a build allocates nothing.  hx_mixmat_release() frees both; hx_init on another device drops them.
struct MixCache {
    MixCtx *ctx = nullptr;
    DevBuf out_tmp;
    int device = -1;
};
static MixCache &mix_cache()
{
    static MixCache *c = new MixCache;  // (never destroyed: its buffers must not be freed behind the HIP runtime's back at process exit)
    return *c;
}
static void mix_cache_drop()
{
    MixCache &mc = mix_cache();
    delete mc.ctx;
    mc.ctx = nullptr;
    mc.out_tmp.release();
}
static int mix_cached_ctx(int l1max, int l2max, int l3max, MixCtx **out)
{
    MixCache &mc = mix_cache();
    if (mc.device != rt().device) {
        mix_cache_drop();
        mc.device = rt().device;
    }
    if (!mc.ctx || mc.ctx->l1max != l1max || mc.ctx->l2max != l2max || mc.ctx->l3max != l3max) {
        if (mc.ctx) HX_HIP(hipStreamSynchronize(rt().stream));
        delete mc.ctx;
        mc.ctx = new MixCtx;
        const int rc = mix_ctx_init(*mc.ctx, l1max, l2max, l3max);
        if (rc != HX_OK) {
            delete mc.ctx;
            mc.ctx = nullptr;
            return rc;
        }
    }
    *out = mc.ctx;
    return HX_OK;
}
}  // namespace hx
void hx::mixmat_drop_cache() { hx::mix_cache_drop(); }
namespace hx {
// destination of a one-shot build: a device pointer as it is, a host pointer through the cached staging buffer
static int mix_bind_out(OutView &vo, double *out, size_t bytes)
{
    vo.bytes = bytes;
    if (is_device_ptr(out)) {
        vo.dev = out;
        vo.host = nullptr;
        return HX_OK;
    }
    HX_TRY(mix_cache().out_tmp.alloc(bytes));
    vo.dev = mix_cache().out_tmp.p;
    vo.host = out;
    return HX_OK;
}
// The three matrices of two fields of non-zero spin weights s1, s2 > 0 for one mask (context c, node weights set) into vo = [3][n1][n2].
// b = G^{(s1,-s2)} first: it IS the third matrix, so a host destination receives it (second stream, ~5 ms at L = 6144) while the
// product a = G^{(s1,s2)} is computed; then [0] = (a + b) / 2, [1] = (a - b) / 2.  Complete on return for a host destination.
static int mix_eb_into(MixCtx &c, OutView &vo, int s1, int s2)
{
    const size_t sz = (size_t)(c.l1max + 1) * (c.l2max + 1);
    double *o0 = vo.as<double>(), *o1 = o0 + sz, *o2 = o0 + 2 * sz;
    hipStream_t st = rt().stream;
    MixTable *ta = nullptr;
    HX_TRY(mix_ctx_product(c, s1, -s2, o2));
    HX_TRY(mix_ctx_table(c, s1, s2, &ta));
    hipStream_t cs = vo.host ? copy_stream() : nullptr;
    if (cs) {
        Runtime &r = rt();
        if (!r.order_ev) HX_HIP(hipEventCreateWithFlags(&r.order_ev, hipEventDisableTiming));
        HX_HIP(hipEventRecord(r.order_ev, st));
        HX_HIP(hipStreamWaitEvent(cs, r.order_ev, 0));
    }
    HX_TRY(mix_ctx_product(c, s1, s2, o0));
    if (cs) HX_TRY(copy_d2h((double *)vo.host + 2 * sz, o2, sizeof(double) * sz, cs));  // (complete on return; the product above runs meanwhile)
    hipLaunchKernelGGL(k_eb_combine, dim3(1024), dim3(256), 0, st, (long long)sz, o0, o1, o2);
    HX_HIP(hipGetLastError());
    if (cs) {
        HX_TRY(copy_d2h(vo.host, o0, sizeof(double) * 2 * sz));
    } else {
        HX_TRY(vo.finish());
    }
    return HX_OK;
}

// The spins of a request by magnitude, checked against HX_MAX_MIX_SPIN.  Both non-zero (eb): three matrices, as mix_eb_into writes
// them; else one matrix, G^{(s,0)} of the non-zero spin, which is brought to s1.
static int mix_spins(const char *who, int &s1, int &s2, bool &eb)
{
    s1 = abs(s1);
    s2 = abs(s2);
    eb = s1 && s2;
    if (std::max(s1, s2) > HX_MAX_MIX_SPIN) return fail(HX_ERR_UNSUPPORTED, "%s: spin %d beyond the supported %d", who, std::max(s1, s2), HX_MAX_MIX_SPIN);
    if (!eb) {
        s1 = std::max(s1, s2);
        s2 = 0;
    }
    return HX_OK;
}
// the spins of a `kind` of hx_mixctx_apply / hx_mixctx_apply_binned / hx_mixmat_batch: 1 -> (0,0), 2 -> (2,0), 4 -> (2,2)
static bool mix_kind_spins(int kind, int &s1, int &s2)
{
    s1 = kind == 1 ? 0 : 2;
    s2 = kind == 4 ? 2 : 0;
    return kind == 1 || kind == 2 || kind == 4;
}
// The matrices of the mask in hand for spins as mix_spins leaves them into out (host or device): (l1max + 1, l2max + 1), three of them
// where both spins are non-zero.  Complete on return.
static int mix_emit(MixCtx &c, int s1, int s2, double *out)
{
    const bool eb = s1 && s2;
    OutView vo;
    HX_TRY(mix_bind_out(vo, out, sizeof(double) * (size_t)(c.l1max + 1) * (c.l2max + 1) * (eb ? 3 : 1)));
    if (eb) {
        HX_TRY(mix_eb_into(c, vo, s1, s2));
    } else {
        HX_TRY(mix_ctx_product(c, s1, 0, vo.as<double>()));
        HX_TRY(vo.finish());
    }
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}

}  // namespace hx

using namespace hx;

static int mixmat_args(const double *cl, int ncl, int l1max, int l2max, int l3max, double *out)
{
    if (!cl || !out || ncl < 1 || l1max < 0 || l2max < 0 || l3max < 0)
        return fail(HX_ERR_ARG, "mixmat: bad argument");
    return HX_OK;
}

extern "C" int hx_mixmat(const double *cl, int ncl, int l1max, int l2max, int l3max, int s1, int s2, double *out)
{
    HX_TRY(ensure_ready());
    HX_TRY(mixmat_args(cl, ncl, l1max, l2max, l3max, out));
    if (s1 != 0 && s2 != 0) return fail(HX_ERR_UNSUPPORTED, "hx_mixmat: spin (%d,%d) not supported (use hx_mixmat_eb_spin for two non-zero spins)", s1, s2);
    bool eb = false;
    HX_TRY(mix_spins("hx_mixmat", s1, s2, eb));
    MixCtx *c = nullptr;
    HX_TRY(mix_cached_ctx(l1max, l2max, l3max, &c));
    HX_TRY(mix_set_mask(*c, cl, ncl));
    return mix_emit(*c, s1, s2, out);
}

extern "C" int hx_mixmat_eb_spin(const double *cl, int ncl, int l1max, int l2max, int l3max, int s1, int s2, double *out)
{
    HX_TRY(ensure_ready());
    HX_TRY(mixmat_args(cl, ncl, l1max, l2max, l3max, out));
    if (s1 == 0 || s2 == 0) return fail(HX_ERR_UNSUPPORTED, "hx_mixmat_eb_spin: spin (%d,%d): three matrices need two non-zero spins (hx_mixmat serves the others)", abs(s1), abs(s2));
    bool eb = false;
    HX_TRY(mix_spins("hx_mixmat_eb_spin", s1, s2, eb));
    MixCtx *c = nullptr;
    HX_TRY(mix_cached_ctx(l1max, l2max, l3max, &c));
    HX_TRY(mix_set_mask(*c, cl, ncl));
    return mix_emit(*c, s1, s2, out);
}

extern "C" int hx_mixmat_eb(const double *cl, int ncl, int l1max, int l2max, int l3max, double *out)
{
    return hx_mixmat_eb_spin(cl, ncl, l1max, l2max, l3max, 2, 2, out);
}

// Frees what hx_mixmat / hx_mixmat_eb / hx_mixmat_batch keep between calls (the tables of the last (l1max, l2max, l3max) and the
// staging buffer of a host destination: ~3 GB at L = 6144).  The next build allocates them again.
extern "C" int hx_mixmat_release(void)
{
    if (rt().ready) (void)hipStreamSynchronize(rt().stream);
    mix_cache_drop();
    return HX_OK;
}

// y[v][i] = sum_j M[i][j] x[v][j]: the products of heracles.twopoint.apply_mixing_matrix (heracles/twopoint.py:497-524: `_M @ cl` per
// component spectrum).  One wave per row, the row read once for all nvec <= 4 vectors (HBM-bound: 8 B per matrix element).
__global__ __launch_bounds__(256) void k_matvec(int n, int m, long long ld, const double *__restrict__ M, int nvec, const double *__restrict__ x,
                                                double *__restrict__ y)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const double *r = M + (long long)row * ld;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = lane; j < m; j += 64) {
        const double a = r[j];
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (v < nvec) acc[v] = fma(a, x[(long long)v * m + j], acc[v]);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        double t = acc[v];
        for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);  // fixed order: bitwise repeatable
        if (lane == 0 && v < nvec) y[(long long)v * n + row] = t;
    }
}

extern "C" int hx_matvec(int n, int m, const double *M, int nvec, const double *x, double *y)
{
    HX_TRY(ensure_ready());
    if (n < 0 || m < 0 || nvec < 0 || ((n > 0 && m > 0 && nvec > 0) && (!M || !x || !y))) return fail(HX_ERR_ARG, "hx_matvec: bad arguments");
    if (n == 0 || nvec == 0) return HX_OK;
    InView vm, vx;
    OutView vy;
    HX_TRY(vm.bind(M, sizeof(double) * (size_t)n * std::max(m, 1)));
    HX_TRY(vx.bind(x, sizeof(double) * (size_t)nvec * std::max(m, 1)));
    HX_TRY(vy.bind(y, sizeof(double) * (size_t)nvec * n));
    for (int v0 = 0; v0 < nvec; v0 += 4) {
        const int nv = std::min(4, nvec - v0);
        hipLaunchKernelGGL(k_matvec, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, rt().stream, n, m, (long long)m, vm.as<double>(), nv,
                           vx.as<double>() + (size_t)v0 * m, vy.as<double>() + (size_t)v0 * n);
        HX_HIP(hipGetLastError());
    }
    HX_TRY(vy.finish());
    return finish_call();
}

// Mixing matrices of nmask mask spectra for one (l1max, l2max, l3max): nodes, Wigner-d tables and tile list are built once,
// then every mask costs its node weights and one GEMM per product.  Replaces the serial loop of convolvecl calls in
// heracles.twopoint.mixing_matrices (heracles/twopoint.py:354-397).
//   cls   [nmask][ncl] (host or device), zero-padded / truncated to l3max + 1 like hx_mixmat
//   kinds [nmask] bit mask: 1 spin (0,0) -> out00[k], 2 spin (0,2) / (2,0) -> out02[k], 4 spin (2,2) -> outeb[k] (3 matrices)
//   out*  [nmask] pointers (host or device; entries of kinds not asked for are ignored and may be NULL)
extern "C" int hx_mixmat_batch(int nmask, const double *cls, int ncl, int l1max, int l2max, int l3max, const int *kinds,
                               double *const *out00, double *const *out02, double *const *outeb)
{
    HX_TRY(ensure_ready());
    if (nmask < 0 || (nmask > 0 && (!cls || !kinds)) || ncl < 1 || l1max < 0 || l2max < 0 || l3max < 0)
        return fail(HX_ERR_ARG, "hx_mixmat_batch: bad argument");
    if (nmask == 0) return HX_OK;
    for (int k = 0; k < nmask; ++k)
        if ((kinds[k] & ~7) || ((kinds[k] & 1) && (!out00 || !out00[k])) || ((kinds[k] & 2) && (!out02 || !out02[k])) ||
            ((kinds[k] & 4) && (!outeb || !outeb[k])))
            return fail(HX_ERR_ARG, "hx_mixmat_batch: mask %d: kinds=%d without an output buffer", k, kinds[k]);
    MixCtx *c = nullptr;
    HX_TRY(mix_cached_ctx(l1max, l2max, l3max, &c));
    double *const *outs[3] = {out00, out02, outeb};
    for (int k = 0; k < nmask; ++k) {
        if (!kinds[k]) continue;
        HX_TRY(mix_set_mask(*c, cls + (size_t)k * ncl, ncl));  // (the node weights: once per mask)
        for (int bit = 0; bit < 3; ++bit)
            if (kinds[k] & (1 << bit)) {
                int s1, s2;
                (void)mix_kind_spins(1 << bit, s1, s2);
                HX_TRY(mix_emit(*c, s1, s2, outs[bit][k]));
            }
    }
    return HX_OK;
}

// ---- the same as an object: tables built once, masks streamed through (the outputs of a 13-bin job do not fit in memory
// at once; the reference's `out` mapping may write each matrix to disk as it arrives, heracles/twopoint.py:393-397) ----
struct hx_mixctx {
    hx::MixCtx c;
};

extern "C" hx_mixctx *hx_mixctx_create(int l1max, int l2max, int l3max)
{
    if (ensure_ready() != HX_OK) return nullptr;
    if (l1max < 0 || l2max < 0 || l3max < 0) {
        set_error("hx_mixctx_create: bad argument");
        return nullptr;
    }
    hx_mixctx *x = new hx_mixctx;
    if (mix_ctx_init(x->c, l1max, l2max, l3max) != HX_OK || hipStreamSynchronize(rt().stream) != hipSuccess) {
        delete x;
        return nullptr;
    }
    return x;
}

extern "C" void hx_mixctx_destroy(hx_mixctx *x)
{
    if (!x) return;
    if (rt().ready) (void)hipStreamSynchronize(rt().stream);
    delete x;
}

// spins (s1, s2) by magnitude: one of them zero -> out (l1max+1, l2max+1); both non-zero -> out (3, l1max+1, l2max+1) as hx_mixmat_eb_spin
extern "C" int hx_mixctx_apply_spin(hx_mixctx *x, const double *cl, int ncl, int s1, int s2, double *out)
{
    HX_TRY(ensure_ready());
    if (!x || !cl || !out || ncl < 1) return fail(HX_ERR_ARG, "hx_mixctx_apply_spin: bad argument");
    bool eb = false;
    HX_TRY(mix_spins("hx_mixctx_apply_spin", s1, s2, eb));
    HX_TRY(mix_set_mask(x->c, cl, ncl));
    return mix_emit(x->c, s1, s2, out);  // (the staging buffer of a host destination is the one-shot cache's, kept between calls)
}

// kind 1: spin (0,0) -> out (l1max+1, l2max+1); 2: spin (0,2)/(2,0) -> the same shape; 4: spin (2,2) -> out (3, l1max+1, l2max+1)
extern "C" int hx_mixctx_apply(hx_mixctx *x, const double *cl, int ncl, int kind, double *out)
{
    int s1, s2;
    if (!mix_kind_spins(kind, s1, s2)) return fail(HX_ERR_ARG, "hx_mixctx_apply: bad argument");
    return hx_mixctx_apply_spin(x, cl, ncl, s1, s2, out);
}

// ---- binned rows: heracles.twopoint.mixing_matrices(..., bins, weights) (heracles/twopoint.py:391-397) ----------------------------
// which [l1max + 1]: bin of output multipole l (0 .. nbins - 1) or -1 (in no bin); w [l1max + 1]: its weight; norm [nbins]: the
// divisor of bin b (the reference: the summed weight).  Host arrays.  The binned tables are built on the first product that needs them.
extern "C" int hx_mixctx_set_bins(hx_mixctx *x, int nbins, const int *which, const double *w, const double *norm)
{
    HX_TRY(ensure_ready());
    if (!x || nbins < 1 || !which || !w || !norm) return fail(HX_ERR_ARG, "hx_mixctx_set_bins: bad argument");
    MixCtx &c = x->c;
    const int n1 = c.l1max + 1;
    for (int l = 0; l < n1; ++l)
        if (which[l] < -1 || which[l] >= nbins) return fail(HX_ERR_ARG, "hx_mixctx_set_bins: which[%d] = %d outside [-1, %d)", l, which[l], nbins);
    HX_HIP(hipStreamSynchronize(rt().stream));  // (a product of the previous bins may still be reading the lists)
    std::vector<int> start(nbins + 1, 0), rows;
    std::vector<double> rw;
    for (int b = 0; b < nbins; ++b) {
        for (int l = 0; l < n1; ++l)
            if (which[l] == b) {
                rows.push_back(l);
                rw.push_back(w[l]);
            }
        start[b + 1] = (int)rows.size();
    }
    c.nbins = nbins;
    c.nbpad = nbins <= 16 ? 16 : nbins <= 32 ? 32 : (nbins + 63) / 64 * 64;
    c.l2pad = (c.l2max + 1 + 63) / 64 * 64;  // (<= rows_pad: the tables are zero-padded to multiples of 128 rows)
    // enough work-groups for every CU to hold a few: the node range in shares of a multiple of 16
    const int mt = std::min(c.nbpad / 16, 4), groups = (c.l2pad / 64) * (c.nbpad / (16 * mt));
    int want = std::max(1, (4 * rt().cus + groups - 1) / groups);
    c.kchunk = std::max(64, ((c.kpad + want - 1) / want + 15) / 16 * 16);
    c.ksplit = (c.kpad + c.kchunk - 1) / c.kchunk;
    HX_TRY(upload_vec(c.b_start, start));
    HX_TRY(upload_vec(c.b_rows, rows));
    HX_TRY(upload_vec(c.b_w, rw));
    std::vector<double> nv(norm, norm + nbins);
    HX_TRY(upload_vec(c.b_norm, nv));
    c.tabs.pinned.have_b = false;
    for (auto &t : c.tabs.tabs) t->have_b = false;
    return HX_OK;
}

namespace hx {
static int mix_ctx_binned_table(MixCtx &c, int a, int b, MixTable **out)
{
    MixTable *t = nullptr;
    HX_TRY(mix_ctx_table(c, a, b, &t));
    *out = t;
    if (t->have_b) return HX_OK;
    const size_t nel = (size_t)c.nbpad * c.kpad;
    HX_TRY(t->Tb.alloc(sizeof(double) * nel));
    HX_HIP(hipMemsetAsync(t->Tb.p, 0, sizeof(double) * nel, rt().stream));
    ProfScope ps("mixmat_bin_table");
    hipLaunchKernelGGL(k_bin_table, dim3((c.kpad + 255) / 256, c.nbins), dim3(256), 0, rt().stream, c.kpad, c.b_start.as<int>(), c.b_rows.as<int>(),
                       c.b_w.as<double>(), t->T.as<double>(), t->Tb.as<double>());
    HX_HIP(hipGetLastError());
    t->have_b = true;
    return HX_OK;
}

// shares of the numerators of product (a, b) for the current mask into c.part[slot]
static int mix_ctx_binned_product(MixCtx &c, int a, int b, int slot)
{
    MixTable *t = nullptr;
    HX_TRY(mix_ctx_binned_table(c, a, b, &t));
    hipStream_t st = rt().stream;
    const size_t nel = (size_t)c.nbpad * c.kpad;
    HX_TRY(c.Tbs.alloc(sizeof(double) * nel));
    HX_TRY(c.part[slot].alloc(sizeof(double) * (size_t)c.ksplit * c.nbpad * c.l2pad));
    ProfScope ps("mixmat_binned");
    HX_TRY(launch_scale_table(256, nel, c.kpad, t->Tb.as<double>(), c.s.as<double>(), c.Tbs.as<double>()));
    const int mt = std::min(c.nbpad / 16, 4);
    const dim3 grid(c.l2pad / 64, c.ksplit, c.nbpad / (16 * mt));
    if (mt == 1)
        hipLaunchKernelGGL(k_binned_gemm<1>, grid, dim3(256), 0, st, c.Tbs.as<double>(), t->T.as<double>(), c.kpad, c.kchunk, c.nbpad, c.l2pad, c.part[slot].as<double>());
    else if (mt == 2)
        hipLaunchKernelGGL(k_binned_gemm<2>, grid, dim3(256), 0, st, c.Tbs.as<double>(), t->T.as<double>(), c.kpad, c.kchunk, c.nbpad, c.l2pad, c.part[slot].as<double>());
    else
        hipLaunchKernelGGL(k_binned_gemm<4>, grid, dim3(256), 0, st, c.Tbs.as<double>(), t->T.as<double>(), c.kpad, c.kchunk, c.nbpad, c.l2pad, c.part[slot].as<double>());
    HX_HIP(hipGetLastError());
    return HX_OK;
}
}  // namespace hx

// spins as hx_mixctx_apply_spin; out (nbins, l2max + 1) or (3, nbins, l2max + 1), host or device: the rows of the matrices binned as
// heracles.result.binned does along axis -2 (weighted mean per bin; exactly 0 where the weighted sum is exactly 0).
extern "C" int hx_mixctx_apply_binned_spin(hx_mixctx *x, const double *cl, int ncl, int s1, int s2, double *out)
{
    HX_TRY(ensure_ready());
    if (!x || !cl || !out || ncl < 1) return fail(HX_ERR_ARG, "hx_mixctx_apply_binned_spin: bad argument");
    bool eb = false;
    HX_TRY(mix_spins("hx_mixctx_apply_binned_spin", s1, s2, eb));
    MixCtx &c = x->c;
    if (c.nbins < 1) return fail(HX_ERR_ARG, "hx_mixctx_apply_binned_spin: no bins set (hx_mixctx_set_bins)");
    const int n2 = c.l2max + 1;
    const size_t sz = (size_t)c.nbins * n2;
    HX_TRY(mix_set_mask(c, cl, ncl));
    const size_t bytes = sizeof(double) * sz * (eb ? 3 : 1);
    const bool to_host = !is_device_ptr(out);
    if (to_host) HX_TRY(c.b_out.alloc(bytes));
    double *d_out = to_host ? c.b_out.as<double>() : out;
    hipStream_t st = rt().stream;
    const dim3 grid((n2 + 255) / 256, c.nbins);
    if (eb) {
        HX_TRY(mix_ctx_binned_product(c, s1, s2, 0));
        HX_TRY(mix_ctx_binned_product(c, s1, -s2, 1));
        hipLaunchKernelGGL(k_binned_finish<true>, grid, dim3(256), 0, st, c.nbins, n2, c.nbpad, c.l2pad, c.ksplit, c.part[0].as<double>(), c.part[1].as<double>(),
                           c.d_cs.as<double>(), c.b_norm.as<double>(), d_out);
    } else {
        HX_TRY(mix_ctx_binned_product(c, s1, 0, 0));
        hipLaunchKernelGGL(k_binned_finish<false>, grid, dim3(256), 0, st, c.nbins, n2, c.nbpad, c.l2pad, c.ksplit, c.part[0].as<double>(), (const double *)nullptr,
                           c.d_cs.as<double>(), c.b_norm.as<double>(), d_out);
    }
    HX_HIP(hipGetLastError());
    if (to_host) {  // (complete on return)
        if (is_pinned_host(out)) {
            HX_TRY(copy_d2h(out, d_out, bytes));
        } else {
            if (c.b_pin_bytes < bytes) {
                if (c.b_pin) (void)hipHostFree(c.b_pin);
                c.b_pin = nullptr;
                c.b_pin_bytes = 0;
                HX_HIP(hipHostMalloc(&c.b_pin, bytes, hipHostMallocDefault));
                c.b_pin_bytes = bytes;
            }
            HX_HIP(hipMemcpyAsync(c.b_pin, d_out, bytes, hipMemcpyDeviceToHost, st));
            HX_HIP(hipStreamSynchronize(st));
            memcpy(out, c.b_pin, bytes);
        }
    }
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}

// kind as hx_mixctx_apply
extern "C" int hx_mixctx_apply_binned(hx_mixctx *x, const double *cl, int ncl, int kind, double *out)
{
    int s1, s2;
    if (!mix_kind_spins(kind, s1, s2)) return fail(HX_ERR_ARG, "hx_mixctx_apply_binned: bad argument");
    return hx_mixctx_apply_binned_spin(x, cl, ncl, s1, s2, out);
}
