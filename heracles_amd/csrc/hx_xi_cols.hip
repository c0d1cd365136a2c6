// hx_xi_cols.hip -- Cl <-> xi(theta) for batches of single columns as FP64 GEMMs against the cached Wigner tables, and the
// element-wise ratio xi_d / damped xi_mask of NaturalSpice between them.  gfx950 only.
//
// A column is one 1-D sequence tied to one table family f (0: P_l, 1: d^l_22, 2: d^l_2-2, 3: d^l_20; the order of k_corr_tables).
// These are the columns of hx_cl2corr / hx_corr2cl (TT; EE + BB; EE - BB; TE) taken apart, so that a scalar key costs one column
// instead of four, and so that the table is read once per 64 columns instead of once per spectrum:
//   forward  xi[c][k] = sum_{l0 <= l < nl} ((2l + 1) / 4 pi  a[c][l]) T_f[l][k]        (k_xi_fwd: contracts over the table's rows)
//   back     b[c][l]  = 2 pi sum_k (w_k xi[c][k]) T_f[l][k],  l0 <= l < nl             (k_xi_back: over its contiguous axis)
// with l0 = 0 for P_l and 2 for the others.  Tiles are 64 x 64 per work-group and 32 x 32 per wave (2 x 2 blocks of
// v_mfma_f64_16x16x4_f64), operands straight from memory as in k_cov_gram: the column operand of a launch (ncol x nl doubles) stays
// in L2 / MALL; of the table a row of 16 lanes reads 128 contiguous bytes (forward) or four lanes read one 128-byte line of a row
// in 128-bit pieces (back).  The columns of one family are gathered through an index list, one launch per family.
//
// Determinism: an output element is the accumulator of one lane, fed by the same sequence of matrix instructions over l (or k)
// whatever else is in the batch: rows of A do not mix in the instruction, a column's slot in its tile only chooses the lane, and a
// tile that is partly empty feeds zeros to other rows.  No split of the contraction, no atomics.  A column alone, at any position
// of any batch, in any chunking of a batch, and from run to run gives the same bits.
//
// Nothing is kept between calls but the tables hx_cl2corr already caches (corr_tables_view: one owner, hx_release_caches frees
// them); index lists and factors are temporaries of the call.
//
// Columns of any spin weight (hx_cl2corr_cols_spin / hx_corr2cl_cols_spin, xi_columns_spin below) are tied to a pair (a, b) instead of
// a family: the same kernels against T_{ab}[l][k] = d^l_{ab}(x_k) with l0 = max(|a|, |b|), one launch per distinct pair, tables from
// the pair cache beside the family tables (xi_pair_table_view in hx_transforms.hip: one owner, bounded, freed by hx_release_caches).
#include <algorithm>
#include <vector>

#include "hx_wigner.h"

namespace hx {
namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int XT = 64;  // output tile of a work-group

// f[l] = (2l + 1) / 4 pi, as k_cl2corr forms it
__global__ void k_xi_factors(int nl, double *__restrict__ f)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l < nl) f[l] = (2.0 * l + 1.0) / (4.0 * M_PI);
}

// Lane (r = lane & 15, kq = lane >> 4) holds A[i = r][kk = kq] and B[kk = kq][j = r] of a 16 x 16 x 4 step; D: column r, row kq + 4 reg.
// i: columns of the batch (through cols[]), j: nodes, kk: multipoles.  T: the family's table [lmax + 1][kpad], kpad = ceil64(n).
__global__ __launch_bounds__(256) void k_xi_fwd(int nl, int n, int kpad, int l0, const double *__restrict__ T, const double *__restrict__ f,
                                                const int *__restrict__ cols, int nc, const double *__restrict__ a, double *__restrict__ xi)
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int i0 = blockIdx.y * XT + (w >> 1) * 32, j0 = blockIdx.x * XT + (w & 1) * 32;
    const bool ma0 = i0 + r < nc, ma1 = i0 + 16 + r < nc;
    const double *pa0 = a + (long long)(ma0 ? cols[i0 + r] : 0) * nl;
    const double *pa1 = a + (long long)(ma1 ? cols[i0 + 16 + r] : 0) * nl;
    const double *pb = T + j0 + r;  // (j0 + r + 16 < kpad: the grid covers ceil64(n) = kpad nodes)
    double4_t acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (double4_t){0.0, 0.0, 0.0, 0.0};
    int lb = 0;
    for (; lb + 16 <= nl; lb += 16) {  // four steps with their loads issued together; every multipole is below nl
        double av[2][4], bv[2][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int l = lb + 4 * u + kq;
            const long long row = (long long)l * kpad;
            const double fl = f[l];
            av[0][u] = ma0 && l >= l0 ? fl * pa0[l] : 0.0;
            av[1][u] = ma1 && l >= l0 ? fl * pa1[l] : 0.0;
            bv[0][u] = pb[row];
            bv[1][u] = pb[row + 16];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0][u], bv[0][u], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0][u], bv[1][u], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1][u], bv[0][u], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1][u], bv[1][u], acc[1][1], 0, 0, 0);
        }
    }
    for (; lb < nl; lb += 4) {
        const int l = lb + kq;
        const bool ok = l < nl && l >= l0;
        const double fl = ok ? f[l] : 0.0;
        const double a0 = ok && ma0 ? fl * pa0[l] : 0.0, a1 = ok && ma1 ? fl * pa1[l] : 0.0;
        const long long row = (long long)l * kpad;
        const double b0 = ok ? pb[row] : 0.0, b1 = ok ? pb[row + 16] : 0.0;
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + 16 * x + kq + 4 * q;
            if (i >= nc) continue;
            double *po = xi + (long long)cols[i] * n;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const int j = j0 + 16 * y + r;
                if (j < n) po[j] = acc[x][y][q];
            }
        }
}

// i: columns of the batch, j: multipoles (rows of the table), kk: nodes.  Of a block of 16 nodes lane (r, kq) takes the four nodes
// 4 kq .. 4 kq + 3 of its A row and its B row (the table's as two 128-bit loads) and the h-th instruction of the block contracts
// node 4 kq + h of every kq: both operands use the same assignment, which is all the instruction asks for.
__global__ __launch_bounds__(256) void k_xi_back(int nl, int n, int kpad, int l0, const double *__restrict__ T, const double *__restrict__ wq,
                                                 const int *__restrict__ cols, int nc, const double *__restrict__ xi, double *__restrict__ b)
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int i0 = blockIdx.y * XT + (w >> 1) * 32, j0 = blockIdx.x * XT + (w & 1) * 32;
    const bool ma[2] = {i0 + r < nc, i0 + 16 + r < nc};
    const bool mb[2] = {j0 + r < nl, j0 + 16 + r < nl};
    const double *pa[2], *pb[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        pa[x] = xi + (long long)(ma[x] ? cols[i0 + 16 * x + r] : 0) * n + 4 * kq;
        pb[x] = T + (long long)(mb[x] ? j0 + 16 * x + r : 0) * kpad + 4 * kq;
    }
    const double *pw = wq + 4 * kq;
    double4_t acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (double4_t){0.0, 0.0, 0.0, 0.0};
    for (int kb = 0; kb < n; kb += 16) {
        double av[2][4], bv[2][4];
        if (kb + 16 <= n) {
            const double2 w01 = *reinterpret_cast<const double2 *>(pw + kb), w23 = *reinterpret_cast<const double2 *>(pw + kb + 2);
            const double wk[4] = {w01.x, w01.y, w23.x, w23.y};
#pragma unroll
            for (int x = 0; x < 2; ++x) {
#pragma unroll
                for (int h = 0; h < 4; ++h) av[x][h] = ma[x] ? wk[h] * pa[x][kb + h] : 0.0;  // (rows of xi are n doubles apart: 8-byte loads)
                double2 t01 = make_double2(0.0, 0.0), t23 = t01;
                if (mb[x]) {
                    t01 = *reinterpret_cast<const double2 *>(pb[x] + kb);
                    t23 = *reinterpret_cast<const double2 *>(pb[x] + kb + 2);
                }
                bv[x][0] = t01.x; bv[x][1] = t01.y; bv[x][2] = t23.x; bv[x][3] = t23.y;
            }
        } else {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const bool in = kb + 4 * kq + h < n;
                const double wk = in ? pw[kb + h] : 0.0;
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    av[x][h] = in && ma[x] ? wk * pa[x][kb + h] : 0.0;
                    bv[x][h] = in && mb[x] ? pb[x][kb + h] : 0.0;
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0][h], bv[0][h], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0][h], bv[1][h], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1][h], bv[0][h], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1][h], bv[1][h], acc[1][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + 16 * x + kq + 4 * q;
            if (i >= nc) continue;
            double *po = b + (long long)cols[i] * nl;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const int j = j0 + 16 * y + r;
                if (j < nl) po[j] = j < l0 ? 0.0 : 2.0 * M_PI * acc[x][y][q];
            }
        }
}

// out[c][k] = xi_d[c][k] / D^ndamp[c](alpha),  alpha = xi_num[num_col[c]][k] (/ xi_den[den_col[c]][k] if den_col[c] >= 0),
// D(alpha) = alpha (1 + exp(-kk (log10 |alpha| - x0))): heracles/unmixing.py:95-101 and heracles/dices/jackknife.py:440-470 in plain IEEE
// arithmetic (alpha = 0: nan; a vanishing alpha: an infinite divisor, 0 out), every operation rounded on its own as numpy does.
__global__ __launch_bounds__(256) void k_xi_ratio(int n, long long total, const double *xi_d, const double *__restrict__ xi_num,
                                                  const int *__restrict__ num_col, const double *__restrict__ xi_den,
                                                  const int *__restrict__ den_col, const int *__restrict__ ndamp, double x0, double kk,
                                                  double *out)  // (out may be xi_d: an element is read and written by one thread)
{
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long c = e / n;
    const int k = (int)(e - c * n);
    double alpha = xi_num[(long long)num_col[c] * n + k];
    const int dc = den_col ? den_col[c] : -1;
    if (dc >= 0) alpha = alpha / xi_den[(long long)dc * n + k];
    for (int d = ndamp[c]; d > 0; --d) alpha = alpha * (1.0 + exp(-kk * (log10(fabs(alpha)) - x0)));
    out[e] = xi_d[e] / alpha;
}

// columns of each family, in batch order
struct FamilyLists {
    std::vector<int> idx;
    int off[5] = {0, 0, 0, 0, 0};
};

bool family_lists(int ncol, const int *family, FamilyLists &fl)
{
    int cnt[4] = {0, 0, 0, 0};
    for (int c = 0; c < ncol; ++c) {
        if (family[c] < 0 || family[c] > 3) return false;
        ++cnt[family[c]];
    }
    for (int f = 0; f < 4; ++f) fl.off[f + 1] = fl.off[f] + cnt[f];
    fl.idx.resize(ncol);
    int at[4] = {fl.off[0], fl.off[1], fl.off[2], fl.off[3]};
    for (int c = 0; c < ncol; ++c) fl.idx[at[family[c]]++] = c;
    return true;
}

int xi_columns(bool fwd, int lmax, int nl, int ncol, const int *family, const double *src, double *dst)
{
    const char *name = fwd ? "hx_cl2corr_cols" : "hx_corr2cl_cols";
    HX_TRY(ensure_ready());
    if (lmax < 0 || nl < 1 || nl > lmax + 1 || ncol < 1 || !family || !src || !dst) return fail(HX_ERR_ARG, "%s: bad argument", name);
    FamilyLists fl;
    if (!family_lists(ncol, family, fl)) return fail(HX_ERR_ARG, "%s: family outside 0..3", name);
    const int n = lmax + 1;
    const double *T, *w;
    int kpad;
    HX_TRY(corr_tables_view(lmax, &T, &w, &kpad));
    hipStream_t st = rt().stream;
    InView vi;
    OutView vo;
    HX_TRY(vi.bind(src, sizeof(double) * (size_t)ncol * (fwd ? nl : n)));
    HX_TRY(vo.bind(dst, sizeof(double) * (size_t)ncol * (fwd ? n : nl)));
    DevBuf d_idx, d_f;
    HX_TRY(d_idx.alloc(sizeof(int) * (size_t)ncol));
    HX_HIP(hipMemcpyAsync(d_idx.p, fl.idx.data(), sizeof(int) * (size_t)ncol, hipMemcpyHostToDevice, st));
    if (fwd) {
        HX_TRY(d_f.alloc(sizeof(double) * (size_t)nl));
        hipLaunchKernelGGL(k_xi_factors, dim3((nl + 255) / 256), dim3(256), 0, st, nl, d_f.as<double>());
    }
    const long long tstride = (long long)n * kpad;
    {
        ProfScope ps(fwd ? "xi_cols_fwd" : "xi_cols_back");
        for (int f = 0; f < 4; ++f) {
            const int nc = fl.off[f + 1] - fl.off[f], l0 = f ? 2 : 0;
            if (!nc) continue;
            const dim3 grid(((fwd ? n : nl) + XT - 1) / XT, (nc + XT - 1) / XT);
            if (fwd)
                hipLaunchKernelGGL(k_xi_fwd, grid, dim3(256), 0, st, nl, n, kpad, l0, T + f * tstride, d_f.as<double>(), d_idx.as<int>() + fl.off[f],
                                   nc, vi.as<double>(), vo.as<double>());
            else
                hipLaunchKernelGGL(k_xi_back, grid, dim3(256), 0, st, nl, n, kpad, l0, T + f * tstride, w, d_idx.as<int>() + fl.off[f], nc,
                                   vi.as<double>(), vo.as<double>());
        }
    }
    HX_HIP(hipGetLastError());
    HX_TRY(vo.finish());
    HX_HIP(hipStreamSynchronize(st));  // the index list and the factors die with this scope
    return HX_OK;
}

__global__ void k_xi_negate(int n, const double *__restrict__ src, double *__restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = -src[i];
}

// Columns tied to a PAIR (a, b) instead of a family: column c runs on T_{ab}[l][k] = d^l_{ab}(x_k) with l0 = max(|a|, |b|), the same two
// kernels, one launch per distinct pair.  Pairs share the table of their normalised pair (xi_pair_table_view); where the
// normalisation leaves a minus sign (d_{12} = -d_{21}) the launch gets the negated factors (forward) or weights (back): every product
// of the contraction changes its sign and nothing else, so the result is the bits of the shared table's, negated.  The determinism
// statement at the top holds as it stands: a column's accumulator sees its pair's table, factors and weights, whatever else is in the
// batch, and the order of the launches does not enter.
int xi_columns_spin(bool fwd, int lmax, int nl, int ncol, const int *pairs, const double *src, double *dst)
{
    const char *name = fwd ? "hx_cl2corr_cols_spin" : "hx_corr2cl_cols_spin";
    HX_TRY(ensure_ready());
    if (lmax < 0 || nl < 1 || nl > lmax + 1 || ncol < 1 || !pairs || !src || !dst) return fail(HX_ERR_ARG, "%s: bad argument", name);
    // columns by (A, B, sign): the launches of pairs that share a table follow each other
    struct Group {
        int A, B, neg, l0;
        std::vector<int> cols;
    };
    std::vector<Group> groups;
    for (int c = 0; c < ncol; ++c) {
        const int a = pairs[2 * c], b = pairs[2 * c + 1];
        if (std::max(abs(a), abs(b)) > HX_MAX_MIX_SPIN)
            return fail(HX_ERR_UNSUPPORTED, "%s: (a,b)=(%d,%d) beyond the supported max(|a|,|b|) <= %d", name, a, b, HX_MAX_MIX_SPIN);
        int A, B;
        const int neg = wigner_pair_normalise(a, b, &A, &B) < 0.0;
        size_t g = 0;
        while (g < groups.size() && !(groups[g].A == A && groups[g].B == B && groups[g].neg == neg)) ++g;
        if (g == groups.size()) groups.push_back(Group{A, B, neg, A, {}});
        groups[g].cols.push_back(c);
    }
    std::stable_sort(groups.begin(), groups.end(), [](const Group &x, const Group &y) { return x.A != y.A ? x.A < y.A : x.B < y.B; });
    std::vector<int> idx;
    idx.reserve(ncol);
    bool any_neg = false;
    for (const Group &g : groups) {
        idx.insert(idx.end(), g.cols.begin(), g.cols.end());
        any_neg = any_neg || g.neg;
    }
    const int n = lmax + 1;
    hipStream_t st = rt().stream;
    InView vi;
    OutView vo;
    HX_TRY(vi.bind(src, sizeof(double) * (size_t)ncol * (fwd ? nl : n)));
    HX_TRY(vo.bind(dst, sizeof(double) * (size_t)ncol * (fwd ? n : nl)));
    DevBuf d_idx, d_f;  // d_f: factors | negated factors (forward), negated weights (back)
    HX_TRY(d_idx.alloc(sizeof(int) * (size_t)ncol));
    HX_HIP(hipMemcpyAsync(d_idx.p, idx.data(), sizeof(int) * (size_t)ncol, hipMemcpyHostToDevice, st));
    if (fwd) {
        HX_TRY(d_f.alloc(sizeof(double) * (size_t)2 * nl));
        hipLaunchKernelGGL(k_xi_factors, dim3((nl + 255) / 256), dim3(256), 0, st, nl, d_f.as<double>());
        if (any_neg) hipLaunchKernelGGL(k_xi_negate, dim3((nl + 255) / 256), dim3(256), 0, st, nl, d_f.as<double>(), d_f.as<double>() + nl);
    } else if (any_neg) {
        HX_TRY(d_f.alloc(sizeof(double) * (size_t)n));
    }
    bool have_wneg = false;
    {
        ProfScope ps(fwd ? "xi_cols_fwd" : "xi_cols_back");
        int off = 0;
        for (const Group &g : groups) {
            const int nc = (int)g.cols.size();
            const double *T, *w;
            int kpad;
            HX_TRY(xi_pair_table_view(lmax, g.A, g.B, &T, &w, &kpad));  // (the weights stay where they are for the whole call: one lmax)
            const dim3 grid(((fwd ? n : nl) + XT - 1) / XT, (nc + XT - 1) / XT);
            if (fwd) {
                hipLaunchKernelGGL(k_xi_fwd, grid, dim3(256), 0, st, nl, n, kpad, g.l0, T, d_f.as<double>() + (g.neg ? nl : 0), d_idx.as<int>() + off, nc,
                                   vi.as<double>(), vo.as<double>());
            } else {
                if (g.neg && !have_wneg) {
                    hipLaunchKernelGGL(k_xi_negate, dim3((n + 255) / 256), dim3(256), 0, st, n, w, d_f.as<double>());
                    have_wneg = true;
                }
                hipLaunchKernelGGL(k_xi_back, grid, dim3(256), 0, st, nl, n, kpad, g.l0, T, g.neg ? d_f.as<const double>() : w, d_idx.as<int>() + off, nc,
                                   vi.as<double>(), vo.as<double>());
            }
            off += nc;
        }
    }
    HX_HIP(hipGetLastError());
    HX_TRY(vo.finish());
    HX_HIP(hipStreamSynchronize(st));  // the index list, the factors and the negated weights die with this scope
    return HX_OK;
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hx_cl2corr_cols_spin(int lmax, int nl, int ncol, const int *pairs, const double *a, double *xi)
{
    return xi_columns_spin(true, lmax, nl, ncol, pairs, a, xi);
}

extern "C" int hx_corr2cl_cols_spin(int lmax, int nl, int ncol, const int *pairs, const double *xi, double *b)
{
    return xi_columns_spin(false, lmax, nl, ncol, pairs, xi, b);
}


extern "C" int hx_cl2corr_cols(int lmax, int nl, int ncol, const int *family, const double *a, double *xi)
{
    return xi_columns(true, lmax, nl, ncol, family, a, xi);
}

extern "C" int hx_corr2cl_cols(int lmax, int nl, int ncol, const int *family, const double *xi, double *b)
{
    return xi_columns(false, lmax, nl, ncol, family, xi, b);
}

extern "C" int hx_xi_ratio(int n, int ncol, const double *xi_d, const double *xi_num, const int *num_col, const double *xi_den,
                           const int *den_col, const int *ndamp, double x0, double k, double *out)
{
    HX_TRY(ensure_ready());
    if (n < 1 || ncol < 1 || !xi_d || !xi_num || !num_col || !ndamp || !out || (den_col && !xi_den))
        return fail(HX_ERR_ARG, "hx_xi_ratio: bad argument");
    int nnum = 0, nden = 0;
    for (int c = 0; c < ncol; ++c) {
        if (num_col[c] < 0 || ndamp[c] < 0 || (den_col && den_col[c] < -1)) return fail(HX_ERR_ARG, "hx_xi_ratio: index out of range");
        nnum = std::max(nnum, num_col[c] + 1);
        if (den_col) nden = std::max(nden, den_col[c] + 1);
    }
    hipStream_t st = rt().stream;
    const size_t row = sizeof(double) * (size_t)n;
    InView vd, vn, ve;
    OutView vo;
    HX_TRY(vd.bind(xi_d, row * ncol));
    HX_TRY(vn.bind(xi_num, row * nnum));
    if (nden) HX_TRY(ve.bind(xi_den, row * nden));
    HX_TRY(vo.bind(out, row * ncol));
    // num_col | den_col | ndamp in one upload
    std::vector<int> ix((size_t)3 * ncol);
    for (int c = 0; c < ncol; ++c) {
        ix[c] = num_col[c];
        ix[(size_t)ncol + c] = nden ? den_col[c] : -1;
        ix[(size_t)2 * ncol + c] = ndamp[c];
    }
    DevBuf d_ix;
    HX_TRY(d_ix.alloc(sizeof(int) * ix.size()));
    HX_HIP(hipMemcpyAsync(d_ix.p, ix.data(), sizeof(int) * ix.size(), hipMemcpyHostToDevice, st));
    const long long total = (long long)ncol * n;
    {
        ProfScope ps("xi_ratio");
        hipLaunchKernelGGL(k_xi_ratio, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, n, total, vd.as<double>(), vn.as<double>(),
                           d_ix.as<int>(), nden ? ve.as<double>() : (const double *)nullptr, d_ix.as<int>() + ncol, d_ix.as<int>() + 2 * (size_t)ncol, x0, k,
                           vo.as<double>());
    }
    HX_HIP(hipGetLastError());
    HX_TRY(vo.finish());
    HX_HIP(hipStreamSynchronize(st));
    return HX_OK;
}
