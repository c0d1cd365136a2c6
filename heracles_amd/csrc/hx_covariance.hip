// hx_covariance.hip -- the covariance estimators of DICES (heracles/dices/jackknife.py:449-593, heracles/dices/shrinkage.py:66-98)
// as FP64 products over the short sample axis.  gfx950 only.
//
// The samples are stacked as X (n x N, one row per sample, in data-vector order).  Every estimator starts from the centred
// columns D = X - mean (k_cov_center; rows padded with zeros to a multiple of 4, which add nothing to any product) and is then
//   * a Gram matrix alpha D^T D, or alpha Dx^T Dy (k_cov_gram: jackknife_covariance, sample_covariance), batched over column slabs
//     for the per-l products of the delete-2 correction (whose ensemble k_cov_delete2_q forms and permutes l-major in one pass);
//   * the two sums of the optimal shrinkage factor (k_shrink_sums + k_shrink_finish), from G1 = D^T D, G22 = (D.D)^T (D.D),
//     G31 = (D.D.D)^T D and G13 = G31^T, accumulated tile by tile and reduced in the epilogue: neither the W ensemble of the
//     reference (Njk x N x N) nor any N x N matrix but the caller's target is formed.
// Output tiles are 64 x 64 per work-group, 32 x 32 per wave (2 x 2 blocks of v_mfma_f64_16x16x4_f64).  The sample axis is short
// (K = n <= a few thousand) and the operands of a product (n x N doubles: 15 MB at N = 14725, n = 128) stay in L2 / MALL, so a lane
// brings its operand straight from memory, one double per block and K step of 4 -- rows of 16 lanes read 128 contiguous bytes --
// without LDS staging; LDS only transposes the mirrored triangle on the way out and the target's (J, I) tile on the way in.
// Reductions are in a fixed order (no atomics): every result is bitwise repeatable.
#include "hx_common.h"

namespace hx {
namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int CT = 64;  // output tile of a work-group

// D[k][j] = X[k][j] - mean_j (k < n), 0 (n <= k < npad);  ss[j] = sum_k D[k][j]^2 (the diagonal of D^T D).
// Work-group: 32 columns x 8 row groups; the mean in two passes (sum, then the sum of the residuals), the partial sums of the row
// groups added in a fixed order.  In place (D == X) is allowed: pass 3 reads and writes each element from the same thread.
__global__ __launch_bounds__(256) void k_cov_center(int n, int npad, int ncol, const double *X, long long ldx, double *D, long long ldd,
                                                   double *__restrict__ ss)
{
    __shared__ double red[8][33];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int j = blockIdx.x * 32 + c;
    const bool ok = j < ncol;
    auto total = [&](double s) {
        red[g][c] = s;
        __syncthreads();
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += red[q][c];
        __syncthreads();
        return t;
    };
    double s = 0.0;
    if (ok)
        for (int k = g; k < n; k += 8) s += X[(long long)k * ldx + j];
    const double m0 = total(s) / n;
    s = 0.0;
    if (ok)
        for (int k = g; k < n; k += 8) s += X[(long long)k * ldx + j] - m0;
    const double mean = m0 + total(s) / n;
    s = 0.0;
    if (ok)
        for (int k = g; k < npad; k += 8) {
            const double d = k < n ? X[(long long)k * ldx + j] - mean : 0.0;
            D[(long long)k * ldd + j] = d;
            s += d * d;
        }
    s = total(s);
    if (ok && g == 0) ss[j] = s;
}

// The delete-2 ensemble of jackknife.py:542-552, column p of Q taken from data-vector column perm[p]:
//   Q[k][p] = Njk c0 - (Njk - 1) c1[a_k] - (Njk - 1) c1[b_k] + (Njk - 2) c2[k]   (in the reference's order of operations)
__global__ __launch_bounds__(256) void k_cov_delete2_q(int m, int N, double njk, const double *__restrict__ c0, const double *__restrict__ c1,
                                                       const double *__restrict__ c2, const int2 *__restrict__ pairs, const int *__restrict__ perm,
                                                       double *__restrict__ Q)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const int s = perm ? perm[p] : p;
    for (int k = blockIdx.y; k < m; k += gridDim.y) {
        const int2 ab = pairs[k];
        double q = njk * c0[s];
        q -= (njk - 1.0) * c1[(long long)ab.x * N + s];
        q -= (njk - 1.0) * c1[(long long)ab.y * N + s];
        q += (njk - 2.0) * c2[(long long)k * N + s];
        Q[(long long)k * N + p] = q;
    }
}

// One product of a batch: C[coff + i ldc + j] = alpha sum_k X[k][xoff + i] Y[k][yoff + j], i < n1, j < n2.
struct GramBatch {
    int xoff, yoff, n1, n2;
    long long coff, ldc;
};

// Lane l of a wave holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] of each 16 x 16 x 4 step; D: col = l & 15,
// row = (l >> 4) + 4 reg.  Tiles {batch, I, J}; SYM: X == Y and only I <= J is listed, the (J, I) tile is written as the
// transpose of the (I, J) tile (through LDS, so that both stores are row-contiguous).
template <bool SYM>
__global__ __launch_bounds__(256) void k_cov_gram(const double *__restrict__ X, const double *__restrict__ Y, long long ld, int kpad,
                                                  const GramBatch *__restrict__ batches, const int4 *__restrict__ tiles, double alpha,
                                                  double *__restrict__ C)
{
    __shared__ double sm[CT][CT + 1];
    const int4 tl = tiles[blockIdx.x];
    const GramBatch bt = batches[tl.x];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int i0 = tl.y * CT + (w >> 1) * 32, j0 = tl.z * CT + (w & 1) * 32;
    const double *px = X + bt.xoff, *py = Y + bt.yoff;
    const bool ma0 = i0 + r < bt.n1, ma1 = i0 + 16 + r < bt.n1, mb0 = j0 + r < bt.n2, mb1 = j0 + 16 + r < bt.n2;
    double4_t acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (double4_t){0.0, 0.0, 0.0, 0.0};
    for (int k = kq; k < kpad; k += 4) {
        const long long row = (long long)k * ld;
        const double a0 = ma0 ? px[row + i0 + r] : 0.0, a1 = ma1 ? px[row + i0 + 16 + r] : 0.0;
        const double b0 = mb0 ? py[row + j0 + r] : 0.0, b1 = mb1 ? py[row + j0 + 16 + r] : 0.0;
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    const bool mirror = SYM && tl.y != tl.z;
    double *pc = C + bt.coff;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int li = (w >> 1) * 32 + 16 * x + kq + 4 * q, lj = (w & 1) * 32 + 16 * y + r;
                const int gi = tl.y * CT + li, gj = tl.z * CT + lj;
                const double v = alpha * acc[x][y][q];
                if (gi < bt.n1 && gj < bt.n2) pc[(long long)gi * bt.ldc + gj] = v;
                if (mirror) sm[li][lj] = v;
            }
    if (mirror) {
        __syncthreads();
        const int cc = t & 63;
#pragma unroll
        for (int u = 0; u < CT / 4; ++u) {
            const int rr = 4 * u + (t >> 6), gr = tl.z * CT + rr, gc = tl.y * CT + cc;
            if (gr < bt.n2 && gc < bt.n1) pc[(long long)gr * bt.ldc + gc] = sm[cc][rr];
        }
    }
}

// Partial sums of the shrinkage factor over one tile (I <= J) of the (i, j) plane, i != j, i, j < N (the double loop of
// shrinkage.py:88-96 with the W ensemble contracted; the notation of DESIGN.md section 4.7 "Covariance"):
//   Wb = c / n G1,  S = c / (n - 1) G1,  c = (n - 1)^2 / n,  f = n / (n - 1)^3
//   covW(ij,ij) = f (c^2 G22 - n Wb_ij^2),  covW(ii,ij) = f (c^2 G31 - n Wb_ii Wb_ij),  covW(jj,ij) = f (c^2 G13 - n Wb_jj Wb_ij)
//   t_ij = T_ij rs_i rs_j,  rs = 1 / sqrt(diag T)
//   num += covW(ij,ij) - t_ij (sqrt(Wb_jj / Wb_ii) covW(ii,ij) + sqrt(Wb_ii / Wb_jj) covW(jj,ij)) / 2
//   den += (S_ij - t_ij sqrt(S_ii S_jj))^2
// Every factor but t is symmetric in (i, j): an off-diagonal tile adds the (j, i) terms with t_ji, read as the transpose of the
// target's (J, I) tile (staged in LDS).  One (num, den) per tile.
__global__ __launch_bounds__(256, 2) void k_shrink_sums(const double *__restrict__ D, long long ld, int kpad, int N, const int2 *__restrict__ tiles,
                                                     const double *__restrict__ ss, const double *__restrict__ T, long long ldt,
                                                     const double *__restrict__ rs, double n, double c, double f, double2 *__restrict__ part)
{
    __shared__ double tt[CT][CT + 1];
    __shared__ double2 red[4];
    const int2 tl = tiles[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const bool off = tl.x != tl.y;
    if (off) {  // tt[rr][cc] = T[J0 + rr][I0 + cc]
        const int cc = t & 63, gc = tl.x * CT + cc;
#pragma unroll
        for (int u = 0; u < CT / 4; ++u) {
            const int rr = 4 * u + (t >> 6), gr = tl.y * CT + rr;
            tt[rr][cc] = (gr < N && gc < N) ? T[(long long)gr * ldt + gc] : 0.0;
        }
    }
    const int i0 = tl.x * CT + (w >> 1) * 32, j0 = tl.y * CT + (w & 1) * 32;
    const bool ma0 = i0 + r < N, ma1 = i0 + 16 + r < N, mb0 = j0 + r < N, mb1 = j0 + 16 + r < N;
    double4_t g1[2][2], g22[2][2], g31[2][2], g13[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) g1[x][y] = g22[x][y] = g31[x][y] = g13[x][y] = (double4_t){0.0, 0.0, 0.0, 0.0};
    // the operands of step k + 4 are requested before the matrix instructions of step k
    double na[2], nb[2];
    auto fetch = [&](int k) __attribute__((always_inline)) {
        const long long row = (long long)k * ld;
        na[0] = ma0 ? D[row + i0 + r] : 0.0;
        na[1] = ma1 ? D[row + i0 + 16 + r] : 0.0;
        nb[0] = mb0 ? D[row + j0 + r] : 0.0;
        nb[1] = mb1 ? D[row + j0 + 16 + r] : 0.0;
    };
    fetch(kq);
    for (int k = kq; k < kpad; k += 4) {
        const double a[2] = {na[0], na[1]}, b[2] = {nb[0], nb[1]};
        if (k + 4 < kpad) fetch(k + 4);
        const double a2[2] = {a[0] * a[0], a[1] * a[1]}, b2[2] = {b[0] * b[0], b[1] * b[1]};
        const double a3[2] = {a2[0] * a[0], a2[1] * a[1]}, b3[2] = {b2[0] * b[0], b2[1] * b[1]};
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                g1[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], g1[x][y], 0, 0, 0);
                g22[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[x], b2[y], g22[x][y], 0, 0, 0);
                g31[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a3[x], b[y], g31[x][y], 0, 0, 0);
                g13[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b3[y], g13[x][y], 0, 0, 0);
            }
    }
    if (off) __syncthreads();  // tt complete
    const double cn = c / n, cs = c / (n - 1.0), c2 = c * c;
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int li = (w >> 1) * 32 + 16 * x + kq + 4 * q, lj = (w & 1) * 32 + 16 * y + r;
                const int i = tl.x * CT + li, j = tl.y * CT + lj;
                if (i < N && j < N && i != j) {
                    const double G1 = g1[x][y][q];
                    const double wii = cn * ss[i], wjj = cn * ss[j], wij = cn * G1;
                    const double cw = f * (c2 * g22[x][y][q] - n * wij * wij);
                    const double ci = f * (c2 * g31[x][y][q] - n * wii * wij);
                    const double cj = f * (c2 * g13[x][y][q] - n * wjj * wij);
                    const double fij = 0.5 * sqrt(wjj / wii) * ci + 0.5 * sqrt(wii / wjj) * cj;
                    const double sij = cs * G1, sd = sqrt((cs * ss[i]) * (cs * ss[j]));
                    const double rr = rs[i] * rs[j];
                    const double t1 = T[(long long)i * ldt + j] * rr;
                    num += cw - t1 * fij;
                    den += (sij - t1 * sd) * (sij - t1 * sd);
                    if (off) {
                        const double t2 = tt[lj][li] * rr;
                        num += cw - t2 * fij;
                        den += (sij - t2 * sd) * (sij - t2 * sd);
                    }
                }
            }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        num += __shfl_xor(num, o);
        den += __shfl_xor(den, o);
    }
    if (lane == 0) red[w] = make_double2(num, den);
    __syncthreads();
    if (t == 0) {
        double2 s = red[0];
        for (int v = 1; v < 4; ++v) s.x += red[v].x, s.y += red[v].y;
        part[blockIdx.x] = s;
    }
}

// out = (sum num, sum den) over the tiles, in a fixed order.  One work-group.
__global__ __launch_bounds__(256) void k_shrink_finish(int ntiles, const double2 *__restrict__ part, double *__restrict__ out)
{
    __shared__ double2 red[256];
    const int t = threadIdx.x;
    double2 s = make_double2(0.0, 0.0);
    for (int q = t; q < ntiles; q += 256) s.x += part[q].x, s.y += part[q].y;
    red[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) red[t].x += red[t + h].x, red[t].y += red[t + h].y;
        __syncthreads();
    }
    if (t == 0) out[0] = red[0].x, out[1] = red[0].y;
}

// rs[i] = 1 / sqrt(T[i][i])
__global__ __launch_bounds__(256) void k_rsqrt_diag(int N, const double *__restrict__ T, long long ldt, double *__restrict__ rs)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) rs[i] = 1.0 / sqrt(T[(long long)i * ldt + i]);
}

int padded_rows(int n) { return (n + 3) & ~3; }

int center(int n, int ncol, const double *X, long long ldx, double *D, double *ss)
{
    ProfScope ps("cov_center");
    hipLaunchKernelGGL(k_cov_center, dim3((ncol + 31) / 32), dim3(256), 0, rt().stream, n, padded_rows(n), ncol, X, (long long)ldx, D,
                       (long long)ncol, ss);
    HX_HIP(hipGetLastError());
    return HX_OK;
}

int tiles_of(int n) { return (n + CT - 1) / CT; }

// the batched Gram products; sym: X == Y, every batch square
int gram(bool sym, const double *X, const double *Y, long long ld, int kpad, const std::vector<GramBatch> &batches, double alpha, double *C)
{
    std::vector<int4> tiles;
    for (int b = 0; b < (int)batches.size(); ++b) {
        const int ti = tiles_of(batches[b].n1), tj = tiles_of(batches[b].n2);
        for (int I = 0; I < ti; ++I)
            for (int J = sym ? I : 0; J < tj; ++J) tiles.push_back(make_int4(b, I, J, 0));
    }
    if (tiles.empty()) return HX_OK;
    DevBuf db, dt;
    HX_TRY(db.alloc(sizeof(GramBatch) * batches.size()));
    HX_TRY(dt.alloc(sizeof(int4) * tiles.size()));
    HX_TRY(copy_h2d(db.p, batches.data(), sizeof(GramBatch) * batches.size()));
    HX_TRY(copy_h2d(dt.p, tiles.data(), sizeof(int4) * tiles.size()));
    {
        ProfScope ps("cov_gram");
        if (sym)
            hipLaunchKernelGGL(k_cov_gram<true>, dim3((unsigned)tiles.size()), dim3(256), 0, rt().stream, X, X, ld, kpad, db.as<GramBatch>(),
                               dt.as<int4>(), alpha, C);
        else
            hipLaunchKernelGGL(k_cov_gram<false>, dim3((unsigned)tiles.size()), dim3(256), 0, rt().stream, X, Y, ld, kpad, db.as<GramBatch>(),
                               dt.as<int4>(), alpha, C);
        HX_HIP(hipGetLastError());
    }
    HX_HIP(hipStreamSynchronize(rt().stream));  // (the descriptor buffers are released on return)
    return HX_OK;
}

}  // namespace
}  // namespace hx

extern "C" int hx_cov_gram(int n, int n1, int n2, const double *x, const double *y, double alpha, double *out)
{
    using namespace hx;
    HX_TRY(ensure_ready());
    if (n < 1 || n1 < 0 || (y && n2 < 0) || !x || !out) return fail(HX_ERR_ARG, "hx_cov_gram: bad arguments");
    if (!y) n2 = n1;
    if (n1 == 0 || n2 == 0) return HX_OK;
    const int npad = padded_rows(n);
    InView vx, vy;
    OutView vo;
    HX_TRY(vx.bind(x, sizeof(double) * n * (size_t)n1));
    if (y) HX_TRY(vy.bind(y, sizeof(double) * n * (size_t)n2));
    HX_TRY(vo.bind(out, sizeof(double) * (size_t)n1 * n2));
    // one buffer for both centred operands, one leading dimension: Dy follows Dx column-wise (columns [n1, n1 + n2))
    const int ncol = y ? n1 + n2 : n1;
    DevBuf d, ss;
    HX_TRY(d.alloc(sizeof(double) * npad * (size_t)ncol));
    HX_TRY(ss.alloc(sizeof(double) * ncol));
    if (!y) {
        HX_TRY(center(n, n1, vx.as<double>(), n1, d.as<double>(), ss.as<double>()));
        HX_TRY(gram(true, d.as<double>(), d.as<double>(), n1, npad, {GramBatch{0, 0, n1, n1, 0, n1}}, alpha, vo.as<double>()));
    } else {
        // X and Y are centred into the same buffer side by side ([k][0, n1) and [k][n1, n1 + n2)): two launches with ldd = ncol
        ProfScope ps("cov_center");
        hipLaunchKernelGGL(k_cov_center, dim3((n1 + 31) / 32), dim3(256), 0, rt().stream, n, npad, n1, vx.as<double>(), (long long)n1,
                           d.as<double>(), (long long)ncol, ss.as<double>());
        hipLaunchKernelGGL(k_cov_center, dim3((n2 + 31) / 32), dim3(256), 0, rt().stream, n, npad, n2, vy.as<double>(), (long long)n2,
                           d.as<double>() + n1, (long long)ncol, ss.as<double>() + n1);
        HX_HIP(hipGetLastError());
        HX_TRY(gram(false, d.as<double>(), d.as<double>(), ncol, npad, {GramBatch{0, n1, n1, n2, 0, n2}}, alpha, vo.as<double>()));
    }
    HX_TRY(vo.finish());
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}

extern "C" int hx_cov_delete2(int njk, int m, int N, const double *c0, const double *c1, const double *c2, const int *pairs, const int *perm,
                              int nb, const int *bstart, double alpha, double *out)
{
    using namespace hx;
    HX_TRY(ensure_ready());
    if (njk < 2 || m < 1 || N < 0 || nb < 0 || !c0 || !c1 || !c2 || !pairs || !bstart || !out)
        return fail(HX_ERR_ARG, "hx_cov_delete2: bad arguments");
    if (N == 0 || nb == 0) return HX_OK;
    std::vector<int> hb(nb + 1);
    if (is_device_ptr(bstart)) HX_HIP(hipMemcpy(hb.data(), bstart, sizeof(int) * (nb + 1), hipMemcpyDeviceToHost));
    else std::memcpy(hb.data(), bstart, sizeof(int) * (nb + 1));
    std::vector<GramBatch> batches;
    long long total = 0;
    for (int b = 0; b < nb; ++b) {
        const int w = hb[b + 1] - hb[b];
        if (hb[b] < 0 || w < 0 || hb[b + 1] > N) return fail(HX_ERR_ARG, "hx_cov_delete2: batch %d out of range", b);
        batches.push_back(GramBatch{hb[b], hb[b], w, w, total, w});
        total += (long long)w * w;
    }
    const int npad = padded_rows(m);
    InView v0, v1, v2, vp, vm;
    OutView vo;
    HX_TRY(v0.bind(c0, sizeof(double) * N));
    HX_TRY(v1.bind(c1, sizeof(double) * njk * (size_t)N));
    HX_TRY(v2.bind(c2, sizeof(double) * m * (size_t)N));
    HX_TRY(vp.bind(pairs, sizeof(int) * 2 * (size_t)m));
    if (perm) HX_TRY(vm.bind(perm, sizeof(int) * (size_t)N));
    HX_TRY(vo.bind(out, sizeof(double) * (size_t)std::max(total, 1LL)));
    DevBuf q, ss;
    HX_TRY(q.alloc(sizeof(double) * npad * (size_t)N));
    HX_TRY(ss.alloc(sizeof(double) * N));
    {
        ProfScope ps("cov_delete2_q");
        hipLaunchKernelGGL(k_cov_delete2_q, dim3((N + 255) / 256, std::min(m, 65535)), dim3(256), 0, rt().stream, m, N, (double)njk,
                           v0.as<double>(), v1.as<double>(), v2.as<double>(), vp.as<int2>(), perm ? vm.as<int>() : nullptr, q.as<double>());
        HX_HIP(hipGetLastError());
    }
    HX_TRY(center(m, N, q.as<double>(), N, q.as<double>(), ss.as<double>()));
    HX_TRY(gram(true, q.as<double>(), q.as<double>(), N, npad, batches, alpha, vo.as<double>()));
    HX_TRY(vo.finish());
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}

extern "C" int hx_cov_shrink_sums(int n, int N, const double *x, const double *target, int64_t ldt, double *out)
{
    using namespace hx;
    HX_TRY(ensure_ready());
    if (n < 2 || N < 0 || ldt < N || !x || !target || !out) return fail(HX_ERR_ARG, "hx_cov_shrink_sums: bad arguments");
    if (N == 0) {
        const double z[2] = {0.0, 0.0};
        OutView vo;
        HX_TRY(vo.bind(out, sizeof(z)));
        HX_HIP(hipMemcpyAsync(vo.dev, z, sizeof(z), hipMemcpyHostToDevice, rt().stream));
        HX_TRY(vo.finish());
        HX_HIP(hipStreamSynchronize(rt().stream));
        return HX_OK;
    }
    const int npad = padded_rows(n);
    InView vx, vt;
    OutView vo;
    HX_TRY(vx.bind(x, sizeof(double) * n * (size_t)N));
    HX_TRY(vt.bind(target, sizeof(double) * ((size_t)(N - 1) * ldt + N)));
    HX_TRY(vo.bind(out, 2 * sizeof(double)));
    std::vector<int2> tiles;
    const int nt = tiles_of(N);
    for (int I = 0; I < nt; ++I)
        for (int J = I; J < nt; ++J) tiles.push_back(make_int2(I, J));
    DevBuf d, ss, rs, dt, part;
    HX_TRY(d.alloc(sizeof(double) * npad * (size_t)N));
    HX_TRY(ss.alloc(sizeof(double) * N));
    HX_TRY(rs.alloc(sizeof(double) * N));
    HX_TRY(dt.alloc(sizeof(int2) * tiles.size()));
    HX_TRY(part.alloc(sizeof(double2) * tiles.size()));
    HX_TRY(copy_h2d(dt.p, tiles.data(), sizeof(int2) * tiles.size()));
    HX_TRY(center(n, N, vx.as<double>(), N, d.as<double>(), ss.as<double>()));
    const double dn = n, c = (dn - 1.0) * (dn - 1.0) / dn, f = dn / ((dn - 1.0) * (dn - 1.0) * (dn - 1.0));
    {
        ProfScope ps("cov_shrink_sums");
        hipLaunchKernelGGL(k_rsqrt_diag, dim3((N + 255) / 256), dim3(256), 0, rt().stream, N, vt.as<double>(), (long long)ldt, rs.as<double>());
        hipLaunchKernelGGL(k_shrink_sums, dim3((unsigned)tiles.size()), dim3(256), 0, rt().stream, d.as<double>(), (long long)N, npad, N,
                           dt.as<int2>(), ss.as<double>(), vt.as<double>(), (long long)ldt, rs.as<double>(), dn, c, f, part.as<double2>());
        hipLaunchKernelGGL(k_shrink_finish, dim3(1), dim3(256), 0, rt().stream, (int)tiles.size(), part.as<double2>(), vo.as<double>());
        HX_HIP(hipGetLastError());
    }
    HX_TRY(vo.finish());
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}
