// hx_gemm.h -- the FP64 matrix-unit products G = T diag(s) T2^T over zero-padded tables (hx_gemm.hip): rows padded to multiples of
// GB, the contracted dimension (kpad) to a multiple of GK.  Users: the mixing matrices (hx_mixmat.hip) and hx_pinv (hx_svd.hip).
#pragma once
#include "hx_common.h"

namespace hx {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int GB = 128;   // block tile edge (l, l')
constexpr int GK = 32;    // nodes per k tile

// G (n1 x n2, leading dimension ldg) = T diag(s) T2^T for two zero-padded tables T [rows1_pad][kpad], T2 [rows2_pad][kpad], on the
// stream of the library; complete on return (hx_svd.hip)
int launch_gemm_tst(const double *T, int rows1_pad, const double *T2, int rows2_pad, int kpad, const double *s, int n1, int n2, double *G, long long ldg);

// Ts[r][k] = T[r][k] s[k] for nel = rows x kpad elements, with `blocks` work-groups
int launch_scale_table(int blocks, size_t nel, int kpad, const double *T, const double *s, double *Ts);

// The symmetric product G[i][j] = colscale[j] sum_k T[i][k] s[k] T[j][k] (n1 x n2, leading dimension ldg) of one table T [rows_pad][kpad]
// over the block tiles (bi <= bj) of `tiles` (device; (-1, -1) = padding entry, see hx_mix_tiles.h); both halves are written.  Ts: room
// for rows_pad x kpad doubles.  Queued on the stream of the library.
int launch_gemm_sym(const double *T, int rows_pad, int kpad, const double *s, double *Ts, const int2 *tiles, size_t ntiles, int n1, int n2,
                    const double *colscale, double *G, long long ldg);

}  // namespace hx
