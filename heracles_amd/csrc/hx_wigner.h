// hx_wigner.h -- Gauss-Legendre nodes and Wigner-d tables in double-double (hx_wigner.hip), and the two owners of what is kept of
// them between calls: a node holder and a bounded set of tables by pair.  Users: the mixing matrices (hx_mixmat.hip), the Cl <-> xi
// pair tables (hx_transforms.hip, hx_xi_cols.hip) and the polar tables of the point transform (hx_nufft.hip).
#pragma once
#include <memory>
#include <vector>

#include "hx_common.h"

namespace hx {

// Gauss-Legendre nodes/weights into device arrays, on the library stream
int launch_gauss_legendre(int n, double *d_x, double *d_w, double *d_xlo = nullptr);  // d_xlo: node k = x[k] + xlo[k] (see k_gauss_legendre)

// Wigner-d tables of any pair by k_wigner_table_dd:
//   wigner_pair_normalise: (a, b) brought to A >= |B|, A >= 0 by d_{ab} = (-1)^{a-b} d_{ba} = d_{-b,-a} (the pair under which
//     tables are kept and shared); returns the sign s with d_{ab} = s d_{AB};
//   wigner_table_build: out[l * sl + k * sk] = d^l_{ab}(x_k + xlo_k), l = 0 .. lmax (0 below max(|a|, |b|)), device pointers, on the
//     library stream; complete on return.
double wigner_pair_normalise(int a, int b, int *A, int *B);
int wigner_table_build(int lmax, int a, int b, int n, const double *d_x, const double *d_xlo, double *d_out, long long sl, long long sk);

// The n Gauss-Legendre nodes and weights on the device, rebuilt when n changes.  node k = x[k] + xlo[k] where xlo is asked for
// (k_gauss_legendre writes the same x, w with or without it).
struct GLNodes {
    int n = 0;
    DevBuf x, w, xlo;
    int ensure(int n_new, bool want_xlo);
    void release();
};

// One cached table T[l][k] = d^l_{ab}(x_k), row stride kpad, of a normalised pair.  Tb: rows derived from T that must die with it
// (the binned rows of the mixing matrices, hx_mixctx_set_bins; unused elsewhere).
struct WigTable {
    int a = 0, b = 0;
    DevBuf T, Tb;
    bool have = false, have_b = false;
    unsigned long long used = 0;
};
// Tables by normalised pair (A >= |B|): rows x kpad doubles each (zero padded), d^l for l <= lmax, at the nodes of one GLNodes.  At
// most max_tabs are kept; for a new one the table used longest ago is dropped, behind a synchronisation of the library stream
// (launches that read it are done by then).  One pair may be pinned: its table has a size of its own and is never dropped.
struct WigTableSet {
    int lmax = -1, rows = 0, kpad = 0, max_tabs = 0;
    int pin_a = -1, pin_b = 0, pin_lmax = -1, pin_rows = 0;
    WigTable pinned;
    std::vector<std::unique_ptr<WigTable>> tabs;
    unsigned long long tick = 0;
    // the table of (A, B), built on first use; *out stays valid until the next call with a pair that is not in the set
    int get(const GLNodes &gl, int A, int B, WigTable **out);
};

}  // namespace hx
