"""The long-double truth of tests/corr_reference.py against mpmath at 50 digits, against orthogonality, and the oracle's closed forms
(the yardstick of tests/test_gpu_corr_stage.py) against that truth.  The GPU tests measure double-precision errors of 4e-13 (interior
nodes) to 2e-9 (end nodes, lmax 6144) with it, so it has to be good to a few 1e-15; it is (test_longdouble_recursion_rounding)."""

import mpmath
import numpy as np
import pytest

import corr_reference as cr

X_END = 0.9999999234  # about the end node of n = 6145
XS = (-X_END, -0.3, 0.0, 0.9985, X_END)
NAMES = ("P", "d22", "d2m2", "d20")


def _mp_rows(lmax, x):
    return cr.recursion_rows(lmax, mpmath.mpf(x), mpmath.mpf, mpmath.sqrt, mpmath.mpf(0))


def _jacobi(n, a, b, x):
    """P_n^(a,b)(x) = sum_s C(n+a, n-s) C(n+b, s) ((x-1)/2)^s ((x+1)/2)^(n-s) (Szego 4.3.2): the finite sum, which mpmath.jacobi's
    hypergeometric series does not manage where the value is exactly zero (P_1^(2,2)(0)).  Its terms cancel over ~n digits, hence
    the working precision of _closed_forms."""
    u, v = (x - 1) / 2, (x + 1) / 2
    return mpmath.fsum(mpmath.binomial(n + a, n - s) * mpmath.binomial(n + b, s) * u**s * v ** (n - s) for s in range(n + 1))


def _closed_forms(l, x):
    """P_l and the spin-2 functions through Jacobi polynomials (Varshalovich et al. 1988, section 4.3.4, eq. 13), at 400 digits."""
    with mpmath.workdps(400):
        x = mpmath.mpf(x)
        P = mpmath.legendre(l, x) if l < 2 else _jacobi(l, 0, 0, x)
        if l < 2:
            return P, mpmath.mpf(0), mpmath.mpf(0), mpmath.mpf(0)
        d22 = ((1 + x) / 2) ** 2 * _jacobi(l - 2, 0, 4, x)
        d2m2 = ((1 - x) / 2) ** 2 * _jacobi(l - 2, 4, 0, x)
        d20 = mpmath.sqrt(mpmath.factorial(l - 2) * mpmath.factorial(l + 2)) / mpmath.factorial(l) * (1 - x) * (1 + x) / 4 * _jacobi(l - 2, 2, 2, x)
        return P, d22, d2m2, d20


def test_recursion_is_the_closed_forms_in_mpmath():
    """(i) the formulas, signs included: the recursion run in mpmath equals Legendre / Jacobi closed forms to 1e-48 relative to 1."""
    with mpmath.workdps(60):
        for x in XS:
            want = {l: _closed_forms(l, x) for l in (0, 1, 2, 3, 50, 300)}
            for l, rows in enumerate(_mp_rows(300, x)):
                if l in want:
                    for name, a, b in zip(NAMES, rows, want[l]):
                        assert abs(a - b) <= mpmath.mpf(10) ** -48, (name, l, x, mpmath.nstr(a - b, 5))


def test_longdouble_recursion_rounding():
    """(ii) the rounding: the long-double recursion against the same recursion in mpmath for every l <= 6144 at the five x: at most
    8 lmax eps_longdouble = 5.3e-15 (measured when this was written: 3.3e-15 P, 7.9e-16 d22, 8.0e-16 d2m2, 2.2e-15 d20, worst at the
    end nodes: linear growth ~5 l eps)."""
    lmax = 6144
    worst = np.zeros(4)
    with mpmath.workdps(50):
        gens = [_mp_rows(lmax, float(x)) for x in XS]
        for l, rows in enumerate(cr.wigner_rows(lmax, np.array(XS))):
            for j, g in enumerate(gens):
                ref = next(g)
                for ix in range(4):
                    got = mpmath.mpf(float(rows[ix][j])) + mpmath.mpf(float(rows[ix][j] - cr.LD(float(rows[ix][j]))))
                    worst[ix] = max(worst[ix], float(abs(got - ref[ix])))
    print("\nlong-double recursion vs mpmath, lmax 6144, max over l and 5 nodes: " + ", ".join(f"{n} {v:.2e}" for n, v in zip(NAMES, worst)))
    assert worst.max() <= 8 * lmax * cr.EPS_LD, worst


def test_orthogonality_at_300(oracle):
    """Formula-free: sum_k w_k d_l d_l' = 2 / (2l + 1) delta_ll' for each family with the oracle's Gauss-Legendre rule (n = 301
    integrates degree 600 exactly; what is left is the rounding of the double nodes and weights)."""
    lmax = 300
    x, w = oracle.gauss_legendre(lmax + 1)
    T = np.zeros((4, lmax + 1, lmax + 1), dtype=cr.LD)
    for l, rows in enumerate(cr.wigner_rows(lmax, x)):
        for ix in range(4):
            T[ix, l] = rows[ix]
    want = np.diag(2 / (2 * np.arange(lmax + 1).astype(cr.LD) + 1))
    worst = []
    for ix in range(4):
        G = (T[ix] * w.astype(cr.LD)[None, :]) @ T[ix].T
        ref = want.copy()
        if ix:
            ref[:2, :2] = 0
        worst.append(float(np.abs(G - ref).max()))
    print("\northogonality at lmax 300, max |G - 2/(2l+1) delta|: " + ", ".join(f"{n} {v:.2e}" for n, v in zip(NAMES, worst)))
    assert max(worst) <= 1e-13, worst


def test_table_truth_rows():
    x = np.array(XS)
    ls = [0, 1, 2, 17, 17, 64]
    tab = cr.table_truth(64, x, ls)
    with mpmath.workdps(50):
        for i, l in enumerate(ls):
            for j, xx in enumerate(x):
                for ix, v in enumerate(_closed_forms(l, float(xx))):
                    assert abs(float(tab[i, ix, j]) - float(v)) <= 1e-15, (l, xx, ix)


def test_truth_sums_are_the_table_contractions():
    """cl2corr_truth / corr2cl_truth against a dense evaluation from table_truth at lmax 40, conventions of transforms.py:115-204."""
    lmax = 40
    rng = np.random.default_rng(3)
    x = np.sort(rng.uniform(-1, 1, lmax + 1))
    w = rng.uniform(0.1, 1.0, lmax + 1)
    tab = cr.table_truth(lmax, x, range(lmax + 1)).astype(np.float64)  # [l][ix][k]
    cls = cr.red_spectra(rng, lmax, 3)
    f = (2 * np.arange(lmax + 1) + 1) / (4 * np.pi)
    for s in range(3):
        c = cls[s]
        want = np.stack([(f * c[:, 0]) @ tab[:, 0], (f * (c[:, 1] + c[:, 2])) @ tab[:, 1], (f * (c[:, 1] - c[:, 2])) @ tab[:, 2],
                         (f * c[:, 3]) @ tab[:, 3]], axis=-1)
        np.testing.assert_allclose(cr.cl2corr_truth(cls, x)[s].astype(np.float64), want, rtol=0, atol=1e-14)
    xi = rng.standard_normal((2, lmax + 1, 4))
    got = cr.corr2cl_truth(xi, x, w).astype(np.float64)
    for s in range(2):
        t0 = tab[:, 0] @ (w * xi[s, :, 0])
        t2 = tab[:, 1] @ (w * xi[s, :, 1] / 2)
        t4 = tab[:, 2] @ (w * xi[s, :, 2] / 2)
        t3 = tab[:, 3] @ (w * xi[s, :, 3])
        want = 2 * np.pi * np.stack([t0, t2 + t4, t2 - t4, t3], axis=-1)
        np.testing.assert_allclose(got[s], want, rtol=0, atol=1e-13)
    # a subset of the nodes: the same as pulses on the full set
    sub = np.array([0, 5, lmax])
    pulses = np.zeros((3, lmax + 1, 4))
    pulses[np.arange(3), sub] = 1.0
    full = cr.corr2cl_truth(pulses, x, w)
    part = cr.corr2cl_truth(pulses[:, sub], x[sub], w[sub], lmax=lmax)
    assert np.abs(full - part).max() == 0


@pytest.mark.parametrize("lmax", [97, 300, 1024, 2048])
def test_oracle_against_truth(oracle, lmax):
    """The yardstick re-measured inside the suite: the oracle (the reference's closed forms in double) against the long-double truth at
    the oracle's own nodes.  Only loose sanity is asserted; the per-column, per-band figures go to the log."""
    rng = np.random.default_rng(lmax)
    x, w = oracle.gauss_legendre(lmax + 1)
    cls = cr.red_spectra(rng, lmax, 1)
    truth = cr.cl2corr_truth(cls, x)
    got = oracle.cl2corr(cls[0])[None]
    bands = cr.node_bands(x)
    err = np.abs(got.astype(cr.LD) - truth).astype(np.float64)[0]
    scale = np.abs(truth).max(axis=(0, 1)).astype(np.float64)
    print(f"\noracle.cl2corr vs truth, lmax {lmax}: max|err| / max|xi| per column [T, Q+U, Q-U, X] and node band")
    for name, m in bands.items():
        if m.any():
            print(f"  {name:>8}: " + " ".join(f"{v:.2e}" for v in err[m].max(axis=0) / scale))
    assert (err.max(axis=0) <= 1e-8 * scale).all(), err.max(axis=0) / scale
    assert int(np.argmax(err[:, 1])) < 8, "the worst node of Q+U is expected among the 8 nearest x = -1"
    xi = truth.astype(np.float64)
    back_truth = cr.corr2cl_truth(xi, x, w)
    back = oracle.corr2cl(xi[0])[None]
    e2 = np.abs(back.astype(cr.LD) - back_truth).astype(np.float64)[0] * (1.0 + np.arange(lmax + 1))[:, None] ** 2
    print(f"oracle.corr2cl vs truth, lmax {lmax}: max |err| (1+l)^2 per column [TT, EE, BB, TE]: " + " ".join(f"{v:.2e}" for v in e2.max(axis=0)))
    for name, m in cr.ell_bands(lmax).items():
        print(f"  {name:>8}: " + " ".join(f"{v:.2e}" for v in e2[m].max(axis=0)))
    assert e2.max() <= 1e-8, e2.max(axis=0)
