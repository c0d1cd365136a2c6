"""tests/svd_reference.py (the long-double one-sided Jacobi pinv the GPU tests of ``hx_pinv`` are compared with) against what is known
without it: matrices built in long double from chosen singular values, the four Penrose conditions, LAPACK on well-conditioned input,
the Kronecker identity -- and the comparison rule against answers that are wrong on purpose, so that the GPU tests are known to be
able to fail."""

import functools

import numpy as np
import pytest

import svd_reference as sr

LD = sr.LD


def _fro(x):
    return sr.fro(x)


@pytest.mark.parametrize("shape", [(1, 1), (5, 4), (40, 24), (33, 33), (24, 40), (65, 31), (130, 64)])
def test_known_singular_values_come_back(shape):
    """M = U diag(s) V^T built in long double (U, V: products of Householder reflectors), s from 2 to 0.5.  The construction itself
    rounds at eps_ld |M| (1.1e-19 sqrt(k) or so), i.e. the singular values of the matrix handed over are the chosen ones to
    kappa eps_ld sqrt(k) = 4 * 1.1e-19 * 8 = 3.5e-18 relative: the reference must return them, and V diag(1/s) U^T, to 1e-17."""
    n, m = shape
    k = min(n, m)
    s = np.linspace(LD(2), LD(0.5), k) if k > 1 else np.array([LD(2)])
    M, U, V = sr.with_spectrum_ld(n, m, s, 11 * n + m)
    ref = sr.pinv_reference(M, 1e-3)
    assert ref.kept == k and ref.s.dtype == LD and ref.pinv.dtype == LD and ref.pinv.shape == (m, n)
    assert float(np.max(np.abs(ref.s - s) / s)) <= 1e-17
    exact = (V / s) @ U.T
    assert _fro(ref.pinv - exact) <= 1e-17 * _fro(exact)


def test_cut_in_a_known_spectrum():
    """Two groups of chosen singular values, 1 .. 0.5 and 1e-6 (1 .. 0.5): rcond = 1e-4 keeps the first group only.  The kept part is
    perturbed by the construction's rounding (eps_ld) and, through the cut, not by the dropped group."""
    s = np.concatenate([np.linspace(LD(1), LD(0.5), 20), LD(1e-6) * np.linspace(LD(1), LD(0.5), 11)])
    M, U, V = sr.with_spectrum_ld(50, 31, s, 5)
    ref = sr.pinv_reference(M, 1e-4)
    assert ref.kept == 20
    assert float(np.max(np.abs(ref.s[:20] - s[:20]) / s[:20])) <= 1e-17
    assert float(np.max(np.abs(ref.s[20:] - s[20:]) / s[20:])) <= 1e-11   # (absolute 1e-19 of the largest on values of 1e-6)
    exact = (V[:, :20] / s[:20]) @ U[:, :20].T
    assert _fro(ref.pinv - exact) <= 1e-17 * _fro(exact)
    assert sr.pinv_reference(M, 1e-8).kept == 31 and sr.pinv_reference(M, 1.0).kept == 0


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "gauss":
        M, rc = sr.gaussian(97, 33), 1e-10
    elif name == "gauss_wide":
        M, rc = sr.gaussian(33, 97), 1e-10
    elif name == "graded":
        M = sr.graded(97, 33)
        rc = sr.rcond_between(sr.pinv_reference(M, 0.0).s, 3e-6)[0]
    elif name == "colscaled":
        M, rc = sr.column_scaled(65, 31), 1e-14
    elif name == "band":
        M = sr.band(64, 48)
        rc = sr.rcond_between(sr.pinv_reference(M, 0.0).s, 1e-5)[0]
    M.setflags(write=False)
    return M, rc, sr.pinv_reference(M, rc)


@pytest.mark.parametrize("name", ["gauss", "gauss_wide", "graded", "colscaled", "band"])
def test_penrose_conditions(name):
    """M X M = M, X M X = X, (M X)^T = M X, (X M)^T = X M for the TRUNCATED matrix M_k = sum of the kept triplets, which X is the exact
    pseudo-inverse of; M_k is rebuilt from X itself (pinv(pinv(M_k)) = M_k) only in the first condition's residual form: all four are
    evaluated in long double on M restricted by the projectors X gives: P = M X and R = X M are symmetric projectors of rank kept."""
    M, rc, ref = _case(name)
    Ml, X = M.astype(LD), ref.pinv
    P, R = Ml @ X, X @ Ml
    nx, nm = _fro(X), _fro(Ml)
    # conditions 3 and 4 hold for the truncated inverse of M itself: M X = U_k U_k^T, X M = V_k V_k^T
    assert _fro(P - P.T) <= 1e-17 * nm * nx
    assert _fro(R - R.T) <= 1e-17 * nm * nx
    # condition 2, and idempotence with the right rank
    assert _fro(X @ P - X) <= 1e-17 * nx * nm * nx
    assert _fro(P @ P - P) <= 1e-17 * (nm * nx) ** 2
    assert abs(float(np.trace(P)) - ref.kept) <= 1e-15 * nm * nx and abs(float(np.trace(R)) - ref.kept) <= 1e-15 * nm * nx
    # condition 1 on the kept part: M_k = P M, and M_k X M_k = M_k
    Mk = P @ Ml
    assert _fro(Mk @ X @ Mk - Mk) <= 1e-17 * nm * nx * nm
    # what was cut is no larger than the cut: |M - M_k|_2 <= rcond s_max (Frobenius: times sqrt of the number dropped)
    dropped = len(ref.s) - ref.kept
    assert _fro(Ml - Mk) <= float(rc * ref.s[0]) * np.sqrt(max(dropped, 1)) * (1 + 1e-10) + 1e-17 * nm


@pytest.mark.parametrize("shape", [(5, 4), (64, 64), (97, 33), (33, 97), (130, 65)])
def test_agrees_with_lapack_where_lapack_is_good(shape):
    """Gaussian matrices (kappa of a few to a few hundred): np.linalg.svd / pinv are backward stable in double, so they sit within
    a modest multiple of 1.1e-16 kappa of the truth: 1e-13 relative (Frobenius) in the pinv, 1e-14 of the largest in every singular value."""
    M = sr.gaussian(*shape, seed=shape[0] + 7 * shape[1])
    ref = sr.pinv_reference(M, 1e-10)
    assert ref.kept == min(shape)
    s = np.linalg.svd(M, compute_uv=False)
    assert float(np.max(np.abs(s - ref.s))) <= 1e-14 * s[0]
    assert _fro(np.linalg.pinv(M, rcond=1e-10) - ref.pinv) <= 1e-13 * _fro(ref.pinv)


def test_kronecker_identity():
    """pinv(A (x) B) = pinv(A) (x) pinv(B), singular values = all products: the reference on the 48 x 35 product against itself on the
    two factors, with a cut that falls in a gap of the products' spectrum."""
    A = sr.with_spectrum_ld(8, 7, np.concatenate([np.linspace(LD(1), LD(0.5), 5), [LD(1e-4), LD(5e-5)]]), 1)[0].astype(np.float64)
    B = sr.with_spectrum_ld(6, 5, np.linspace(LD(1), LD(0.4), 5), 2)[0].astype(np.float64)
    K = np.kron(A.astype(LD), B.astype(LD))   # exact to eps_ld: the reference takes long-double input as it is
    rk, ra, rb = sr.pinv_reference(K, 1e-2), sr.pinv_reference(A, 1e-2), sr.pinv_reference(B, 1e-8)
    assert (ra.kept, rb.kept, rk.kept) == (5, 5, 25)
    want = np.kron(ra.pinv, rb.pinv)
    assert _fro(rk.pinv - want) <= 1e-16 * _fro(want)    # (eps_ld kappa of the product: 1.1e-19 * 5e4)
    prod = np.sort(np.outer(ra.s, rb.s).ravel())[::-1]
    assert float(np.max(np.abs(rk.s - prod) / prod[0])) <= 1e-17


def test_kron_case_is_what_it_says():
    c = sr.kron_case()
    assert c["M"].shape == (2240, 2079) and c["M"].dtype == np.float64 and c["ref"].kept == 1701
    assert c["ref"].pinv.shape == (2079, 2240)
    assert abs(float(c["ref"].s[0]) - 1.0) < 1e-12 and abs(float(c["ref"].s[1700]) - 0.06) < 1e-12


def test_rcond_between_refuses_a_cut_without_a_gap():
    s = np.array([1.0, 0.5, 0.49, 0.1])
    rc, kept = sr.rcond_between(s, 0.22)
    assert kept == 3 and abs(rc - np.sqrt(0.049)) < 1e-15
    with pytest.raises(AssertionError):
        sr.rcond_between(s, 0.495)


# ---- the comparison rule must be able to fail --------------------------------------------------------------------------------
def _triplets(M, rc):
    """Kept / dropped triplets of M from the reference's own factors: (s, U columns, V columns), descending."""
    tr = M.shape[0] < M.shape[1]
    Wt, Vt, _ = sr.jacobi_svd((M.T if tr else M).astype(LD))
    s = np.sqrt((Wt * Wt).sum(1))
    order = np.argsort(-s)
    s, Ut, Vt = s[order], Wt[order] / s[order][:, None], Vt[order]
    return (s, Vt, Ut) if tr else (s, Ut, Vt)   # rows: u_j (length n), v_j (length m) of M as given


@pytest.mark.parametrize("name", ["gauss", "gauss_wide", "graded", "colscaled", "band"])
def test_the_rule_accepts_lapack_and_the_reference(name):
    M, rc, ref = _case(name)
    assert sr.assert_pinv_close(ref.pinv.astype(np.float64), M, rc, ref, label=name) <= 1.0
    assert sr.assert_pinv_close(np.linalg.pinv(M, rcond=rc), M, rc, ref, label=name) <= 1.0


_WRONG = [(name, wrong) for name in ("gauss", "gauss_wide", "graded", "band")
          for wrong in ("kept_one_fewer", "kept_one_more", "smallest_scaled_1e-9", "corner_transposed")
          if not (wrong == "kept_one_more" and name.startswith("gauss"))]   # (nothing is dropped in the Gaussian cases)


@pytest.mark.parametrize("name,wrong", _WRONG)
def test_the_rule_rejects_a_wrong_answer(name, wrong):
    """Each of these is the kind of error a subtly wrong kernel makes: a cut on the wrong side of one singular value, a smallest kept
    singular value that is right to nine digits only, two entries in each other's place."""
    M, rc, ref = _case(name)
    s, Ut, Vt = _triplets(M, rc)
    k = ref.kept
    X = ref.pinv.copy()
    if wrong == "kept_one_fewer":
        X -= np.outer(Vt[k - 1], Ut[k - 1]) / s[k - 1]
    elif wrong == "kept_one_more":
        assert k < len(s)
        X += np.outer(Vt[k], Ut[k]) / s[k]
    elif wrong == "smallest_scaled_1e-9":
        X += LD(1e-9) * np.outer(Vt[k - 1], Ut[k - 1]) / s[k - 1]
    else:
        X[0, 1], X[1, 0] = X[1, 0], X[0, 1]
    with pytest.raises(AssertionError, match="max\\(LAPACK"):
        sr.assert_pinv_close(X.astype(np.float64), M, rc, ref, label=f"{name}/{wrong}")


def test_the_rule_rejects_non_finite_and_misshapen():
    M, rc, ref = _case("gauss")
    X = ref.pinv.astype(np.float64)
    X[3, 3] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        sr.assert_pinv_close(X, M, rc, ref)
    with pytest.raises(ValueError):
        sr.pinv_errors(ref.pinv.T, M, rc, ref)
