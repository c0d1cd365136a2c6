"""Ground truth of the truncated pseudo-inverse (numpy only, no GPU, no LAPACK): an unblocked one-sided Jacobi (Hestenes) SVD in
np.longdouble on the taller orientation of the matrix, the comparison rule the GPU tests of ``hx_pinv`` use, and the test matrices.

The Jacobi: columns are paired by a round-robin tournament (circle method); the rotations of a round act on disjoint pairs and are
applied together.  It stops when every pair of non-null columns is orthogonal to 8 long-double ulps, |w_p . w_q| <= 8 eps |w_p| |w_q|.
A column counts as null below 1e-17 of the matrix' Frobenius norm: 100 times below what any double-precision routine can resolve and
1000 times below the smallest ``rcond`` in use here, so a null column is always a dropped one.  Two null columns are not rotated
against each other (they are rounding noise; orthogonalising noise takes most of the sweeps of a rank-deficient matrix and changes
nothing that is kept); a null column is still rotated against a non-null one.  Then the columns of W are u_j sigma_j, those of V are
v_j, and

    pinv(M) = sum_j v_j w_j^T / sigma_j^2   over sigma_j > rcond sigma_max   (numpy's rule)

The columns are held as ROWS (W^T, V^T): a round gathers and scatters whole rows.

The comparison rule (``pinv_errors``): with X_ref the long-double result on the same double-rounded input,

    e_gpu = |X - X_ref|_F,  e_lapack = |np.linalg.pinv(M, rcond) - X_ref|_F,  allowed: e_gpu <= 4 max(e_lapack, tau |X_ref|_F),
    tau = max(1e-14, 16 * 1.1e-16 sqrt(n_tall))

tau is the orthogonality ``hx_pinv`` itself stops at; LAPACK is what the reference project calls; the factor 4 covers the different
summation orders of two backward-stable double algorithms.  Nothing in the rule is taken from the output under test."""

import collections
import functools

import numpy as np

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
if EPS_LD > 2e-19:
    raise RuntimeError(f"np.longdouble has eps {EPS_LD:.3g} on this platform (an 80-bit type with eps 1.08e-19 is needed): "
                       "a truth in double precision proves nothing about a double-precision kernel")

NULL_LEVEL = LD(1e-17)   # of the Frobenius norm
FACTOR = 4.0

PinvRef = collections.namedtuple("PinvRef", "pinv s kept")


def jacobi_svd(a, max_sweeps=60):
    """One-sided Jacobi of a (n x m, n >= m) in long double.  Returns (Wt, Vt, sweeps): Wt (m, n), row j = u_j sigma_j; Vt (m, m), row j
    = v_j.  (A padding column makes the count even for the tournament; it is removed again: it stays exactly zero.)"""
    a = np.asarray(a, dtype=LD)
    n, m = a.shape
    if n < m:
        raise ValueError("jacobi_svd wants the taller orientation")
    mp = m + (m & 1)
    Wt = np.zeros((mp, n), LD)
    Wt[:m] = a.T
    Vt = np.zeros((mp, mp), LD)
    Vt[np.arange(m), np.arange(m)] = 1
    tol = 8 * LD(EPS_LD)
    null2 = NULL_LEVEL * NULL_LEVEL * (Wt * Wt).sum()
    k = np.arange(mp // 2)
    one = LD(1)
    for sweep in range(max_sweeps):
        off = LD(0)
        for r in range(mp - 1):
            p = np.where(k == 0, mp - 1, (r + k) % (mp - 1))
            q = np.where(k == 0, r, (r - k + (mp - 1)) % (mp - 1))
            wp, wq = Wt[p], Wt[q]
            app, aqq, apq = (wp * wp).sum(1), (wq * wq).sum(1), (wp * wq).sum(1)
            d = np.sqrt(app) * np.sqrt(aqq)
            pos = d > 0
            rel = np.where(pos, np.abs(apq) / np.where(pos, d, one), 0)
            live_p, live_q = app > null2, aqq > null2
            both = live_p & live_q
            if both.any():
                off = max(off, rel[both].max())
            act = (rel > tol) & (apq != 0) & (live_p | live_q)
            if not act.any():
                continue
            tau = np.where(act, (aqq - app) / np.where(act, 2 * apq, one), 0)
            t = np.where(act, np.where(tau >= 0, one, -one) / (np.abs(tau) + np.sqrt(1 + tau * tau)), 0)
            c = 1 / np.sqrt(1 + t * t)
            s = t * c
            c, s = c[:, None], s[:, None]
            Wt[p], Wt[q] = c * wp - s * wq, s * wp + c * wq
            vp, vq = Vt[p], Vt[q]
            Vt[p], Vt[q] = c * vp - s * vq, s * vp + c * vq
        if off <= tol:
            break
    else:
        raise RuntimeError(f"jacobi_svd: no convergence in {max_sweeps} sweeps (largest |w_p.w_q| / |w_p||w_q| = {float(off):.3g})")
    return Wt[:m], Vt[:m, :m], sweep + 1


def pinv_reference(a, rcond):
    """Long-double pinv(a, rcond) of a (n x m, any orientation): PinvRef(pinv (m x n, long double), s (min(n, m) singular values,
    descending, long double; those below the null level are noise), kept (how many are > rcond * s[0]))."""
    return pinv_from_factors(factors(a), rcond)


def factors(a):
    """(Wt, Vt, transposed) of a matrix of any orientation: the expensive part, reusable for several ``rcond``."""
    a = np.asarray(a, dtype=LD)
    if a.ndim != 2:
        raise ValueError("the reference wants a matrix")
    tr = a.shape[0] < a.shape[1]
    Wt, Vt, _ = jacobi_svd(a.T if tr else a)
    return Wt, Vt, tr


def pinv_from_factors(f, rcond):
    Wt, Vt, tr = f
    s2 = (Wt * Wt).sum(1)
    s = np.sqrt(s2)
    keep = (s > LD(rcond) * s.max()) & (s > 0)
    inv = np.where(keep, 1 / np.where(keep, s2, LD(1)), 0)
    X = (Vt * inv[:, None]).T @ Wt
    return PinvRef(X.T if tr else X, np.sort(s)[::-1], int(keep.sum()))


def tau(n_tall):
    """The orthogonality hx_pinv stops at (hx_svd.hip: ``tol``) for a matrix whose longer side is n_tall."""
    return max(1e-14, 16.0 * 1.1e-16 * np.sqrt(float(n_tall)))


def fro(x):
    x = np.asarray(x, dtype=LD)
    return float(np.sqrt((x * x).sum()))


def pinv_errors(x, M, rcond, ref, lapack=None):
    """The figures of the comparison rule for a candidate x of pinv(M, rcond): dict(e_gpu, e_lapack, floor = tau |X_ref|_F, ratio =
    e_gpu / max(e_lapack, floor)).  ``lapack``: np.linalg.pinv(M, rcond) if the caller holds it already."""
    M = np.asarray(M, dtype=np.float64)
    xr = ref.pinv if isinstance(ref, PinvRef) else np.asarray(ref, dtype=LD)
    x = np.asarray(x)
    if x.shape != xr.shape:
        raise ValueError(f"pinv of shape {x.shape}, expected {xr.shape}")
    if lapack is None:
        lapack = np.linalg.pinv(M, rcond=rcond)
    e_gpu = fro(x.astype(LD) - xr)
    e_lapack = fro(lapack.astype(LD) - xr)
    floor = tau(max(M.shape)) * fro(xr)
    return {"e_gpu": e_gpu, "e_lapack": e_lapack, "floor": floor, "ratio": e_gpu / max(e_lapack, floor) if max(e_lapack, floor) > 0 else
            (0.0 if e_gpu == 0 else np.inf)}


def assert_pinv_close(x, M, rcond, ref, lapack=None, label=""):
    """Assert the comparison rule; prints the figures first (pytest -s shows them).  Returns the ratio."""
    x = np.asarray(x)
    assert np.isfinite(x).all(), f"{label}: non-finite entries in the pinv"
    e = pinv_errors(x, M, rcond, ref, lapack)
    print(f"pinv {label} {np.shape(M)} rcond={rcond:.3g}: e_gpu={e['e_gpu']:.3e} e_lapack={e['e_lapack']:.3e} floor={e['floor']:.3e} "
          f"ratio={e['ratio']:.3f}")
    assert e["e_gpu"] <= FACTOR * max(e["e_lapack"], e["floor"]), \
        f"{label}: |X - X_ref|_F = {e['e_gpu']:.3e} > {FACTOR:g} max(LAPACK's {e['e_lapack']:.3e}, tau |X_ref|_F = {e['floor']:.3e})"
    return e["ratio"]


# ---- matrices ----------------------------------------------------------------------------------------------------------------
def orthonormal_ld(n, k, rng, reflectors=3):
    """n x k with orthonormal columns in long double: the first k columns of a product of Householder reflectors I - 2 v v^T / v.v."""
    q = np.zeros((n, k), LD)
    q[np.arange(k), np.arange(k)] = 1
    if n == 1:
        return q
    for _ in range(reflectors):
        v = rng.standard_normal(n).astype(LD)
        q -= np.outer(v, (2 / (v * v).sum()) * (v @ q))
    return q


def with_spectrum_ld(n, m, s, seed):
    """(M, U, V) in long double: M = U diag(s) V^T (n x m), len(s) = min(n, m), U and V products of Householder reflectors."""
    rng = np.random.default_rng(seed)
    s = np.asarray(s, dtype=LD)
    k = min(n, m)
    assert s.shape == (k,)
    U, V = orthonormal_ld(n, k, rng), orthonormal_ld(m, k, rng)
    return (U * s) @ V.T, U, V


def gaussian(n, m, seed=None):
    return np.random.default_rng(n * 1000 + m if seed is None else seed).standard_normal((n, m))


def graded(n, m, decades=8, seed=None):
    """U diag(logspace(0, -decades)) V^T, rounded to double."""
    k = min(n, m)
    s = LD(10) ** (-LD(decades) * np.arange(k, dtype=LD) / max(k - 1, 1))
    return with_spectrum_ld(n, m, s, n * 1000 + m if seed is None else seed)[0].astype(np.float64)


def column_scaled(n, m, decades=12, seed=None):
    """A diag(logspace(0, -decades)), A Gaussian: small singular values that are defined to high relative accuracy by the entries."""
    return gaussian(n, m, seed) * np.logspace(0, -decades, m)


def band(n, m, width=3.0):
    """exp(-((i - j) / width)^2 / 2): a mixing-matrix-like band without noise; its singular values fall smoothly to rounding level."""
    i, j = np.arange(n)[:, None], np.arange(m)[None, :]
    return np.exp(-0.5 * ((i - j) / width) ** 2)


def rcond_between(s, target, min_gap=1.05):
    """rcond in the middle (geometric mean) of the two adjacent reference singular values whose middle, relative to s[0], is nearest to
    ``target``; asserts that both neighbours are at least ``min_gap`` away from the cut (a condition on the case, not a measurement of
    the code under test).  Returns (rcond, kept)."""
    s = np.asarray(s, dtype=LD)
    live = int(np.sum(s > NULL_LEVEL * 100 * s[0]))
    assert live >= 2
    mid = np.sqrt(s[:live - 1] * s[1:live]) / s[0]
    i = int(np.argmin(np.abs(np.log(mid.astype(np.float64)) - np.log(target))))
    rc = float(mid[i])
    cut = LD(rc) * s[0]
    assert s[i] >= min_gap * cut and cut >= min_gap * s[i + 1], (float(s[i] / cut), float(cut / s[i + 1]))
    return rc, i + 1


def _gap_ok(s, rc, min_gap):
    s = np.asarray(s, dtype=LD)
    cut = LD(rc) * s[0]
    above, below = s[s > cut], s[s <= cut]
    return above.size > 0 and above.min() >= min_gap * cut and (below.size == 0 or cut >= min_gap * below.max())


def rcond_common(spectra, target, min_gap=1.05):
    """One rcond for several matrices (the three a spin-2 key inverts share one): the middle of two adjacent singular values of any of
    them that is nearest to ``target`` among those that leave every spectrum a gap of ``min_gap`` on both sides of its cut.
    Returns (rcond, [kept per spectrum])."""
    cands = []
    for s in spectra:
        s = np.asarray(s, dtype=LD)
        live = s[s > NULL_LEVEL * 100 * s[0]]
        cands += [float(c) for c in np.sqrt(live[:-1] * live[1:]) / s[0]]
    for rc in sorted(cands, key=lambda c: abs(np.log(c / target))):
        if all(_gap_ok(s, rc, min_gap) for s in spectra):
            return rc, [int(np.sum(np.asarray(s, dtype=LD) > LD(rc) * LD(s[0]))) for s in spectra]
    raise AssertionError("no common rcond with a gap in every spectrum")


@functools.lru_cache(maxsize=None)
def kron_case():
    """M = A (x) B at a size near production, with an exact answer: A (35 x 33) has 27 singular values from 1 to 0.3 and 6 near 1e-7, B
    (64 x 63) from 1 to 0.2; at rcond = 1e-5 the cut falls between A's groups, and pinv_cut(M) = pinv_cut(A) (x) pinv(B) from two small
    references (the singular values of a Kronecker product are the products).  A and B are doubles; M is their product rounded to
    double (relative 1.1e-16 per entry: LAPACK's distance to the exact answer is measured on the same M).
    Returns dict(M (2240 x 2079, float64), rcond, ref = PinvRef(pinv, s, kept))."""
    sa = np.concatenate([np.linspace(1.0, 0.3, 27), 1e-7 * np.linspace(1.0, 0.5, 6)])
    sb = np.linspace(1.0, 0.2, 63)
    A = with_spectrum_ld(35, 33, sa, 351)[0].astype(np.float64)
    B = with_spectrum_ld(64, 63, sb, 641)[0].astype(np.float64)
    rcond = 1e-5
    ra, rb = pinv_reference(A, rcond), pinv_reference(B, 1e-12)
    assert ra.kept == 27 and rb.kept == 63
    M = np.kron(A.astype(LD), B.astype(LD)).astype(np.float64)
    s = np.sort(np.outer(ra.s, rb.s).ravel())[::-1]
    kept = int(np.sum(s > LD(rcond) * s[0]))
    assert kept == 27 * 63 and s[kept - 1] >= 1.05 * rcond * s[0] and rcond * s[0] >= 1.05 * s[kept]
    return {"M": M, "rcond": rcond, "ref": PinvRef(np.kron(ra.pinv, rb.pinv), s, kept)}
