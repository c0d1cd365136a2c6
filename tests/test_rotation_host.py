"""Host side of the rotation of alms (no GPU): the numpy restatement (tests/rotation_reference.py) pinned through the defining identity
f'(n) = f(R^-1 n) and the properties of the Wigner matrices, the long-double column restatement that reaches production lmax
(against the eigh one, its seeds against exact integers, its row norms at lmax 2048), the Euler-angle and coordinate-system helpers of
``heracles_amd.rotation``, and its tile constants against the kernel source."""

import functools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import rotation_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ANGLES = [(0.3, 1.1, -2.2), (-1.9, 2.7, 0.4), (2.5, 0.05, 1.3)]


# ---- the restatement, pinned on its own ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("psi,theta,phi", ANGLES)
def test_reference_satisfies_the_defining_identity(psi, theta, phi):
    lmax, npts = 12, 200
    rng = np.random.default_rng(int(1000 * theta))
    alm = rr.random_alm(rng, lmax)
    th, ph = np.arccos(rng.uniform(-1, 1, npts)), rng.uniform(0, 2 * np.pi, npts)
    R = rr.rotation_matrix(psi, theta, phi)
    back_th, back_ph = rr.angles(R.T @ rr.directions(th, ph))  # R^-1 n
    want = rr.values(alm, lmax, back_th, back_ph)
    got = rr.values(rr.rotate_alm_ref(alm, lmax, psi, theta, phi), lmax, th, ph)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"identity: max |delta| = {err:.3e}, max |f| = {scale:.3e}")
    assert err <= 1e-12 * scale


@pytest.mark.parametrize("l", [0, 1, 2, 7, 33, 64])
def test_wigner_d_properties(l):
    t1, t2 = 0.83, 1.9
    d1, d2 = rr.wigner_d(l, t1), rr.wigner_d(l, t2)
    eye = np.eye(2 * l + 1)
    assert np.abs(d1.T @ d1 - eye).max() < 1e-13
    assert np.abs(rr.wigner_d(l, 0.0) - eye).max() < 1e-13
    assert np.abs(d1 @ d2 - rr.wigner_d(l, t1 + t2)).max() < 1e-13


def test_wigner_d_sign_convention():
    for theta in (0.4, 2.0, -1.1):
        d = rr.wigner_d(1, theta)
        assert abs(d[1 + 1, 0 + 1] + np.sin(theta) / np.sqrt(2)) < 1e-15  # d^1_10 = -sin(theta) / sqrt(2)
        assert abs(d[0 + 1, 1 + 1] - np.sin(theta) / np.sqrt(2)) < 1e-15
        assert abs(d[1, 1] - np.cos(theta)) < 1e-15


def test_wigner_d_at_pi():
    for l in (1, 4, 9):
        m = np.arange(-l, l + 1)
        want = np.zeros((2 * l + 1, 2 * l + 1))
        want[l + m, l - m] = (-1.0) ** (l + m)  # (-1)^(l - m') delta_(m, -m') at m' = -m
        assert np.abs(rr.wigner_d(l, np.pi) - want).max() < 1e-13


# ---- the long-double restatement that reaches production lmax, pinned on its own -----------------------------------------------------

def test_long_double_is_wider_than_double():
    """Asserted, not a skip condition: every comparison against ``rotate_column_ref`` rests on it (x86-64: 2^-63 = 1.08e-19)."""
    assert np.finfo(np.longdouble).eps < 2e-19


#: the angle edges of tests/test_gpu_rotate_alm.py and the angles at which the seeds leave the range of a double
COLUMN_THETAS = [1.234, 0.02, 3.1, 1e-8, np.pi - 1e-8, -0.7, 4.0]


@functools.lru_cache(maxsize=None)
def _alm_for(lmax):
    return rr.random_alm(np.random.default_rng(lmax), lmax)


@pytest.mark.parametrize("theta", COLUMN_THETAS)
@pytest.mark.parametrize("lmax", [96, 200])
def test_column_reference_against_the_eigh_restatement(lmax, theta):
    """Every column.  The bound is the eigh restatement's own figure (1e-12 of max |a_ref|); the difference measured is eigh's error,
    2e-15 .. 5e-14.  The float64 yardstick is printed, not asserted."""
    psi, phi = 0.4, -0.8
    alm = _alm_for(lmax)
    ref = rr.rotate_alm_ref(alm, lmax, psi, theta, phi)
    rows = rr.phased_rows(alm, lmax, psi)
    scale, worst, yard = np.abs(ref).max(), 0.0, 0.0
    for m in range(lmax + 1):
        col = rr.rotate_column_ref(alm, lmax, m, psi, theta, phi, rows=rows)
        assert col.shape == (lmax + 1 - m,) and np.isfinite(col.real).all() and np.isfinite(col.imag).all()
        worst = max(worst, float(np.abs(col - ref[rr.column_slice(lmax, m)]).max()))
        if m % 50 == 0:
            yard = max(yard, float(np.abs(rr.rotate_column_ref(alm, lmax, m, psi, theta, phi, np.float64, rows=rows) - col).max()))
    print(f"lmax {lmax} theta {theta!r}: column - eigh = {worst / scale:.2e} of max |a_ref|; float64 chains - long double (every 50th column) {yard / scale:.2e}")
    assert worst <= 1e-12 * scale
    assert (rr.rotate_column_ref(alm, lmax, 0, psi, theta, phi, rows=rows).imag == 0).all()


def test_column_reference_takes_dead_rows_as_zero():
    lmax, lmin = 40, 30
    alm = rr.sparse_alm(np.random.default_rng(4), lmax, lmin)
    l, _ = rr.lm_index(lmax)
    assert (alm[l < lmin] == 0).all() and (alm[l >= lmin] != 0).all()
    for m in (0, 7, 35):
        full = rr.rotate_column_ref(alm, lmax, m, 0.3, 0.9, -1.0)
        cut = rr.rotate_column_ref(alm, lmax, m, 0.3, 0.9, -1.0, lmin=lmin)
        assert (full == cut).all() and (cut[: max(lmin - m, 0)] == 0).all()


def _exact_seed_ratio(A, B, theta, mant, expo):
    """got / exact - 1 for the seed sqrt(C(2A, A+B)) c^(A+B) s^(A-B): the square in exact rationals (math.comb, the long doubles c
    and s as fractions), one integer square root to 128 bits."""
    def frac(v):
        mm, ee = np.frexp(v)
        return Fraction(int(np.ldexp(mm, 64))) * Fraction(2) ** (int(ee) - 64)

    c, s = rr.half_angle(theta)
    sq = math.comb(2 * A, A + B) * frac(c) ** (2 * (A + B)) * frac(s) ** (2 * (A - B))
    k = 128 - (sq.numerator.bit_length() - sq.denominator.bit_length()) // 2  # root ~ 2^128 after the shift
    root = Fraction(math.isqrt((sq.numerator << (2 * k + 2 * 128)) // sq.denominator), 2 ** (k + 128)) if k >= 0 else None
    if root is None:
        root = Fraction(math.isqrt((sq.numerator << 256) // (sq.denominator << (-2 * k))) << (-k), 2**128)
    got = frac(abs(mant)) * Fraction(2) ** int(expo)
    return float(got / root - 1)


@pytest.mark.parametrize("A,B,theta", [(5, 3, 1.234), (40, -17, 0.02), (700, 180, 0.02), (2048, 2, 1e-3), (2048, -1023, 1.234),
                                       (2048, 2047, np.pi - 0.02), (6144, 4096, 0.02), (6144, -5001, 1.097), (6144, 0, 1e-8)])
def test_chain_seeds_against_exact_integers(A, B, theta):
    """Relative error <= 1e-16 sqrt(A): 2A + 2A running products of long doubles (2^-64 each at most) stay far inside it."""
    lmax = A + 3
    for m, mp in ((A, B), (abs(B), A if B >= 0 else -A)):  # the seed as the start of column A, and of column |B| at m' = +-A
        mant, expo = rr.chain_seeds(lmax, m, theta)
        got_m, got_e = mant[mp + lmax], expo[mp + lmax]
        # d^A_(A,B) carries (-1)^(A-B); d^A_(|B|,+A) is positive, d^A_(|B|,-A) carries (-1)^(A+|B|) and swaps c and s
        if m == A:
            sign, b = (-1) ** (A - B), B
        else:
            sign, b = (1, abs(B)) if mp > 0 else ((-1) ** (A + abs(B)), -abs(B))
        s_half = rr.half_angle(theta)[1]
        assert np.sign(got_m) == sign * (np.sign(s_half) ** ((A - b) & 1))
        rel = _exact_seed_ratio(A, b, theta, got_m, got_e)
        print(f"A {A} B {b} theta {theta!r} column {m}: seed 2^{int(got_e)}, relative error {rel:.2e}, bound {1e-16 * np.sqrt(A):.2e}")
        assert abs(rel) <= 1e-16 * np.sqrt(A)


@pytest.mark.parametrize("theta", [1.234, 0.02, 1e-8, np.pi - 1e-3])
def test_row_norms_at_production_size(theta, m=1024):
    """sum_m' d^l_(m,m')(theta)^2 = 1 for every l of column 1024 at lmax 2048 (1024 steps of every chain), to 1e-15: the reference's
    accuracy certificate where eigh cannot go.  Measured: 8.1e-17 (1.234), 2.2e-18 (0.02), 9.5e-17 (1e-8), 7.6e-17 (pi - 1e-3); the
    seeds alone (2 m running products) give that much.  With the chains in the three-term form pi - 1e-3 gave 1.21e-15 and missed the
    bound: long-double rounding comes back 1 / sin(theta) larger there too, which is why the chains run in differences."""
    lmax, worst = 2048, 0.0
    for l, d in rr.wigner_d_column(lmax, m, theta):
        assert d.shape == (2 * l + 1,)
        worst = max(worst, abs(float(np.sum(d * d) - 1)))
    print(f"theta {theta!r} column {m}: max |sum d^2 - 1| = {worst:.2e}")
    assert worst <= 1e-15


# ---- Euler angles and matrices -----------------------------------------------------------------------------------------------------------

def test_matrix_from_euler_is_the_definition():
    import heracles_amd as hx

    for psi, theta, phi in ANGLES:
        assert np.abs(hx.matrix_from_euler(psi, theta, phi) - rr.rotation_matrix(psi, theta, phi)).max() < 1e-15
    # counter-clockwise about the fixed axes: Rz(90 deg) takes x to y, Ry(90 deg) takes z to x
    assert np.abs(hx.matrix_from_euler(np.pi / 2, 0, 0) @ [1, 0, 0] - [0, 1, 0]).max() < 1e-15
    assert np.abs(hx.matrix_from_euler(0, np.pi / 2, 0) @ [0, 0, 1] - [1, 0, 0]).max() < 1e-15


@pytest.mark.parametrize("psi,theta,phi", ANGLES + [(0.2, -0.7, 1.0), (0.2, 4.0, 1.0), (3.0, 1e-8, -3.0), (1.0, np.pi - 1e-8, 2.0)])
def test_euler_round_trip(psi, theta, phi):
    import heracles_amd as hx

    R = hx.matrix_from_euler(psi, theta, phi)
    a = hx.euler_from_matrix(R)
    assert 0.0 <= a[1] <= np.pi and all(-np.pi <= x <= np.pi for x in (a[0], a[2]))
    assert np.abs(hx.matrix_from_euler(*a) - R).max() < 1e-14
    if 0.0 < theta < np.pi:  # angles already in range come back themselves
        assert np.allclose(a, (psi, theta, phi), rtol=0, atol=1e-7)


@pytest.mark.parametrize("theta", [0.0, np.pi])
def test_euler_degenerate(theta):
    import heracles_amd as hx

    R = hx.matrix_from_euler(0.6, theta, -1.5)
    psi, th, phi = hx.euler_from_matrix(R)
    assert phi == 0.0 and th == theta
    assert np.abs(hx.matrix_from_euler(psi, th, phi) - R).max() < 1e-14


def test_euler_rejects_what_is_no_rotation():
    import heracles_amd as hx

    R = hx.matrix_from_euler(0.3, 1.1, -2.2)
    with pytest.raises(ValueError, match="reflection"):
        hx.euler_from_matrix(R @ np.diag([1.0, 1.0, -1.0]))
    bad = R.copy()
    bad[0, 1] += 1e-9
    with pytest.raises(ValueError, match="orthogonal"):
        hx.euler_from_matrix(bad)
    with pytest.raises(ValueError, match="3 x 3"):
        hx.euler_from_matrix(np.eye(2))
    with pytest.raises(ValueError, match="once"):
        hx.rotate_alm(np.zeros(3, dtype=complex), 0.1, 0.2, 0.3, matrix=R)
    with pytest.raises(ValueError, match="once"):
        hx.rotate_alm(np.zeros(3, dtype=complex), matrix=R, coord=("G", "C"))
    with pytest.raises(ValueError, match="coefficients"):
        hx.rotate_alm(np.zeros(4, dtype=complex), 0.1, 0.2, 0.3)


# ---- coordinate systems ------------------------------------------------------------------------------------------------------------------

def _radec(v):
    return np.degrees(np.arctan2(v[1], v[0])) % 360.0, np.degrees(np.arcsin(v[2] / np.linalg.norm(v)))


def test_coord_matrix_known_answers():
    import heracles_amd as hx

    tol = 1e-4  # degrees: the rounding of the published constants
    gc = hx.coord_matrix("G", "C")
    ra, dec = _radec(gc @ [0.0, 0.0, 1.0])  # the galactic pole
    assert abs(ra - 192.85948) < tol and abs(dec - 27.12825) < tol
    ra, dec = _radec(gc @ [1.0, 0.0, 0.0])  # the galactic centre
    assert abs(ra - 266.40499) < tol and abs(dec + 28.93617) < tol
    ra, dec = _radec(hx.coord_matrix("E", "C") @ [0.0, 0.0, 1.0])  # the ecliptic pole
    assert abs(ra - 270.0) < tol and abs(dec - (90.0 - 23.4392911)) < tol


def test_coord_matrix_group_properties():
    import heracles_amd as hx

    tol = 1e-14  # products of two or three 3 x 3 orthogonal matrices in doubles: a few dozen 2^-53

    for a in "CGE":
        assert np.abs(hx.coord_matrix(a, a) - np.eye(3)).max() < tol
        for b in "CGE":
            M = hx.coord_matrix(a, b)
            assert np.abs(M - hx.coord_matrix(b, a).T).max() < tol
            assert np.abs(M.T @ M - np.eye(3)).max() < tol and np.linalg.det(M) > 0
            hx.euler_from_matrix(M)  # passes the orthogonality check
    assert np.abs(hx.coord_matrix("G", "E") - hx.coord_matrix("C", "E") @ hx.coord_matrix("G", "C")).max() < tol
    with pytest.raises(ValueError, match="unknown coordinate system"):
        hx.coord_matrix("G", "X")


# ---- the kernel's constants ---------------------------------------------------------------------------------------------------------------

def test_tile_constants_restated_in_python_match_the_kernel():
    from heracles_amd import rotation

    text = open(os.path.join(ROOT, "heracles_amd", "csrc", "hx_rotate.hip")).read()
    for name, value in (("ROT_CB", rotation.TILE_COMP), ("ROT_MO", rotation.TILE_COLS), ("ROT_MB", rotation.TILE_M), ("ROT_LB", rotation.TILE_L)):
        assert re.search(rf"constexpr int {name} = (\d+);", text).group(1) == str(value)


def test_exported():
    import heracles_amd as hx
    from heracles_amd import rotation

    for name in rotation.__all__:
        assert name in hx.__all__ and getattr(hx, name) is getattr(rotation, name)
    assert "hx_rotate_alm" in hx._lib.SYMBOLS
