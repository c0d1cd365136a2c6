"""Host side of the rotation of alms (no GPU): the numpy restatement (tests/rotation_reference.py) pinned through the defining identity
f'(n) = f(R^-1 n) and the properties of the Wigner matrices, the Euler-angle and coordinate-system helpers of
``heracles_amd.rotation``, and its tile constants against the kernel source."""

import os
import re

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
