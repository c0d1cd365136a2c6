"""tests/spin_synthesis_reference.py against what the project already trusts: the explicit finite sum ``helpers.sYlm`` over
l and ALL m, the oracle's alm2map at spin 2, and the adjoint identity with ``points2alm_spin``.  No GPU."""
import numpy as np
import pytest

import helpers
from oracle import hxoracle as oracle
from spin_reference import points2alm_spin
from spin_synthesis_reference import alm2points_spin, harmonic_inner


def _points(rng, n):
    return np.arccos(rng.uniform(-1, 1, n)), rng.uniform(0, 2 * np.pi, n)


def _alm(rng, lmax, s, rows=2):
    return helpers.random_alm(rng, lmax, s, (rows,))


@pytest.mark.parametrize("s,lmax", [(1, 3), (2, 3), (3, 3), (1, 6), (2, 6), (3, 6), (4, 6), (5, 6), (4, 10), (5, 10), (8, 10)])
def test_values_against_explicit_sum(s, lmax):
    """Q + iU = sum_l sum_{m = -l..l} (+s)a_lm (+s)Y_lm with (+s)a_lm = -(E_lm + i B_lm) and E_{l,-m} = (-1)^m conj(E_lm) (B
    likewise), term by term from helpers.sYlm: 1e-10 of the largest value (the explicit sum's own cancellation)."""
    rng = np.random.default_rng(100 * s + lmax)
    theta, phi = _points(rng, 25)
    theta[:3] = [1e-3, np.pi - 1e-3, np.pi / 2]
    alm = _alm(rng, lmax, s, 4)
    got = alm2points_spin(theta, phi, alm, lmax, s)
    for f in range(2):
        e, b = alm[2 * f], alm[2 * f + 1]
        want = np.zeros(theta.size, dtype=complex)
        for l in range(s, lmax + 1):
            for m in range(-l, l + 1):
                i = helpers.idx(lmax, l, abs(m))
                elm = e[i] if m >= 0 else (-1) ** m * np.conj(e[i])
                blm = b[i] if m >= 0 else (-1) ** m * np.conj(b[i])
                want += -(elm + 1j * blm) * helpers.sYlm(s, l, m, theta, phi)
        scale = np.abs(want).max()
        assert np.abs(got[2 * f] - want.real).max() < 1e-10 * scale
        assert np.abs(got[2 * f + 1] - want.imag).max() < 1e-10 * scale


def test_spin2_is_the_oracle():
    nside, lmax = 4, 8
    rng = np.random.default_rng(8)
    alm = _alm(rng, lmax, 2)
    theta, phi = oracle.pix2ang(nside)
    got = alm2points_spin(theta, phi, alm, lmax, 2)
    want = oracle.alm2map(alm, nside, lmax, spin=2)
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("s", [1, 2, 3, 4, 5, 8])
def test_adjoint_of_points2alm_spin(s):
    """sum_p (Q_p Q'_p + U_p U'_p) = sum_{l, all m} Re(E conj(E') + B conj(B')) for (E, B) = points2alm_spin(Q, U) and
    (Q', U') = alm2points_spin(E', B'): both are sums of the same products, so they agree to rounding."""
    lmax, n = 20, 60
    rng = np.random.default_rng(30 + s)
    theta, phi = _points(rng, n)
    v = rng.normal(size=(2, n))
    alm = _alm(rng, lmax, s)
    back = alm2points_spin(theta, phi, alm, lmax, s)
    lhs = float(np.sum(v * back))
    rhs = harmonic_inner(points2alm_spin(theta, phi, v, lmax, s), alm, lmax)
    assert abs(lhs - rhs) < 1e-12 * np.sqrt(np.sum(v**2) * np.sum(back**2))  # (the Cauchy-Schwarz bound of lhs as the scale)


def test_orders_read_the_listed_rows_only():
    """``orders=`` is the synthesis of the alms with every other order set to zero, bit for bit."""
    lmax, s, n = 12, 3, 20
    rng = np.random.default_rng(6)
    theta, phi = _points(rng, n)
    alm = _alm(rng, lmax, s)
    assert np.array_equal(alm2points_spin(theta, phi, alm, lmax, s, orders=range(lmax + 1)), alm2points_spin(theta, phi, alm, lmax, s))
    ms = (7, 0, 2, 12)
    only = np.zeros_like(alm)
    for m in ms:
        i = helpers.idx(lmax, m, m)
        only[:, i : i + lmax - m + 1] = alm[:, i : i + lmax - m + 1]
    got = alm2points_spin(theta, phi, alm, lmax, s, orders=ms)
    assert np.array_equal(got, alm2points_spin(theta, phi, only, lmax, s)) and np.abs(got).max() > 0
    assert np.abs(got - alm2points_spin(theta, phi, alm, lmax, s)).max() > 0.1 * np.abs(got).max()  # (the other orders are not read)
