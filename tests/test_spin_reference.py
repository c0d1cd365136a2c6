"""tests/spin_reference.py against what the project already trusts: the explicit finite sum ``helpers.sYlm`` for odd and even
weights up to 8 (more than three orders m < s, which start at l0 = s > m), and the oracle's direct sum at spin 2, up to lmax 6144
on a sample of m.  No GPU."""
import numpy as np
import pytest

import helpers
from oracle import hxoracle as oracle
from spin_reference import points2alm_spin, spin_lambda


def _points(rng, n):
    return np.arccos(rng.uniform(-1, 1, n)), rng.uniform(0, 2 * np.pi, n)


@pytest.mark.parametrize("s", [1, 3, 4, 5, 8])
def test_lambda_against_explicit_sum(s):
    """Both signed weights, every (l, m) up to lmax 16: 1e-10 of the largest value (the explicit sum's own cancellation)."""
    lmax = 16
    rng = np.random.default_rng(s)
    theta = np.concatenate([np.arccos(rng.uniform(-1, 1, 20)), [1e-3, np.pi - 1e-3, np.pi / 2]])
    zero = np.zeros_like(theta)
    for t in (+s, -s):
        for m in range(lmax + 1):
            got = spin_lambda(t, m, lmax, theta).astype(np.float64)
            l0 = max(m, s)
            want = np.array([helpers.sYlm(t, l, m, theta, zero).real for l in range(l0, lmax + 1)])
            assert got.shape == want.shape
            assert np.abs(got - want).max() < 1e-10 * max(np.abs(want).max(), 1.0), (t, m)


@pytest.mark.parametrize("s", [1, 3, 4, 5, 8])
def test_alms_against_explicit_sum(s):
    """The E / B combination of the definition, term by term from helpers.sYlm."""
    lmax, n = 16, 30
    rng = np.random.default_rng(10 + s)
    theta, phi = _points(rng, n)
    v = rng.normal(size=(4, n))
    got = points2alm_spin(theta, phi, v, lmax, s)
    want = np.zeros_like(got)
    for f in range(2):
        q, u = v[2 * f], v[2 * f + 1]
        for m in range(lmax + 1):
            for l in range(max(m, s), lmax + 1):
                ap = np.sum((q + 1j * u) * np.conj(helpers.sYlm(s, l, m, theta, phi)))
                am = np.sum((q - 1j * u) * np.conj(helpers.sYlm(-s, l, m, theta, phi)))
                i = helpers.idx(lmax, l, m)
                want[2 * f, i] = -(ap + (-1) ** s * am) / 2
                want[2 * f + 1, i] = 1j * (ap - (-1) ** s * am) / 2
    assert np.abs(got - want).max() < 1e-10 * np.abs(want).max()
    for m in range(min(s, lmax + 1)):  # rows l < s are zero
        i = helpers.idx(lmax, m, m)
        assert not got[:, i : i + s - m].any()


@pytest.mark.parametrize("lmax", [100, 300])
def test_spin2_is_the_oracle(lmax):
    rng = np.random.default_rng(lmax)
    n = 40
    theta, phi = _points(rng, n)
    theta[:3] = [1e-4, np.pi - 3e-4, np.pi / 2]
    v = rng.normal(size=(2, n))
    got = points2alm_spin(theta, phi, v, lmax, 2)
    want = oracle.points2alm(theta, phi, v, lmax, spin=2)
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max()


def test_orders_select_rows_and_leave_the_rest_zero():
    """``orders=`` computes the listed m only, bit for bit what the full transform holds there; every other row stays zero."""
    lmax, s, n = 12, 3, 20
    rng = np.random.default_rng(5)
    theta, phi = _points(rng, n)
    v = rng.normal(size=(2, n))
    full = points2alm_spin(theta, phi, v, lmax, s)
    assert np.array_equal(points2alm_spin(theta, phi, v, lmax, s, orders=range(lmax + 1)), full)
    ms = (7, 0, 2, 12, 7)  # (any iterable, in any order)
    got = points2alm_spin(theta, phi, v, lmax, s, orders=ms)
    rows = np.zeros(full.shape[1], dtype=bool)
    for m in ms:
        rows[helpers.idx(lmax, m, m) : helpers.idx(lmax, m, m) + lmax - m + 1] = True
    assert np.array_equal(got[:, rows], full[:, rows]) and np.abs(full[:, rows]).min(axis=0).max() > 0
    assert not got[:, ~rows].any()
    with pytest.raises(ValueError):
        points2alm_spin(theta, phi, v, lmax, s, orders=[lmax + 1])


def test_spin2_is_the_oracle_at_lmax_6144():
    """Full length on the orders 0, 1024, ..., 6144 (the oracle's Legendre stage restricted by set_mstride), 100 random points.
    Measured with 400 points: 6.7e-13 of max|alm|; the two form cos(theta) differently, hence 1e-11.  This is what entitles the
    full-size GPU tests of tests/test_gpu_spin_fullsize.py to their 1e-10 yardstick."""
    lmax, n, stride = 6144, 100, 1024
    rng = np.random.default_rng(lmax)
    theta, phi = _points(rng, n)
    v = rng.normal(size=(2, n))
    got = points2alm_spin(theta, phi, v, lmax, 2, orders=range(0, lmax + 1, stride))
    oracle.set_mstride(stride)
    try:
        want = oracle.points2alm(theta, phi, v, lmax, spin=2)
    finally:
        oracle.set_mstride(1)
    worst = 0.0
    for m in range(0, lmax + 1, stride):
        lo = helpers.idx(lmax, m, m)
        worst = max(worst, np.abs(got[:, lo : lo + lmax - m + 1] - want[:, lo : lo + lmax - m + 1]).max())
    print(f"lmax {lmax}: {worst / np.abs(got).max():.3e} of max|alm|")
    assert np.abs(got).max() > 0 and worst < 1e-11 * np.abs(got).max()
