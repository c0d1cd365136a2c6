"""GPU parity of the point transform (hx_pointsht_adjoint) for fields of a spin weight other than 0 and 2, against the
long-double direct sum of tests/spin_reference.py (itself tied to helpers.sYlm and to the oracle by tests/test_spin_reference.py).
Tolerance: that of tests/test_gpu_pointsht.py for the same transform, 1e-11 of the largest |alm|."""
import numpy as np
import pytest

import helpers
from oracle import hxoracle as oracle
from spin_reference import points2alm_spin

pytestmark = pytest.mark.gpu


def _points(rng, n):
    theta = np.arccos(rng.uniform(-1, 1, n))
    phi = rng.uniform(0, 2 * np.pi, n)
    return theta, phi


def _err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


_CASES = {}


def _case(lmax, s, n, rows=4):
    """Points, values and reference alms: computed once, shared, never written."""
    key = (lmax, s, n, rows)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * lmax + 10 * s + rows)
        theta, phi = _points(rng, n)
        v = rng.normal(size=(rows, n))
        want = points2alm_spin(theta, phi, v, lmax, s)
        for a in (theta, phi, v, want):
            a.setflags(write=False)
        _CASES[key] = (theta, phi, v, want)
    return _CASES[key]


@pytest.mark.parametrize("lmax", [0, 1, 2, 3, 7, 31, 100])  # 3 with s = 3: only the rows l0 = s; 31: smallest oversampling
@pytest.mark.parametrize("s", [1, 3])
def test_random_points_against_direct_sum(lmax, s):
    import heracles_amd as hx

    theta, phi, v, want = _case(lmax, s, 500)
    got = hx.PointSHT(lmax).adjoint_synthesis(np.stack([theta, phi], axis=1), v, spin=s)
    assert got.shape == want.shape
    if s > lmax:
        assert np.abs(got).max() == 0.0
        return
    print(f"lmax {lmax} s {s}: err {_err(got, want):.3e}")
    assert _err(got, want) < 1e-11
    for m in range(min(s, lmax + 1)):  # rows l < s are exact zeros
        i = helpers.idx(lmax, m, m)
        assert not got[:, i : i + s - m].any()


# weights with more than three orders m < s (the m < s seeds, chains from l0 = s > m, off = (l0 + m) & 1 on both parities), even
# and odd; 8 with s = 8: s = lmax, one row per order
@pytest.mark.parametrize("lmax", [8, 31, 100])
@pytest.mark.parametrize("s", [4, 5, 8])
def test_higher_weights_against_direct_sum(lmax, s):
    import heracles_amd as hx

    theta, phi, v, want = _case(lmax, s, 500)
    got = hx.PointSHT(lmax).adjoint_synthesis(np.stack([theta, phi], axis=1), v, spin=s)
    assert got.shape == want.shape and np.abs(want).max() > 0
    print(f"lmax {lmax} s {s}: err {_err(got, want):.3e}")
    assert _err(got, want) < 1e-11
    for m in range(s):  # rows l < s are exact zeros
        i = helpers.idx(lmax, m, m)
        assert not got[:, i : i + s - m].any()


@pytest.mark.parametrize("s", [1, 3])
def test_lmax_300_all_m(s):
    """Ring pruning by ring_mlim(lmax, s) and the scaled seeds are live: sin^m(theta) underflows on the polar rings."""
    import heracles_amd as hx

    lmax = 300
    theta, phi, v, want = _case(lmax, s, 300, rows=2)
    got = hx.PointSHT(lmax).adjoint_synthesis(np.stack([theta, phi], axis=1), v, spin=s)
    print(f"lmax {lmax} s {s}: err {_err(got, want):.3e}")
    assert _err(got, want) < 1e-11


@pytest.mark.parametrize("s", [1, 3, 4, 5])
def test_poles_seam_and_longitude_range(s):
    import heracles_amd as hx

    lmax = 40
    theta = np.array([0.0, np.pi, 1e-9, np.pi - 1e-9, 0.7, 0.7, 2.0, 2.0, np.pi / 2])
    phi = np.array([0.3, 1.0, 0.0, 6.0, 0.0, 2 * np.pi - 1e-12, -1.0, 7.5, 4 * np.pi + 0.25])
    v = np.arange(1.0, 2 * theta.size + 1).reshape(2, -1)
    sht = hx.PointSHT(lmax)
    got = sht.adjoint_synthesis(np.stack([theta, phi], axis=1), v, spin=s)
    want = points2alm_spin(theta, phi, v, lmax, s)
    print(f"poles and seam, s {s}: err {_err(got, want):.3e}")
    assert _err(got, want) < 1e-11
    # a single unit Q at the north pole: (+-s)Y_lm(0, phi) vanishes but for m = -+s, so only m = s is left of m >= 0
    loc = np.array([[0.0, 0.3]])
    one = np.array([[1.0], [0.0]])
    got = sht.adjoint_synthesis(loc, one, spin=s)
    want = points2alm_spin(loc[:, 0], loc[:, 1], one, lmax, s)
    lo = helpers.idx(lmax, s, s)
    others = np.ones(want.shape[1], dtype=bool)
    others[lo : lo + lmax - s + 1] = False
    assert not want[:, others].any() and np.abs(want).max() > 0.1
    assert _err(got, want) < 1e-11


_LONG_CASES = {}
_LONG_STRIDE = 300


def _long_case(lmax, s):
    """The point sets of tests/test_gpu_pointsht.py's test_long_transforms_on_sampled_m (40 points away from the poles; the same with
    three of them at 1e-4, pi - 3e-4 and pi / 2) and their direct-sum alms on every 300th m: computed once per (lmax, s), shared
    by the two spreading paths, never written."""
    if (lmax, s) not in _LONG_CASES:
        rng = np.random.default_rng(10 * lmax + s)
        n = 40
        theta = np.arccos(rng.uniform(-0.995, 0.995, n))
        phi = rng.uniform(0, 2 * np.pi, n)
        v = rng.normal(size=(2, n))
        polar = theta.copy()
        polar[:3] = [1e-4, np.pi - 3e-4, np.pi / 2]
        wants = [points2alm_spin(t, phi, v, lmax, s, orders=range(0, lmax + 1, _LONG_STRIDE)) for t in (theta, polar)]
        for a in (theta, polar, phi, v, *wants):
            a.setflags(write=False)
        _LONG_CASES[lmax, s] = (phi, v, (theta, wants[0]), (polar, wants[1]))
    return _LONG_CASES[lmax, s]


@pytest.mark.parametrize("tiles", [False, True])  # the default spreading path, and the LDS tiles (HX_NUFFT_TILES=1, read on every call)
@pytest.mark.parametrize("lmax", [2100, 4200])  # FFT lengths 16384 and 32768
@pytest.mark.parametrize("s", [1, 3])
def test_long_transforms_on_sampled_m(s, lmax, tiles, monkeypatch):
    """tests/test_gpu_pointsht.py's test of the same name for the run-time-spin sweep, with its bounds and their reasons: 1e-11 away
    from the poles; for the set with points within a few rings of a pole 10 * lmax * 1.1e-16 / sin(first ring), the conditioning of
    a three-term recursion through x = cos(theta) in float64 (the direct sum runs in extended precision)."""
    import heracles_amd as hx

    if tiles:
        monkeypatch.setenv("HX_NUFFT_TILES", "1")
    else:
        monkeypatch.delenv("HX_NUFFT_TILES", raising=False)
    sht = hx.PointSHT(lmax)
    phi, v, away, polar = _long_case(lmax, s)

    def worst_error(theta, want):
        got = sht.adjoint_synthesis(np.stack([theta, phi], axis=1), v, spin=s)
        worst = 0.0
        for m in range(0, lmax + 1, _LONG_STRIDE):
            lo = helpers.idx(lmax, m, m)
            hi = lo + lmax - m + 1
            worst = max(worst, np.abs(got[:, lo:hi] - want[:, lo:hi]).max())
            if m < s:
                assert not got[:, lo : lo + s - m].any()
        return worst / np.abs(want).max()

    e_away, e_polar = worst_error(*away), worst_error(*polar)
    bound = 10 * lmax * 1.1e-16 / np.sin(np.pi / sht.nrings_circle)
    print(f"lmax {lmax} s {s} tiles {tiles}: away {e_away:.3e} (1e-11), polar {e_polar:.3e} ({bound:.3e})")
    assert e_away < 1e-11
    assert e_polar < bound


@pytest.mark.parametrize("lmax", [100, 300])
def test_spin2_through_the_general_sweep(lmax, monkeypatch):
    """HX_SPIN_GENERIC=1 (read on every call) sends s = 2 through the run-time-spin kernel: the new kernel against the oracle."""
    import heracles_amd as hx

    rng = np.random.default_rng(lmax + 2)
    n = 300
    theta, phi = _points(rng, n)
    v = rng.normal(size=(2, n))
    loc = np.stack([theta, phi], axis=1)
    want = oracle.points2alm(theta, phi, v, lmax, spin=2)
    sht = hx.PointSHT(lmax)
    monkeypatch.setenv("HX_SPIN_GENERIC", "1")
    got = sht.adjoint_synthesis(loc, v, spin=2)
    monkeypatch.delenv("HX_SPIN_GENERIC")
    usual = sht.adjoint_synthesis(loc, v, spin=2)
    print(f"lmax {lmax}: general sweep err {_err(got, want):.3e}, spin-2 kernel err {_err(usual, want):.3e}")
    assert _err(got, want) < 1e-11
    assert _err(usual, want) < 1e-11
    assert np.abs(got - usual).max() > 0.0  # (other seeds, other tables: the hook did take the other kernel)


def test_tiled_spreading_path(monkeypatch):
    import heracles_amd as hx

    monkeypatch.setenv("HX_NUFFT_TILES", "1")
    lmax, s = 48, 1
    theta, phi, v, want = _case(lmax, s, 3000)
    got = hx.PointSHT(lmax).adjoint_synthesis(np.stack([theta, phi], axis=1), v, spin=s)
    assert _err(got, want) < 1e-11


def test_three_fields_as_device_tensors():
    import torch
    import heracles_amd as hx

    lmax, s = 24, 1
    theta, phi, v, want = _case(lmax, s, 300, rows=6)
    loc = np.stack([theta, phi], axis=1)
    got = hx.PointSHT(lmax).adjoint_synthesis(torch.as_tensor(loc).cuda(), torch.as_tensor(np.array(v)).cuda(), spin=s)
    assert got.is_cuda and tuple(got.shape) == want.shape
    assert _err(got.cpu().numpy(), want) < 1e-11


def test_alternating_spins_on_one_transform():
    """The tables and task sets of a spin weight are kept per (plan, s): 1 and 3 in turn must not see each other's, and the
    spin-2 result on the same object stays what it was (bit for bit up to the order of the spread's atomics: 1e-13)."""
    import heracles_amd as hx

    lmax = 64
    theta1, phi1, v1, want1 = _case(lmax, 1, 400)
    theta, phi, v, want3 = _case(lmax, 3, 400)
    loc1, loc = np.stack([theta1, phi1], axis=1), np.stack([theta, phi], axis=1)
    sht = hx.PointSHT(lmax)
    before = sht.adjoint_synthesis(loc, v, spin=2)
    for _ in range(2):
        assert _err(sht.adjoint_synthesis(loc1, v1, spin=1), want1) < 1e-11
        assert _err(sht.adjoint_synthesis(loc, v, spin=3), want3) < 1e-11
    after = sht.adjoint_synthesis(loc, v, spin=2)
    assert _err(after, before) < 1e-13
    assert _err(before, oracle.points2alm(theta, phi, v, lmax, spin=2)) < 1e-11


def test_bad_arguments_raise():
    import heracles_amd as hx

    sht = hx.PointSHT(16)
    loc = np.array([[0.5, 1.0], [1.5, 1.0]])
    with pytest.raises(ValueError):
        sht.adjoint_synthesis(loc, np.ones((2, 2)), spin=-1)
    with pytest.raises(ValueError):
        sht.adjoint_synthesis(loc, np.ones((3, 2)), spin=1)
    with pytest.raises(ValueError):
        sht.adjoint_synthesis(loc, np.ones((1, 2)), spin=1)
