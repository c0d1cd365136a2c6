"""GPU parity of the forward point transform (hx_pointsht_synthesis, hx_pointgrid_*: alm -> values at arbitrary points) against
direct sums.

References: spin 0 and 2 -- the oracle, through unit impulses: it is linear, so the alm of a unit value at point p is the conjugate
harmonic table of p and v_p = harmonic_inner(alm, oracle.points2alm(unit impulse at p)); for spin 2 the impulses (e_p, 0) and (0, e_p)
give Q and U.  s >= 1: spin_synthesis_reference.alm2points_spin, in long double.
Tolerance: max |got - want| / max |want| < 1e-11 at epsilon = 1e-12 and < 1e-5 at epsilon = 1e-5, the bounds of
tests/test_gpu_pointsht.py for the adjoint (a numpy model of the construction sits at 2e-14 and 1e-7)."""
import numpy as np
import pytest

import helpers
from oracle import hxoracle as oracle
from spin_synthesis_reference import alm2points_spin, harmonic_inner

pytestmark = pytest.mark.gpu


def _points(rng, n):
    theta = np.arccos(rng.uniform(-1, 1, n))
    phi = rng.uniform(0, 2 * np.pi, n)
    return theta, phi


def _err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def _alm(rng, rows, lmax, spin=0, orders=None):
    """Random alms of real fields: real at m = 0, zero below l = spin; ``orders``: non-zero on those m only."""
    nlm = (lmax + 1) * (lmax + 2) // 2
    a = rng.normal(size=(rows, nlm)) + 1j * rng.normal(size=(rows, nlm))
    a[:, : lmax + 1] = a[:, : lmax + 1].real
    keep = np.zeros(nlm, dtype=bool)
    for m in range(lmax + 1) if orders is None else orders:
        lo = helpers.idx(lmax, m, m)
        keep[lo + max(spin - m, 0) : lo + lmax - m + 1] = True
    a[:, ~keep] = 0.0
    return a


def _impulse_values(theta, phi, alm, lmax, spin, orders=None):
    """Spin 0 / 2 through the oracle's unit impulses, point by point.  ``orders``: the m the alms are non-zero on (the inner product is
    then taken over their rows only)."""
    rows, n = alm.shape[0], theta.size
    sel = slice(None)
    if orders is not None:
        sel = np.concatenate([np.arange(helpers.idx(lmax, m, m), helpers.idx(lmax, m, m) + lmax - m + 1) for m in orders])
    a = alm[:, sel]
    w = np.full(alm.shape[1], 2.0)
    w[: lmax + 1] = 1.0
    w = w[sel]
    out = np.zeros((rows, n))
    for p in range(n):
        t, f = theta[p : p + 1], phi[p : p + 1]
        if spin == 0:
            tab = oracle.points2alm(t, f, np.ones((1, 1)), lmax, spin=0)[:, sel]
            out[:, p] = (w * (a.real * tab.real + a.imag * tab.imag)).sum(axis=1)
        else:
            for comp, impulse in enumerate(([[1.0], [0.0]], [[0.0], [1.0]])):
                tab = oracle.points2alm(t, f, np.array(impulse), lmax, spin=2)[:, sel]
                both = (w * (a.real.reshape(-1, 2, a.shape[1]) * tab.real + a.imag.reshape(-1, 2, a.shape[1]) * tab.imag)).sum(axis=(1, 2))
                out[comp::2, p] = both
    return out


def _direct(theta, phi, alm, lmax, spin, orders=None):
    if spin in (0, 2):
        return _impulse_values(theta, phi, alm, lmax, spin, orders)
    return alm2points_spin(theta, phi, alm, lmax, spin, orders=orders)


_CASES = {}


def _case(lmax, spin, n=500, rows=4, seed=0):
    """Points, alms and the direct sum: computed once, shared, never written."""
    key = (lmax, spin, n, rows, seed)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * lmax + 10 * spin + rows + 7 * seed)
        theta, phi = _points(rng, n)
        alm = _alm(rng, rows, lmax, spin)
        want = _direct(theta, phi, alm, lmax, spin) if spin <= lmax else np.zeros((rows, n))
        for a in (theta, phi, alm, want):
            a.setflags(write=False)
        _CASES[key] = (theta, phi, alm, want)
    return _CASES[key]


def test_impulse_reference_is_the_harmonic_inner_product():
    """The vectorised inner product of _impulse_values is spin_synthesis_reference.harmonic_inner, and at s = 2 the impulses agree
    with the long-double direct sum."""
    lmax = 12
    rng = np.random.default_rng(5)
    theta, phi = _points(rng, 6)
    alm = _alm(rng, 2, lmax, 2)
    got = _impulse_values(theta, phi, alm, lmax, 2)
    for p in range(theta.size):
        tq = oracle.points2alm(theta[p : p + 1], phi[p : p + 1], np.array([[1.0], [0.0]]), lmax, spin=2)
        assert abs(got[0, p] - harmonic_inner(alm, tq, lmax)) < 1e-12
    assert _err(got, alm2points_spin(theta, phi, alm, lmax, 2)) < 1e-12


# ---- 1. random points against the direct sum -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax", [0, 1, 7, 31, 48, 100])  # 31: smallest oversampling (n1 / (2 lmax + 1) = 2.03)
@pytest.mark.parametrize("spin", [0, 2])
def test_random_points_against_direct_sum(lmax, spin):
    import heracles_amd as hx

    theta, phi, alm, want = _case(lmax, spin)
    got = hx.PointSHT(lmax).synthesis(np.stack([theta, phi], axis=1), alm, spin=spin)
    assert got.shape == want.shape == (4, 500) and got.dtype == np.float64
    if spin > lmax:
        assert np.abs(got).max() == 0.0
        return
    print(f"lmax {lmax} spin {spin}: err {_err(got, want):.3e}")
    assert _err(got, want) < 1e-11


@pytest.mark.parametrize("lmax", [0, 1, 2, 3, 7, 31, 100])
@pytest.mark.parametrize("s", [1, 3])
def test_random_points_of_odd_weights(lmax, s):
    import heracles_amd as hx

    theta, phi, alm, want = _case(lmax, s)
    got = hx.PointSHT(lmax).synthesis(np.stack([theta, phi], axis=1), alm, spin=s)
    assert got.shape == want.shape
    if s > lmax:
        assert np.abs(got).max() == 0.0
        return
    print(f"lmax {lmax} s {s}: err {_err(got, want):.3e}")
    assert _err(got, want) < 1e-11


@pytest.mark.parametrize("lmax", [8, 31])
@pytest.mark.parametrize("s", [4, 5, 8])
def test_higher_weights_against_direct_sum(lmax, s):
    import heracles_amd as hx

    theta, phi, alm, want = _case(lmax, s)
    got = hx.PointSHT(lmax).synthesis(np.stack([theta, phi], axis=1), alm, spin=s)
    assert np.abs(want).max() > 0
    print(f"lmax {lmax} s {s}: err {_err(got, want):.3e}")
    assert _err(got, want) < 1e-11


# ---- 2. poles, seam and longitude range ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin", [0, 2, 1, 3])
def test_poles_seam_and_longitude_range(spin):
    """The nine points of tests/test_gpu_pointsht.py's test of the same name."""
    import heracles_amd as hx

    lmax = 40
    theta = np.array([0.0, np.pi, 1e-9, np.pi - 1e-9, 0.7, 0.7, 2.0, 2.0, np.pi / 2])
    phi = np.array([0.3, 1.0, 0.0, 6.0, 0.0, 2 * np.pi - 1e-12, -1.0, 7.5, 4 * np.pi + 0.25])
    alm = _alm(np.random.default_rng(40 + spin), 2, lmax, spin)
    got = hx.PointSHT(lmax).synthesis(np.stack([theta, phi], axis=1), alm, spin=spin)
    want = _direct(theta, phi, alm, lmax, spin)
    print(f"poles and seam, spin {spin}: err {_err(got, want):.3e}")
    assert _err(got, want) < 1e-11


# ---- 3. device adjointness, against the existing adjoint ---------------------------------------------------------------------------
@pytest.mark.parametrize("spin", [0, 2, 3])
def test_adjoint_of_the_adjoint(spin):
    """sum_p v_p S(a)_p = <a, S^+(v)> within 1e-11 of sum_p |v_p S(a)_p|."""
    import heracles_amd as hx

    lmax, n = 48, 500
    rng = np.random.default_rng(300 + spin)
    theta, phi = _points(rng, n)
    loc = np.stack([theta, phi], axis=1)
    a = _alm(rng, 2, lmax, spin)
    v = rng.normal(size=(2, n))
    sht = hx.PointSHT(lmax)
    sa = sht.synthesis(loc, a, spin=spin)
    stv = sht.adjoint_synthesis(loc, v, spin=spin)
    lhs, rhs = float(np.sum(v * sa)), harmonic_inner(a, stv, lmax)
    scale = float(np.sum(np.abs(v * sa)))
    print(f"spin {spin}: <v, S a> - <a, S+ v> = {abs(lhs - rhs):.3e} of {scale:.3e}")
    assert abs(lhs - rhs) < 1e-11 * scale


# ---- 4. batching ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin, rows", [(0, 20), (2, 6), (1, 6)])  # five sweeps of four maps; a sweep of two fields and one of one; three fields
def test_batches_as_device_tensors_with_out(spin, rows):
    import torch
    import heracles_amd as hx

    lmax = 24
    theta, phi, alm, want = _case(lmax, spin, n=300, rows=rows)
    loc = torch.as_tensor(np.stack([theta, phi], axis=1)).cuda()
    sht = hx.PointSHT(lmax)
    got = sht.synthesis(loc, torch.as_tensor(np.array(alm)).cuda(), spin=spin)
    assert got.is_cuda and tuple(got.shape) == want.shape
    assert _err(got.cpu().numpy(), want) < 1e-11
    out = torch.full((rows, 300), np.nan, dtype=torch.float64, device="cuda")
    back = sht.synthesis(loc, torch.as_tensor(np.array(alm)).cuda(), spin=spin, out=out)
    assert back is out and torch.equal(out, got)
    host = np.empty((rows, 300))
    assert sht.synthesis(np.stack([theta, phi], axis=1), alm, spin=spin, out=host) is host
    assert np.array_equal(host, got.cpu().numpy())


# ---- 5. gather paths -----------------------------------------------------------------------------------------------------------------
def test_gather_paths_agree_and_repeat(monkeypatch):
    import heracles_amd as hx

    lmax = 100
    theta, phi, alm, want = _case(lmax, 0)
    loc = np.stack([theta, phi], axis=1)
    sht = hx.PointSHT(lmax)
    res = {}
    for tiles in ("1", "0"):
        monkeypatch.setenv("HX_NUFFT_TILES", tiles)
        res[tiles] = sht.synthesis(loc, alm)
        assert np.array_equal(res[tiles], sht.synthesis(loc, alm))
        assert _err(res[tiles], want) < 1e-11
    print(f"tiles against one thread per point: {_err(res['1'], res['0']):.3e}, bit for bit: {np.array_equal(res['1'], res['0'])}")
    assert _err(res["1"], res["0"]) < 1e-13
    assert np.array_equal(res["1"], res["0"])  # (more than asked: every path forms a point's sums in the same order, with fma spelled out)


@pytest.mark.parametrize("lmax", [5, 300])  # a grid smaller than one 64-cell tile, and many tiles
def test_tiled_gather_on_small_and_large_grids(lmax, monkeypatch):
    import heracles_amd as hx

    monkeypatch.setenv("HX_NUFFT_TILES", "1")
    theta, phi, alm, want = _case(lmax, 2, n=300, rows=2)
    theta = np.array(theta)
    theta[:4] = [0.0, np.pi, 1e-7, np.pi - 1e-7]
    want = _direct(theta, phi, alm, lmax, 2)
    got = hx.PointSHT(lmax).synthesis(np.stack([theta, phi], axis=1), alm, spin=2)
    print(f"tiles, lmax {lmax}: err {_err(got, want):.3e}")
    assert _err(got, want) < 1e-11


# ---- 6. long transforms --------------------------------------------------------------------------------------------------------------
_LONG_CASES = {}
_LONG_STRIDE = 97


def _long_case(lmax):
    """40 points, three of them at 1e-4, pi - 3e-4 and pi / 2; alms on every 97th order; the direct sums for spin 2 (oracle impulses
    with set_mstride(97)) and s = 1 (alm2points_spin(orders=...)): computed once per lmax, shared by the two gather paths, never
    written."""
    if lmax not in _LONG_CASES:
        rng = np.random.default_rng(lmax)
        n = 40
        theta = np.arccos(rng.uniform(-0.995, 0.995, n))
        phi = rng.uniform(0, 2 * np.pi, n)
        theta[:3] = [1e-4, np.pi - 3e-4, np.pi / 2]
        orders = range(0, lmax + 1, _LONG_STRIDE)
        alm2, alm1 = _alm(rng, 2, lmax, 2, orders), _alm(rng, 2, lmax, 1, orders)
        oracle.set_mstride(_LONG_STRIDE)
        try:
            want2 = _impulse_values(theta, phi, alm2, lmax, 2, orders)
        finally:
            oracle.set_mstride(1)
        want1 = alm2points_spin(theta, phi, alm1, lmax, 1, orders=orders)
        for a in (theta, phi, alm2, alm1, want2, want1):
            a.setflags(write=False)
        _LONG_CASES[lmax] = (theta, phi, {2: (alm2, want2), 1: (alm1, want1)})
    return _LONG_CASES[lmax]


@pytest.mark.parametrize("tiles", [False, True])
@pytest.mark.parametrize("lmax", [2100, 4200])  # FFT lengths 16384 / 32768: the split above 8192
def test_long_transforms_on_sampled_m(lmax, tiles, monkeypatch):
    """Bound: 1e-11 on all 40 points, as for every case of this file.  The two points next to the poles read the modes of the rings next
    to a pole, where the Legendre sweeps' recursion through x = cos(theta) in float64 carries l * 1.1e-16 / sin(theta_ring): with the
    sweeps' modes alone they sat at 3.9e-11 at lmax 4200 (8.8e-12 at 2100) while every other point was at 8e-13.  k_polar_modes forms
    those rings' modes again from double-double Wigner-d tables; measured with it on the MI355X: 5.3e-12 (spin 2) and 4.5e-13 (s = 1)
    at lmax 4200, 3.9e-13 and 3.2e-13 at 2100."""
    import heracles_amd as hx

    if tiles:
        monkeypatch.setenv("HX_NUFFT_TILES", "1")
    else:
        monkeypatch.delenv("HX_NUFFT_TILES", raising=False)
    theta, phi, by_spin = _long_case(lmax)
    loc = np.stack([theta, phi], axis=1)
    sht = hx.PointSHT(lmax)
    errs = {}
    for spin, (alm, want) in by_spin.items():
        got = sht.synthesis(loc, alm, spin=spin)
        errs[spin] = _err(got, want)
        per_point = np.abs(got - want).max(axis=0) / np.abs(want).max()
        print(f"lmax {lmax} tiles {tiles} spin {spin}: err {errs[spin]:.3e}; the two polar points {per_point[:2].max():.3e}, the other 38 {per_point[2:].max():.3e}")
    assert errs[2] < 1e-11
    assert errs[1] < 1e-11


# ---- 7. pixel centres ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin", [0, 2])
def test_pixel_centres_reproduce_alm2map(spin):
    import heracles_amd as hx

    nside, lmax = 32, 64
    alm = _alm(np.random.default_rng(11 + spin), 2, lmax, spin)
    theta, phi = oracle.pix2ang(nside)
    want = np.asarray(hx.get_plan(nside, lmax).alm2map(alm, spin))
    got = hx.PointSHT(lmax).synthesis(np.stack([theta, phi], axis=1), alm, spin=spin)
    assert _err(got, want) < 1e-11


# ---- 8. PointField -------------------------------------------------------------------------------------------------------------------
def test_point_field_pages_and_interleaved_adjoint():
    import heracles_amd as hx

    lmax = 48
    theta, phi, alm, want = _case(lmax, 2)
    loc = np.stack([theta, phi], axis=1)
    sht = hx.PointSHT(lmax)
    one_shot = sht.synthesis(loc, alm, spin=2)
    field = sht.field(alm, spin=2)
    assert isinstance(field, hx.PointField)
    assert np.array_equal(field.at(loc), one_shot)
    first = field.at(loc[:123])
    sht.adjoint_synthesis(loc, np.ones((2, 500)), spin=2)  # the object's own grid and FFT scratch are used in between
    second = field.at(loc[123:])
    assert np.array_equal(np.concatenate([first, second], axis=1), one_shot)
    assert field.at(loc[:0]).shape == (4, 0)
    with pytest.raises(ValueError):
        field.at(np.array([[-0.1, 0.0]]))
    assert np.array_equal(field.at(loc), one_shot)
    field.close()
    field.close()
    with pytest.raises(ValueError):
        field.at(loc)


def test_point_field_on_device_tensors():
    import torch
    import heracles_amd as hx

    lmax = 24
    theta, phi, alm, want = _case(lmax, 0, n=300, rows=20)
    loc = torch.as_tensor(np.stack([theta, phi], axis=1)).cuda()
    field = hx.PointSHT(lmax).field(torch.as_tensor(np.array(alm)).cuda())
    got = field.at(loc)
    assert got.is_cuda and _err(got.cpu().numpy(), want) < 1e-11
    out = torch.empty_like(got)
    assert field.at(loc, out=out) is out and torch.equal(out, got)


# ---- 9. interleaving on one object ---------------------------------------------------------------------------------------------------
def test_interleaved_directions_and_spins_on_one_object():
    import heracles_amd as hx

    lmax = 64
    theta, phi, alm0, want0 = _case(lmax, 0, n=400)
    theta3, phi3, alm3, want3 = _case(lmax, 3, n=400)  # (other points: each case has its own)
    loc0, loc3 = np.stack([theta, phi], axis=1), np.stack([theta3, phi3], axis=1)
    v = np.random.default_rng(9).normal(size=(2, 400))
    sht = hx.PointSHT(lmax)
    first = sht.synthesis(loc0, alm0)
    adj = sht.adjoint_synthesis(loc0, v, spin=2)
    other = sht.synthesis(loc3, alm3, spin=3)
    last = sht.synthesis(loc0, alm0)
    assert np.array_equal(first, last)
    assert _err(first, want0) < 1e-11 and _err(other, want3) < 1e-11
    fresh = hx.PointSHT(lmax).adjoint_synthesis(loc0, v, spin=2)
    assert _err(adj, fresh) < 1e-13


# ---- 10. HX_SPIN_GENERIC=1 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax", [100, 300])
def test_spin2_through_the_general_sweep(lmax, monkeypatch):
    import heracles_amd as hx

    theta, phi, alm, want = _case(lmax, 2, n=300, rows=2)
    loc = np.stack([theta, phi], axis=1)
    sht = hx.PointSHT(lmax)
    monkeypatch.setenv("HX_SPIN_GENERIC", "1")
    got = sht.synthesis(loc, alm, spin=2)
    monkeypatch.delenv("HX_SPIN_GENERIC")
    usual = sht.synthesis(loc, alm, spin=2)
    print(f"lmax {lmax}: general sweep err {_err(got, want):.3e}, spin-2 kernel err {_err(usual, want):.3e}")
    assert _err(got, want) < 1e-11
    assert _err(usual, want) < 1e-11
    assert _err(got, usual) < 1e-11
    assert np.abs(got - usual).max() > 0.0  # (other seeds, other tables: the hook did take the other kernel)


# ---- 11. epsilon = 1e-5 --------------------------------------------------------------------------------------------------------------
def test_float32_accuracy_class():
    import heracles_amd as hx

    lmax = 64
    theta, phi, alm, want = _case(lmax, 0, n=400, rows=1)
    sht = hx.PointSHT(lmax, epsilon=1e-5)
    assert sht.kernel_width < hx.PointSHT(lmax).kernel_width
    got = sht.synthesis(np.stack([theta, phi], axis=1), alm)
    print(f"epsilon 1e-5: err {_err(got, want):.3e}")
    assert _err(got, want) < 1e-5


# ---- 12. arguments -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_leave_the_object_usable():
    import heracles_amd as hx

    lmax = 16
    theta, phi, alm, want = _case(lmax, 0, n=50, rows=2)
    loc = np.stack([theta, phi], axis=1)
    sht = hx.PointSHT(lmax)

    def good():
        assert _err(sht.synthesis(loc, alm), want) < 1e-11

    good()
    for bad_theta in (-0.1, np.pi + 1e-3):
        bad = loc.copy()
        bad[7, 0] = bad_theta
        with pytest.raises(ValueError):
            sht.synthesis(bad, alm)
        good()
    bad = loc.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        sht.synthesis(bad, alm)
    good()
    with pytest.raises(ValueError):
        sht.synthesis(loc, alm, spin=-1)
    good()
    with pytest.raises(ValueError):
        sht.synthesis(loc, alm[:1], spin=1)
    good()
    with pytest.raises(ValueError):
        sht.synthesis(loc, alm[:, :-1])
    good()
    with pytest.raises(ValueError):
        sht.synthesis(loc.T, alm)
    good()
    empty = sht.synthesis(loc[:0], alm)
    assert empty.shape == (2, 0)
    good()


# ---- 13. HipDiscreteMapper.sample ----------------------------------------------------------------------------------------------------
def test_discrete_mapper_sample():
    import heracles_amd as hx
    from heracles_amd import HipDiscreteMapper

    rng = np.random.default_rng(21)
    lmax, n = 30, 200
    lon = rng.uniform(-180, 540, n)
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, n)))
    loc = np.stack([np.radians(90 - lat), np.radians(lon % 360)], axis=1)
    mapper = HipDiscreteMapper(lmax)
    alm = _alm(rng, 2, lmax, 2)
    got = mapper.sample(lon, lat, alm, spin=2)
    assert np.array_equal(got, hx.get_point_sht(lmax).synthesis(loc, alm, spin=2))
    one = mapper.sample(lon, lat, alm[0])
    assert one.shape == (n,)
    assert np.array_equal(one, hx.get_point_sht(lmax).synthesis(loc, alm[:1])[0])
    single = mapper.sample(lon, lat, alm.astype(np.complex64), spin=2)
    assert np.array_equal(single, hx.get_point_sht(lmax, 1e-5).synthesis(loc, alm.astype(np.complex64), spin=2))
    assert 1e-14 < _err(single, got) < 1e-5
    with pytest.raises(ValueError):
        mapper.sample(lon, lat, alm[:, :-1])
