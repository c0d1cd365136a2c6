"""GPU parity of HEALPix map2alm / alm2map for fields of a spin weight other than 0 and 2 (the run-time-spin sweeps of
hx_legendre_valu.hip) against the long-double direct sums of tests/spin_reference.py and tests/spin_synthesis_reference.py
(themselves tied to helpers.sYlm and to the oracle by tests/test_spin_reference.py and tests/test_spin_synthesis_reference.py).
Tolerance against a direct sum: 1e-11 of the largest value, the yardstick of tests/test_gpu_pointsht_spin.py and of
tests/test_gpu_sht.py for the same sweeps at spin 2."""
import ctypes

import numpy as np
import pytest

import helpers
from oracle import hxoracle as oracle
from healpix_pixels import special_pixels as _special_pixels
from spin_reference import points2alm_spin
from spin_synthesis_reference import alm2points_spin, harmonic_inner

pytestmark = pytest.mark.gpu
TOL = 1e-11


def _err(got, want):
    return np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(want).max()


def plan_nlm(lmax):
    return (lmax + 1) * (lmax + 2) // 2


def _low_rows_are_zero(alm, lmax, s):
    for m in range(min(s, lmax + 1)):
        i = helpers.idx(lmax, m, m)
        if alm[..., i : i + min(s, lmax + 1) - m].any():
            return False
    return True


def _ring_of_pixels(nside):
    """Ring index (0 .. 4 nside - 2, north to south) of every pixel, and the first pixel of every ring."""
    theta, _ = oracle.pix2ang(nside)
    start = np.concatenate([[0], np.flatnonzero(np.diff(theta) > 0) + 1])
    assert start.size == 4 * nside - 1
    ring = np.searchsorted(start, np.arange(theta.size), side="right") - 1
    return ring, start


_CASES = {}


def _analysis_case(nside, lmax, s, sparse=False):
    """(Q, U) maps and their direct-sum alms with unit weights: computed once, shared, never written."""
    key = ("a", nside, lmax, s, sparse)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * nside + 10 * lmax + s)
        npix = 12 * nside * nside
        theta, phi = oracle.pix2ang(nside)
        maps = rng.standard_normal((2, npix))
        pix = _special_pixels(nside, rng) if sparse else np.arange(npix)
        if sparse:
            full = maps
            maps = np.zeros_like(full)
            maps[:, pix] = full[:, pix]
        want = points2alm_spin(theta[pix], phi[pix], maps[:, pix] * (4 * np.pi / npix), lmax, s)
        for a in (maps, want):
            a.setflags(write=False)
        _CASES[key] = (maps, want)
    return _CASES[key]


def _synthesis_case(nside, lmax, s):
    """(E, B) alms with zeros below l = s, sampled pixels and the direct-sum (Q, U) there."""
    key = ("s", nside, lmax, s)
    if key not in _CASES:
        rng = np.random.default_rng(77 * nside + 3 * lmax + s)
        alm = helpers.random_alm(rng, lmax, s, (2,))
        pix = _special_pixels(nside, rng)
        theta, phi = oracle.pix2ang(nside)
        want = alm2points_spin(theta[pix], phi[pix], alm, lmax, s)
        for a in (alm, pix, want):
            a.setflags(write=False)
        _CASES[key] = (alm, pix, want)
    return _CASES[key]


# ---- 1. map2alm against the direct sum ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside,lmax", [(1, 2), (2, 5), (4, 8), (8, 23), (12, 20), (16, 24)])
@pytest.mark.parametrize("s", [1, 3])
def test_map2alm_against_direct_sum(nside, lmax, s):
    import heracles_amd as hx

    maps, want = _analysis_case(nside, lmax, s)
    plan = hx.Plan(nside, lmax)
    got = plan.map2alm(maps, s)
    if s > lmax:  # no l >= s below the band limit: zero alms, zero maps, and iterations whose residual is the map itself
        again = plan.map2alm(maps, s, niter=2)
        back = plan.alm2map(np.ones((2, plan.nlm), dtype=complex), s)
        plan.close()
        assert got.shape == want.shape and not got.any() and not want.any()
        assert not again.any() and back.shape == maps.shape and not back.any()
        return
    plan.close()
    assert got.shape == want.shape
    print(f"nside {nside} lmax {lmax} s {s}: err {_err(got, want):.3e}")
    assert _err(got, want) < TOL
    assert _low_rows_are_zero(got, lmax, s)


# weights with more than three orders m < s (the m < s seeds of spin_seeds, chains from l0 = s > m), even and odd; (8, 8) with
# s = 8: s = lmax, one row per order
@pytest.mark.parametrize("nside,lmax,s", [(n, l, s) for s in (4, 5, 8) for n, l in ((4, 8), (8, 23), (16, 24))] + [(8, 8, 8)])
def test_map2alm_higher_weights_against_direct_sum(nside, lmax, s):
    import heracles_amd as hx

    maps, want = _analysis_case(nside, lmax, s)
    plan = hx.Plan(nside, lmax)
    got = plan.map2alm(maps, s)
    plan.close()
    assert got.shape == want.shape and np.abs(want).max() > 0
    print(f"nside {nside} lmax {lmax} s {s}: err {_err(got, want):.3e}")
    assert _err(got, want) < TOL
    assert _low_rows_are_zero(got, lmax, s)


# ---- 2. scaled chains and ring pruning ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 3, 8])
def test_map2alm_scaled_chains_and_pruning(s):
    """nside 128 / lmax 200: sin^m(theta) underflows on the polar rings and ring_mlim(lmax, s) prunes (it depends on s); a map that is
    non-zero in at most 400 pixels (poles, cap / belt boundary, shifted and unshifted belt rings, equator, ring ends) keeps the direct sum cheap."""
    import heracles_amd as hx

    nside, lmax = 128, 200
    maps, want = _analysis_case(nside, lmax, s, sparse=True)
    assert 0 < np.count_nonzero(maps[0]) <= 400
    got = hx.get_plan(nside, lmax).map2alm(maps, s)
    print(f"nside {nside} lmax {lmax} s {s}: err {_err(got, want):.3e}")
    assert _err(got, want) < TOL
    assert _low_rows_are_zero(got, lmax, s)


# ---- 3. the two front ends agree ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 3, 4])
def test_pixel_centres_reproduce_map2alm(s):
    """A HEALPix map is a set of points of weight 4 pi / npix: the HEALPix route and the point transform must agree."""
    import heracles_amd as hx

    nside, lmax = 32, 64
    npix = 12 * nside * nside
    rng = np.random.default_rng(11 + s)
    maps = rng.normal(size=(2, npix))
    theta, phi = oracle.pix2ang(nside)
    got = hx.get_plan(nside, lmax).map2alm(maps, s)
    want = hx.PointSHT(lmax).adjoint_synthesis(np.stack([theta, phi], axis=1), maps * (4 * np.pi / npix), spin=s)
    print(f"s {s}: err {_err(got, want):.3e}")
    assert _err(got, np.asarray(want)) < TOL


# ---- 4. alm2map against the direct sum ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside,lmax", [(4, 8), (8, 20), (12, 20), (32, 48), (128, 200)])
@pytest.mark.parametrize("s", [1, 3])
def test_alm2map_against_direct_sum(nside, lmax, s):
    import heracles_amd as hx

    alm, pix, want = _synthesis_case(nside, lmax, s)
    got = hx.get_plan(nside, lmax).alm2map(alm, s)
    assert got.shape == (2, 12 * nside * nside)
    err = np.abs(got[:, pix] - want).max() / np.abs(want).max()
    print(f"nside {nside} lmax {lmax} s {s}: err {err:.3e} at {pix.size} pixels")
    assert err < TOL


@pytest.mark.parametrize("nside,lmax", [(8, 20), (32, 48), (128, 200)])
@pytest.mark.parametrize("s", [4, 5, 8])
def test_alm2map_higher_weights_against_direct_sum(nside, lmax, s):
    import heracles_amd as hx

    alm, pix, want = _synthesis_case(nside, lmax, s)
    got = hx.get_plan(nside, lmax).alm2map(alm, s)
    assert got.shape == (2, 12 * nside * nside) and np.abs(want).max() > 0
    err = np.abs(got[:, pix] - want).max() / np.abs(want).max()
    print(f"nside {nside} lmax {lmax} s {s}: err {err:.3e} at {pix.size} pixels")
    assert err < TOL


# ---- 5. adjointness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside,lmax", [(16, 24), (64, 100)])
def test_adjointness(nside, lmax):
    """With unit weights map2alm is (4 pi / npix) x the adjoint of alm2map in the inner product that counts the orders m > 0 twice:

        sum_p (Q_p Q'_p + U_p U'_p) = (npix / 4 pi) sum_{l, all m} Re(E conj(E') + B conj(B'))

    for (E, B) = map2alm(Q, U) and (Q', U') = alm2map(E', B').  Both sides are sums of the same products.  Bound: each transform
    is within 1e-11 of its largest value in every entry (the yardstick above), so with d(Q', U') and d(E, B) those errors
        |lhs - rhs| <= |(Q, U)| |d(Q', U')| + (npix / 4 pi) |d(E, B)| |(E', B')|
                    <= 1e-11 (|(Q, U)| sqrt(2 npix) max|(Q', U')| + (npix / 4 pi) sqrt(2 nall) max|(E, B)| |(E', B')|),
    2-norms over pixels / over all m; nall = 2 (lmax + 1)^2 entries of (E, B) over all m.  Spin 2 on its own kernels goes first, so that
    the test is known to be right before it judges the run-time-spin sweeps."""
    import heracles_amd as hx

    npix = 12 * nside * nside
    plan = hx.get_plan(nside, lmax)
    for s in (2, 1, 3, 4, 5):
        rng = np.random.default_rng(5 * nside + s)
        maps = rng.standard_normal((2, npix))
        alm2 = helpers.random_alm(rng, lmax, s, (2,))
        alm = plan.map2alm(maps, s)
        maps2 = plan.alm2map(alm2, s)
        lhs = float(np.sum(maps * maps2))
        rhs = npix / (4 * np.pi) * harmonic_inner(alm, alm2, lmax)
        bound = 1e-11 * (np.sqrt(np.sum(maps**2)) * np.sqrt(2 * npix) * np.abs(maps2).max()
                         + npix / (4 * np.pi) * np.sqrt(2 * 2 * (lmax + 1) ** 2) * np.abs(alm).max()
                         * np.sqrt(harmonic_inner(alm2, alm2, lmax)))
        print(f"nside {nside} lmax {lmax} s {s}: lhs {lhs:.15e} rhs {rhs:.15e} diff {abs(lhs - rhs):.3e} bound {bound:.3e}")
        assert abs(lhs - rhs) < bound, s


# ---- 6. spin 2 through the run-time-spin sweeps ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nside,lmax", [(32, 64), (128, 200)])
def test_spin2_through_the_general_sweeps(nside, lmax, monkeypatch):
    """HX_SPIN_GENERIC=1 (read on every call) sends s = 2 through the run-time-spin kernels, analysis and synthesis.  The two paths
    differ in the rounding of seeds and tables only (2.7e-14 in the point transform): 1e-12 of the largest value.  Without the
    variable the spin-2 results are bit for bit what they were."""
    import heracles_amd as hx

    rng = np.random.default_rng(nside + lmax)
    maps = rng.standard_normal((2, 12 * nside * nside))
    alm = helpers.random_alm(rng, lmax, 2, (2,))
    plan = hx.get_plan(nside, lmax)
    a_before, m_before = plan.map2alm(maps, 2), plan.alm2map(alm, 2)
    monkeypatch.setenv("HX_SPIN_GENERIC", "1")
    a_gen, m_gen = plan.map2alm(maps, 2), plan.alm2map(alm, 2)
    monkeypatch.delenv("HX_SPIN_GENERIC")
    a_after, m_after = plan.map2alm(maps, 2), plan.alm2map(alm, 2)
    print(f"nside {nside} lmax {lmax}: map2alm {_err(a_gen, a_before):.3e} alm2map {_err(m_gen, m_before):.3e}")
    assert _err(a_gen, a_before) < 1e-12
    assert _err(m_gen, m_before) < 1e-12
    assert np.abs(a_gen - a_before).max() > 0.0 and np.abs(m_gen - m_before).max() > 0.0  # (the hook did take the other kernels)
    assert np.array_equal(a_after, a_before) and np.array_equal(m_after, m_before)


# ---- 6b. the run-time-spin sweep in m-chunks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 3])
def test_map2alm_m_chunked(s):
    """tests/test_gpu_sht.py's test_map2alm_m_chunked_batches_medium for the run-time-spin sweep: nside 256 / lmax 511 with the scratch
    budget lowered through hx_set_scratch_budget, so that the sweep is cut into m-chunks [m0, m1) whose rows of partial sums start at
    rows_before_m[m0] != 0, without and with one Jacobi iteration (whose second analysis ADDS into the alms: add = 1 in
    k_alm_reduce_spin).  The chunking must not change a bit, and the chunked alms are the direct sum of the map (at most 400 non-zero
    pixels, resident on the device) on every 16th m."""
    import torch
    import heracles_amd as hx

    nside, lmax = 256, 511
    npix = 12 * nside * nside
    rng = np.random.default_rng(2560 + s)
    pix = _special_pixels(nside, rng)
    vals = rng.standard_normal((2, pix.size))
    assert 0 < pix.size <= 400
    dev = torch.zeros((2, npix), dtype=torch.float64, device="cuda")
    dev[:, torch.as_tensor(pix).cuda()] = torch.as_tensor(vals).cuda()
    plan = hx.get_plan(nside, lmax)
    whole = plan.map2alm(dev, s).cpu().numpy()
    assert plan.last_chunks == 1
    whole1 = plan.map2alm(dev, s, niter=1).cpu().numpy()
    assert plan.last_chunks == 1
    hx._lib.set_scratch_budget(2.0e6)
    try:
        out = plan.map2alm(dev, s).cpu().numpy()
        nchunks = plan.last_chunks
        out1 = plan.map2alm(dev, s, niter=1).cpu().numpy()
        nchunks1 = plan.last_chunks
    finally:
        hx._lib.set_scratch_budget(0)
    print(f"nside {nside} lmax {lmax} s {s}: {nchunks} m-chunks, {nchunks1} with niter 1")
    assert nchunks >= 3 and nchunks1 >= 3, (nchunks, nchunks1)
    np.testing.assert_array_equal(out, whole)  # the chunking does not change a bit
    np.testing.assert_array_equal(out1, whole1)
    assert np.abs(out1 - out).max() > 0  # (the iteration did add something)
    orders = range(0, lmax + 1, 16)
    theta, phi = oracle.pix2ang(nside)
    want = points2alm_spin(theta[pix], phi[pix], vals * (4 * np.pi / npix), lmax, s, orders=orders)
    scale = np.abs(want).max()
    worst = 0.0
    for m in orders:
        lo = helpers.idx(lmax, m, m)
        worst = max(worst, np.abs(out[:, lo : lo + lmax - m + 1] - want[:, lo : lo + lmax - m + 1]).max())
    print(f"nside {nside} lmax {lmax} s {s}: err {worst / scale:.3e} on every 16th m")
    assert worst < TOL * scale
    assert _low_rows_are_zero(out, lmax, s) and _low_rows_are_zero(out1, lmax, s)


# ---- 7. iterations, weights, filter -----------------------------------------------------------------------------------------------
def test_iterations_weights_filter():
    import heracles_amd as hx

    nside, lmax, s = 16, 24, 1
    npix = 12 * nside * nside
    maps, want = _analysis_case(nside, lmax, s)
    plan = hx.get_plan(nside, lmax)
    # the Jacobi loop written out (tolerance of tests/test_gpu_sht.py for iterated transforms)
    a = plan.map2alm(maps, s)
    for _ in range(2):
        a = a + plan.map2alm(maps - plan.alm2map(a, s), s)
    got = plan.map2alm(maps, s, niter=2)
    print(f"niter 2 against the loop: {_err(got, a):.3e}")
    assert _err(got, a) < 1e-10
    # ring weights (per ring pair, north ring 1 .. 2 nside) and pixel weights: the direct sum of the weighted values
    rng = np.random.default_rng(17)
    rw = rng.uniform(0.9, 1.1, 2 * nside)
    pw = rng.uniform(0.9, 1.1, npix)
    theta, phi = oracle.pix2ang(nside)
    ring, _ = _ring_of_pixels(nside)
    rw_pix = rw[np.minimum(ring, 4 * nside - 2 - ring)]
    for kw, w in (({"ring_weights": rw}, rw_pix), ({"pix_weights": pw}, pw), ({"ring_weights": rw, "pix_weights": pw}, rw_pix * pw)):
        ref = points2alm_spin(theta, phi, maps * w * (4 * np.pi / npix), lmax, s)
        got = plan.map2alm(maps, s, **kw)
        print(f"{sorted(kw)}: err {_err(got, ref):.3e}")
        assert _err(got, ref) < TOL
    # fl multiplies row l
    fl = rng.uniform(0.5, 1.5, lmax + 1)
    plain, got = plan.map2alm(maps, s), plan.map2alm(maps, s, fl=fl)
    got2 = plan.map2alm(maps, s, fl=fl, niter=2)
    for m in range(lmax + 1):
        i = helpers.idx(lmax, m, m)
        assert _err(got[:, i + max(s - m, 0) : i + lmax - m + 1], (plain[:, i : i + lmax - m + 1] * fl[m:])[:, max(s - m, 0) :]) < 1e-14
        assert np.abs(got2[:, i : i + lmax - m + 1] - a[:, i : i + lmax - m + 1] * fl[m:]).max() < 1e-10 * np.abs(a).max()
    # a band-limited map (made by the new alm2map) gets closer to its alms with iterations
    alm = helpers.random_alm(rng, lmax, s, (2,))
    band = plan.alm2map(alm, s)
    e0, e3 = _err(plan.map2alm(band, s), alm), _err(plan.map2alm(band, s, niter=3), alm)
    print(f"band-limited map: niter 0 err {e0:.3e}, niter 3 err {e3:.3e}")
    assert e3 < e0


# ---- 8. plumbing ------------------------------------------------------------------------------------------------------------------
def test_three_fields_numpy_and_device_tensors():
    import torch
    import heracles_amd as hx

    nside, lmax, s = 16, 24, 1
    rng = np.random.default_rng(23)
    maps = rng.standard_normal((3, 2, 12 * nside * nside))
    alm = helpers.random_alm(rng, lmax, s, (3, 2))
    plan = hx.get_plan(nside, lmax)
    for niter in (0, 2):
        each = np.stack([plan.map2alm(maps[f], s, niter=niter) for f in range(3)])
        got = plan.map2alm(maps, s, niter=niter)
        assert got.shape == (3, 2, plan.nlm) and _err(got, each) < 1e-13  # (the ring stage takes the six components at once)
        dev = plan.map2alm(torch.as_tensor(maps).cuda(), s, niter=niter)
        assert dev.is_cuda and tuple(dev.shape) == (3, 2, plan.nlm)
        assert np.array_equal(dev.cpu().numpy(), got)
    each = np.stack([plan.alm2map(alm[f], s) for f in range(3)])
    assert _err(plan.alm2map(alm, s), each) < 1e-13
    dev = plan.alm2map(torch.as_tensor(alm).cuda(), s)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), plan.alm2map(alm, s))


def test_alternating_spins_on_one_plan():
    """The tables and task sets of a weight are kept per (plan, s): 1, 3, 1 in turn must not see each other's."""
    import heracles_amd as hx

    nside, lmax = 16, 24
    plan = hx.Plan(nside, lmax)
    for s in (1, 3, 1, 3):
        maps, want = _analysis_case(nside, lmax, s)
        assert _err(plan.map2alm(maps, s), want) < TOL
        alm, pix, vals = _synthesis_case(12, 20, s)  # (another plan in between)
        assert np.abs(hx.get_plan(12, 20).alm2map(alm, s)[:, pix] - vals).max() < TOL * np.abs(vals).max()
    plan.close()


def test_mapper_transform_metadata_and_device_array():
    import torch
    import heracles_amd as hx

    nside, lmax, s = 16, 24, 1
    maps, want = _analysis_case(nside, lmax, s)
    mapper = hx.HipHealpixMapper(nside, lmax, deconvolve=False, niter=0, ring_weights=np.ones(2 * nside))
    data = mapper.create(2, spin=s)
    data[...] = maps
    alm = mapper.transform(data, spin=s)
    assert isinstance(alm, np.ndarray) and _err(alm, want) < TOL
    assert alm.dtype.metadata == {**data.dtype.metadata, "deconv": False} and alm.dtype.metadata["spin"] == s
    dev = mapper.transform(hx.DeviceArray(torch.as_tensor(np.array(maps)).cuda(), data.dtype.metadata), spin=s)
    assert isinstance(dev, hx.DeviceArray) and dev.tensor.is_cuda
    assert dict(dev.dtype.metadata) == dict(alm.dtype.metadata)
    assert np.array_equal(dev.tensor.cpu().numpy(), np.asarray(alm))
    ten = mapper.transform(torch.as_tensor(np.array(maps)).cuda(), spin=s)
    assert ten.is_cuda and np.array_equal(ten.cpu().numpy(), np.asarray(alm))
    # the default three iterations run (the synthesis exists)
    it = hx.HipHealpixMapper(nside, lmax, deconvolve=False, ring_weights=np.ones(2 * nside)).transform(data, spin=s)
    assert _err(it, hx.get_plan(nside, lmax).map2alm(maps, s, niter=3)) < 1e-14


@pytest.mark.parametrize("device", [None, "cuda"])
def test_transform_many_mixed_spins(device):
    import heracles_amd as hx

    nside, lmax = 16, 24
    npix = 12 * nside * nside
    rng = np.random.default_rng(31)
    mapper = hx.HipHealpixMapper(nside, lmax, deconvolve=False, niter=0, ring_weights=np.ones(2 * nside))
    spins = [0, 1, 2, 3]
    maps = []
    for sp in spins:
        m = mapper.create(*(() if sp == 0 else (2,)), spin=sp)
        m[...] = rng.standard_normal(m.shape)
        maps.append(m)
    kw = {} if device is None else {"device": device}
    got = mapper.transform_many(maps, spins, **kw)
    only02 = mapper.transform_many([maps[0], maps[2]], [0, 2], **kw)
    host = lambda a: a.tensor.cpu().numpy() if isinstance(a, hx.DeviceArray) else np.asarray(a)
    assert len(got) == 4
    for a, sp in zip(got, spins):
        assert isinstance(a, hx.DeviceArray if device else np.ndarray)
        assert a.dtype.metadata["spin"] == sp and a.dtype.metadata["deconv"] is False
        assert a.shape == ((plan_nlm(lmax),) if sp == 0 else (2, plan_nlm(lmax)))
    assert np.array_equal(host(got[0]), host(only02[0])) and np.array_equal(host(got[2]), host(only02[1]))
    theta, phi = oracle.pix2ang(nside)
    for k in (1, 3):
        ref = points2alm_spin(theta, phi, np.asarray(maps[k]) * (4 * np.pi / npix), lmax, spins[k])
        assert _err(host(got[k]), ref) < TOL


def test_map_catalogs_then_transform_for_a_spin1_field():
    import heracles_amd as hx

    class Deflection(hx.ComplexField, spin=1):
        pass

    nside, lmax, n = 16, 24, 4000
    npix = 12 * nside * nside
    rng = np.random.default_rng(41)
    c = {"lon": rng.uniform(0, 360, n), "lat": np.degrees(np.arcsin(rng.uniform(-1, 1, n))),
         "w": rng.uniform(0.5, 1.5, n), "g1": rng.normal(0, 0.3, n), "g2": rng.normal(0, 0.3, n)}
    mapper = hx.HipHealpixMapper(nside, lmax, deconvolve=False, niter=0, ring_weights=np.ones(2 * nside))
    fields = {"D": Deflection(mapper, "lon", "lat", "g1", "g2", "w")}
    maps = hx.map_catalogs(fields, {0: hx.ArrayCatalog(c, page_size=2500)})
    m = maps["D", 0]
    assert m.shape == (2, npix) and m.dtype.metadata["spin"] == 1 and np.count_nonzero(np.asarray(m)[0]) > 1000
    alms = hx.transform(fields, maps)
    theta, phi = oracle.pix2ang(nside)
    ref = points2alm_spin(theta, phi, np.asarray(m) * (4 * np.pi / npix), lmax, 1)
    got = alms["D", 0]
    assert got.dtype.metadata["spin"] == 1
    print(f"map_catalogs -> transform, spin 1: err {_err(got, ref):.3e}")
    assert _err(got, ref) < TOL


def test_errors_and_pixel_window():
    import heracles_amd as hx
    from heracles_amd import _lib

    nside, lmax = 8, 12
    npix = 12 * nside * nside
    plan = hx.get_plan(nside, lmax)
    rng = np.random.default_rng(43)
    maps = rng.standard_normal((2, npix))
    for bad in (lambda: plan.map2alm(np.ones((3, npix)), 1),  # odd component count
                lambda: plan.alm2map(np.ones((3, plan.nlm), dtype=complex), 1),
                lambda: plan.map2alm(maps, -1), lambda: plan.alm2map(np.ones((2, plan.nlm), dtype=complex), -1)):
        with pytest.raises(hx.HxError) as exc:
            bad()
        assert exc.value.code == _lib.HX_ERR_ARG
    # the C ABI itself: odd component count and a negative spin are HX_ERR_ARG; the list entry point keeps HX_ERR_UNSUPPORTED
    L = _lib.load()
    three = np.ones((3, npix))
    out = np.zeros((3, plan.nlm), dtype=complex)
    assert L.hx_map2alm(plan._h, 1, 3, _lib.ptr(three), _lib.ptr(out), None, None, None, 0) == _lib.HX_ERR_ARG
    assert L.hx_map2alm(plan._h, -1, 2, _lib.ptr(three), _lib.ptr(out), None, None, None, 0) == _lib.HX_ERR_ARG
    assert L.hx_alm2map(plan._h, 3, 3, _lib.ptr(out), _lib.ptr(three)) == _lib.HX_ERR_ARG
    assert L.hx_alm2map(plan._h, -3, 2, _lib.ptr(out), _lib.ptr(three)) == _lib.HX_ERR_ARG
    sp = (ctypes.c_int * 1)(1)
    pm, pa = (ctypes.c_void_p * 1)(_lib.ptr(maps)), (ctypes.c_void_p * 1)(_lib.ptr(out))
    assert L.hx_map2alm_list(plan._h, 1, sp, pm, pa, None, None, None, None, 0) == _lib.HX_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="spin-1 maps not yet supported"):
        plan._map2alm_list([maps], [1])
    # pixel window: none for spin 1 -> ValueError naming the two remedies; pixwin={1: w} is applied
    w = rng.uniform(0.5, 1.0, lmax + 1)
    kw = dict(niter=0, ring_weights=np.ones(2 * nside))
    with pytest.raises(ValueError, match=r"deconvolve=False.*pixwin=\{1: "):
        hx.HipHealpixMapper(nside, lmax, pixwin=(w, w), **kw).transform(maps, spin=1)
    got = hx.HipHealpixMapper(nside, lmax, pixwin={1: w}, **kw).transform(maps, spin=1)
    plain = plan.map2alm(maps, 1)
    for m in range(lmax + 1):
        i = helpers.idx(lmax, m, m)
        lo = max(1 - m, 0)
        want = plain[:, i + lo : i + lmax - m + 1] / w[m + lo :]
        assert np.abs(got[:, i + lo : i + lmax - m + 1] - want).max() < 1e-14 * np.abs(plain).max() / w.min()
    with pytest.raises(NotImplementedError, match="spin-1 maps not yet supported"):
        hx.HipHealpixMapper(nside, lmax, deconvolve=False).transform(maps[0], spin=1)
    with pytest.raises(NotImplementedError, match="spin--1 maps not yet supported"):
        hx.HipHealpixMapper(nside, lmax, deconvolve=False).transform(maps, spin=-1)
