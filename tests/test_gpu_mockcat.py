"""hx_mockcat_counts / hx_mockcat_points and their Python surface on the GPU against the numpy restatement of the definition
(tests/mockcat_reference.py; pinned on its own in tests/test_mockcat_host.py).

Counts are compared exactly, except in the pixels the reference marks unsafe (a comparison or floor taken within 1e-9 of its
threshold, where another exp / log / lgamma may go the other way); at most 10^-3 of the pixels may be so marked.  Positions are
within 1e-12 degrees (a handful of ulps of 360: the device's sqrt and atan2 against the host's), noise normals within 1e-12 (the
figure of tests/test_gpu_synalm.py for the same Box-Muller).  The points are compared against the reference catalogue of the counts
the GPU returned, so a count that went the other way in an unsafe pixel does not shift every later point."""

import functools

import numpy as np
import pytest

import mockcat_reference as mr

pytestmark = pytest.mark.gpu

SEED = (11 << 32) + 77
REAL = 3
from heracles_amd.mocks import POINTS_PER_GROUP  # noqa: E402


@pytest.fixture(scope="module")
def hx():
    import heracles_amd

    heracles_amd.init(0)
    return heracles_amd


def expected_counts(nside):
    """Four kinds of expected count, laid out over the map: pixels at 5000 (each spans 20 work-groups of points), a run of empty
    pixels longer than a work-group's span of points, 1e-3, a band straddling the switch of the samplers at 32, empty pixels again at
    the end.  On the 12 and 48 pixels of nside 1 and 2 the parts are single pixels, cycled."""
    npix = 12 * nside * nside
    if npix < 3072:
        cycle = np.array([5000.0, 0.0, 1e-3, 31.9, np.nextafter(32.0, 0.0), 32.0, 32.1, 0.0, 0.0, 3.0, 700.0, 0.0])
        return cycle[np.arange(npix) % cycle.size]
    lam = np.zeros(npix)
    lam[2:6] = 5000.0
    zeros = 2 * POINTS_PER_GROUP + 44  # pixels 6 .. : empty
    a = 6 + zeros
    lam[a : a + 900] = 1e-3
    band = npix - (a + 900) - (POINTS_PER_GROUP + 9)
    lam[a + 900 : a + 900 + band] = np.linspace(31.9, 32.1, band)
    lam[a + 900 + band - 3] = 5000.0  # one more next to the trailing run of empty pixels
    return lam


def lib_counts(hx, nside, begin, end, lam, seed=SEED, realisation=REAL):
    from heracles_amd import mocks

    return mocks._mockcat_counts(nside, begin, end, np.ascontiguousarray(lam), seed, realisation)


def lib_points(hx, nside, begin, end, counts, total, maps=None, sigma=None, seed=SEED, realisation=REAL):
    from heracles_amd import mocks

    return mocks._mockcat_points(nside, begin, end, counts, total, seed, realisation, maps, sigma, np.zeros(0), pix=True)


@functools.lru_cache(maxsize=None)
def case(nside):
    """One GPU run and one reference per nside, shared (read-only) by the tests: all pixels, two value columns -- a map without
    noise, and noise of 0.3 on a zero map."""
    import heracles_amd as hx

    hx.init(0)
    npix = 12 * nside * nside
    lam = expected_counts(nside)
    counts, total = lib_counts(hx, nside, 0, npix, lam)
    maps = np.stack([np.random.default_rng(nside).standard_normal(npix), np.zeros(npix)])
    sigma = np.array([0.0, 0.3])
    lon, lat, values, pix = lib_points(hx, nside, 0, npix, counts, total, maps, sigma)
    ref_counts, unsafe = mr.counts(lam, np.arange(npix), SEED, REAL)
    ref = mr.catalog(nside, 0, counts, SEED, REAL, maps=maps, sigma=sigma)
    out = dict(nside=nside, lam=lam, counts=counts, total=total, lon=lon, lat=lat, values=values, pix=pix, maps=maps, ref_counts=ref_counts,
               unsafe=unsafe, ref=ref)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


NSIDES = [1, 2, 5, 16]


@pytest.mark.parametrize("nside", NSIDES)
def test_counts_match_the_reference(hx, nside):
    c = case(nside)
    npix = 12 * nside * nside
    assert c["counts"].dtype == np.int64 and c["total"] == c["counts"].sum()
    excluded = c["unsafe"].mean()
    print(f"nside {nside}: {c['total']} points, {int(c['unsafe'].sum())} of {npix} pixels excluded")
    assert excluded <= 1e-3
    safe = ~c["unsafe"]
    bad = np.flatnonzero(c["counts"][safe] != c["ref_counts"][safe])
    assert bad.size == 0, (bad[:5], c["counts"][safe][bad[:5]], c["ref_counts"][safe][bad[:5]])
    assert (c["counts"][c["lam"] == 0] == 0).all()


@pytest.mark.parametrize("nside", NSIDES)
def test_points_lie_in_their_pixels_and_match_the_reference(hx, nside):
    from heracles_amd.mapper import ang2pix_ring

    c = case(nside)
    assert (c["pix"] == np.repeat(np.arange(12 * nside * nside), c["counts"])).all()
    assert (ang2pix_ring(nside, c["lon"], c["lat"]) == c["pix"]).all()
    dlon, dlat = np.abs(c["lon"] - c["ref"]["lon"]).max(), np.abs(c["lat"] - c["ref"]["lat"]).max()
    print(f"nside {nside}: max |dlon| = {dlon:.2e}, max |dlat| = {dlat:.2e} degrees over {c['total']} points")
    assert dlon <= 1e-12 and dlat <= 1e-12
    assert (c["lon"] >= 0).all() and (c["lon"] < 360).all()


@pytest.mark.parametrize("nside", NSIDES)
def test_values(hx, nside):
    c = case(nside)
    assert (c["values"][0] == c["maps"][0][c["pix"]]).all()  # sigma = 0: the map, bit for bit
    err = np.abs(c["values"][1] - c["ref"]["values"][1]).max()
    print(f"nside {nside}: max |noise - reference| = {err:.2e}")
    assert err <= 1e-12
    assert c["values"][1].std() > 0.2


NS_BIG = 8192
BIG_RANGES = [0, 2 * NS_BIG * (NS_BIG - 1) - 2048, 12 * NS_BIG**2 - 4096]


@pytest.mark.parametrize("begin", BIG_RANGES)
def test_production_nside_ranges(hx, begin):
    """4096 pixels at nside 8192: the first, those across the cap / belt boundary, the last (pixel indices up to 2^29.6)."""
    from heracles_amd.mapper import ang2pix_ring

    end = begin + 4096
    lam = np.full(4096, 2.0)
    counts, total = lib_counts(hx, NS_BIG, begin, end, lam)
    ref_counts, unsafe = mr.counts(lam, np.arange(begin, end), SEED, REAL)
    assert not unsafe.any() and (counts == ref_counts).all()
    lon, lat, _, pix = lib_points(hx, NS_BIG, begin, end, counts, total)
    assert (pix == np.repeat(np.arange(begin, end), counts)).all()
    assert (ang2pix_ring(NS_BIG, lon, lat) == pix).all()
    ref = mr.catalog(NS_BIG, begin, counts, SEED, REAL)
    assert np.abs(lon - ref["lon"]).max() <= 1e-12 and np.abs(lat - ref["lat"]).max() <= 1e-12
    assert (lon >= 0).all() and (lon < 360).all()


def test_pixel_ranges_concatenate_to_the_whole(hx):
    nside = 64
    npix = 12 * nside * nside
    rng = np.random.default_rng(5)
    lam = rng.uniform(0.0, 4.0, npix) * (rng.uniform(size=npix) < 0.7)
    lam[rng.integers(0, npix, 40)] = 40.0
    maps = rng.standard_normal((2, npix))
    sigma = np.array([0.3, 0.0])
    counts, total = lib_counts(hx, nside, 0, npix, lam)
    whole = lib_points(hx, nside, 0, npix, counts, total, maps, sigma)
    cuts = [0, 1, 300, 301, 7000, 20011, 40000, npix]
    parts, pcounts = [], []
    for b, e in zip(cuts[:-1], cuts[1:]):
        cn, tot = lib_counts(hx, nside, b, e, lam[b:e])
        pcounts.append(cn)
        parts.append(lib_points(hx, nside, b, e, cn, tot, np.ascontiguousarray(maps[:, b:e]), sigma))
    assert (np.concatenate(pcounts) == counts).all()
    for k in range(4):
        assert (np.concatenate([p[k] for p in parts], axis=-1) == whole[k]).all()
    other, _ = lib_counts(hx, nside, 0, npix, lam, realisation=REAL + 1)
    assert (other != counts).mean() > 0.3
    lon2 = lib_points(hx, nside, 0, npix, counts, total, realisation=REAL + 1)[0]
    assert (lon2 != whole[0]).mean() > 0.99


@pytest.mark.parametrize("bad", [np.nan, -1e-300, 2.0**30 + 1.0, np.inf])
def test_invalid_expected_counts_are_rejected(hx, bad):
    import ctypes

    import torch

    from heracles_amd import _lib

    nside, begin, end = 4, 20, 120
    lam = np.full(end - begin, 1.5)
    lam[[37, 80]] = bad
    total = ctypes.c_int64(-7)
    for out in (np.full(end - begin, -5, dtype=np.int64), torch.full((end - begin,), -5, dtype=torch.int64, device="cuda")):
        rc = _lib.load().hx_mockcat_counts(nside, begin, end, _lib.ptr(lam), SEED, 0, _lib.ptr(out), ctypes.byref(total))
        assert rc == _lib.HX_ERR_ARG
        assert "pixel 57" in _lib.load().hx_last_error().decode()
        assert bool((out == -5).all()) and total.value == -7
    with pytest.raises(hx.HxError, match="pixel 57"):
        hx.poisson_catalog(lam, nside=nside, pixel_range=(begin, end), seed=SEED)


def test_invalid_counts_and_totals_are_rejected(hx):
    import ctypes

    from heracles_amd import _lib

    n = 48
    counts = np.full(n, 2, dtype=np.int64)
    counts[9] = -1
    lon, lat, pix = np.full(2 * n, -5.0), np.full(2 * n, -5.0), np.full(2 * n, -5, dtype=np.int64)
    rc = _lib.load().hx_mockcat_points(2, 0, n, _lib.ptr(counts), SEED, 0, 0, None, None, _lib.ptr(lon), _lib.ptr(lat), None, _lib.ptr(pix))
    assert rc == _lib.HX_ERR_ARG and "pixel 9" in _lib.load().hx_last_error().decode()
    assert (lon == -5).all() and (lat == -5).all() and (pix == -5).all()
    # 2^31 points and more in one call: three pixels at 2^30
    total = ctypes.c_int64(-7)
    out = np.full(3, -5, dtype=np.int64)
    rc = _lib.load().hx_mockcat_counts(1, 0, 3, _lib.ptr(np.full(3, 2.0**30)), SEED, 0, _lib.ptr(out), ctypes.byref(total))
    assert rc == _lib.HX_ERR_ARG and "2^31" in _lib.load().hx_last_error().decode() and (out == -5).all() and total.value == -7
    rc = _lib.load().hx_mockcat_counts(3, 0, 109, _lib.ptr(np.ones(109)), SEED, 0, _lib.ptr(np.zeros(109, dtype=np.int64)), ctypes.byref(total))
    assert rc == _lib.HX_ERR_ARG  # 109 pixels at nside 3


def test_empty_and_exactly_full_work_groups(hx):
    """No point at all; one point; and totals of exactly one and two work-groups of the point kernel (counts given, not drawn)."""
    cat = hx.poisson_catalog(np.zeros(48), np.ones((1, 48)), seed=SEED)
    assert cat.size == 0 and cat.names == ["ra", "dec", "value0"] and cat.metadata["total"] == 0
    for counts in ([0] * 47 + [1], [POINTS_PER_GROUP] + [0] * 47, [0, POINTS_PER_GROUP - 1, 0, 1, 0, POINTS_PER_GROUP] + [0] * 42):
        counts = np.array(counts, dtype=np.int64)
        lon, lat, _, pix = lib_points(hx, 2, 0, 48, counts, int(counts.sum()))
        ref = mr.catalog(2, 0, counts, SEED, REAL)
        assert (pix == ref["pix"]).all()
        assert np.abs(lon - ref["lon"]).max() <= 1e-12 and np.abs(lat - ref["lat"]).max() <= 1e-12


def test_catalogue_maps_back_to_its_counts(hx):
    """No tolerance on randomness: the catalogue's ones map back to the counts exactly, a value column to n_p v_p."""
    import torch

    nside = 16
    c = case(nside)
    npix = 12 * nside * nside
    lam = torch.from_numpy(np.array(c["lam"])).cuda()
    vmap = torch.from_numpy(np.array(c["maps"][:1])).cuda()
    cat = hx.poisson_catalog(lam, vmap, seed=SEED, realisation=REAL, value_names=("v",), weight="w")
    assert cat.size == c["total"] and cat.metadata["total"] == c["total"] and cat.metadata["nside"] == nside
    page = cat._page_columns(0, cat.size)
    assert all(page[k].is_cuda and page[k].dtype == torch.float64 for k in ("ra", "dec", "v", "w"))
    assert (page["ra"].cpu().numpy() == c["lon"]).all() and (page["v"].cpu().numpy() == c["values"][0]).all()
    mapper = hx.HipHealpixMapper(nside, 16, deconvolve=False)
    data = torch.zeros(2, npix, dtype=torch.float64, device="cuda")
    mapper.map_values(page["ra"], page["dec"], data, torch.stack([page["w"], page["v"]]))
    data = data.cpu().numpy()
    assert (data[0] == c["counts"]).all()
    want = c["counts"] * c["maps"][0]
    assert (np.abs(data[1] - want) <= 1e-13 * np.abs(want)).all()


@pytest.mark.filterwarnings("ignore:HipHealpixMapper")
def test_closed_loop_mock_catalogs_to_spectra(hx):
    import synalm_reference as sr

    nside, lmax = 32, 32
    npix = 12 * nside * nside
    mapper = hx.HipHealpixMapper(nside, lmax, deconvolve=False)
    fields = {"POS": hx.Positions(mapper, "ra", "dec"), "SHE": hx.Shears(mapper, "ra", "dec", "g1", "g2", "w")}
    layout = (("POS", 1, 0), ("POS", 2, 0), ("SHE", 1, 2), ("SHE", 2, 2))
    C = 0.002 * sr.conditioned_spectra(6, lmax, 9, {2: 2, 3: 2, 4: 2, 5: 2})
    cls = sr.matrix_to_cls(C, layout)
    maps = hx.gaussian_maps(fields, cls, seed=SEED, realisation=1, device="cuda")
    vis = np.ones(npix)
    nbar = {1: 2.0, 2: 1.2}
    cats = hx.mock_catalogs(fields, maps, nbar, visibility=vis, noise={"SHE": 0.3}, seed=SEED, realisation=1, page_size=30_000)
    assert list(cats) == [1, 2] and cats[1].names == ["ra", "dec", "g1", "g2", "w"]
    data = hx.map_catalogs(fields, cats, device="cuda")
    data = {(name, i): data[name, i] for name, i, _ in layout}  # (the order of the spectra's fields)
    for i in (1, 2):
        delta = maps["POS", i].tensor.cpu().numpy()
        total_lam = (nbar[i] * np.maximum(0.0, 1.0 + delta)).sum()
        reported = data["POS", i].dtype.metadata["nbar"] * npix  # fsky = 1: the mean count per pixel the mapping reports
        print(f"bin {i}: sum lambda = {total_lam:.1f}, catalogue {cats[i].size}, reported {reported:.1f}")
        assert abs(reported - cats[i].size) < 1e-6 * reported
        assert abs(reported - total_lam) < 5 * np.sqrt(total_lam)
    alms = hx.transform(fields, data, device="cuda")
    est = hx.angular_power_spectra(alms, debias=True)
    assert set(est) == set(cls)
    for key, block in est.items():
        array = np.asarray(getattr(block, "array", block))
        assert array.shape == cls[key].shape, key
        assert np.isfinite(array).all(), key
