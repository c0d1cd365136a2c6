"""``hx.mask_polygons`` on the device against the brute-force restatement of the rule (tests/maskpoly_reference.py), at nside 1, 8, 12, 16
and 32: a pentagon and a triangle over the poles, rectangles across phi = 0, on the cap / belt transition ring and on the equator, a
thin trail, a 64-gon, a 7-gon of 85 degrees, a sliver of 170 degrees, a rectangle that holds no pixel centre, the long triangle whose
bounding cap is wider than a hemisphere, 40 random rectangles (which overlap), 2 000 sub-pixel rectangles.

Every comparison is exact on every pixel: the reference asserts that no pixel / edge pair of its inputs has |d| / |n_e| < 1e-9
(the smallest is 3.3e-7 for the shapes, 4.8e-8 for the sub-pixel rectangles), while the device's and numpy's sin and cos differ by
a few 2^-53.  All of it fails without ``hx.mask_polygons`` / ``hx_mask_polygons``."""

import numpy as np
import pytest

import maskpoly_reference as mp

pytestmark = pytest.mark.gpu

NSIDES = (1, 8, 12, 16, 32)
WIDE_MIN = 512  # of hx_masktools.h: polygons whose bounding cap holds more pixels (estimated) get a work-group of their own


@pytest.fixture(scope="module")
def cases():
    """{nside: (polygons, inside [npoly, npix], reference from ones)}, computed once and left unchanged; no pixel on an edge."""
    polygons = [p for _, p in mp.test_shapes()]
    out = {}
    for nside in NSIDES:
        hit = np.stack([mp.inside(nside, *p) for p in polygons])  # (asserts the gap)
        out[nside] = (polygons, hit, np.where(hit.any(axis=0), 0.0, 1.0))
    assert all(mp.is_valid(*p) for p in polygons)
    return out


def _cap_pixels(nside, polygon):
    """6 nside^2 h_cap, the estimate that picks the launch shape (inf for the whole-sphere fallback)."""
    v = mp.vertices(*polygon)
    c = v.sum(axis=0)
    c /= np.linalg.norm(c)
    h = (0.5 * ((v - c) ** 2).sum(axis=1)).max()
    return np.inf if h >= 1 else 6 * nside * nside * h


# ---- exactness ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nside", NSIDES)
def test_polygons_equal_the_reference_on_every_pixel(cases, nside, monkeypatch):
    import torch

    import heracles_amd as hx

    polygons, hit, want = cases[nside]
    lon, lat, offsets = mp.flatten(polygons)
    estimates = np.array([_cap_pixels(nside, p) for p in polygons])
    assert (estimates > WIDE_MIN).any() and (estimates <= WIDE_MIN).any()  # both launch shapes in this one call
    got = hx.mask_polygons(np.ones(want.size), lon, lat, offsets)
    print(f"nside {nside}: {np.count_nonzero(got != want)} of {want.size} pixels differ, {np.count_nonzero(want == 0)} are cleared")
    assert got.tobytes() == want.tobytes()
    assert hx.mask_polygons(nside, lon, lat, offsets).tobytes() == want.tobytes()  # an int nside starts from ones
    assert hx.mask_polygons(np.ones(want.size), lon, lat, offsets).tobytes() == got.tobytes()  # two runs
    # the other winding of every polygon
    rlon, rlat, _ = mp.flatten([mp.reverse(p) for p in polygons])
    assert hx.mask_polygons(np.ones(want.size), rlon, rlat, offsets).tobytes() == want.tobytes()
    # a call split into two halves of the list, in place on the device with the vertices there too, the second half first
    t = torch.ones(want.size, dtype=torch.float64, device="cuda")
    half = len(polygons) // 2
    a, b = mp.flatten(polygons[half:]), mp.flatten(polygons[:half])
    assert hx.mask_polygons(t, *[torch.from_numpy(x).cuda() for x in a]) is t
    hx.mask_polygons(t, *b)
    assert t.is_cuda and t.cpu().numpy().tobytes() == want.tobytes()
    # one by one, both windings (the union can hide a pixel one polygon lost and another one covered)
    for k, p in enumerate(polygons):
        one = np.where(hit[k], 0.0, 1.0)
        for q in (p, mp.reverse(p)):
            assert hx.mask_polygons(nside, q[0][None, :], q[1][None, :]).tobytes() == one.tobytes(), k
    # the other launch shape: every polygon down the work-group-per-polygon path
    monkeypatch.setenv("HX_MASK_WIDE", "1")
    assert hx.mask_polygons(np.ones(want.size), lon, lat, offsets).tobytes() == want.tobytes()
    assert hx.mask_polygons(np.ones(want.size), rlon, rlat, offsets).tobytes() == want.tobytes()
    for k, p in enumerate(polygons):
        assert hx.mask_polygons(nside, p[0][None, :], p[1][None, :]).tobytes() == np.where(hit[k], 0.0, 1.0).tobytes(), k


def test_sub_pixel_rectangles_and_the_work_item_per_polygon_path(monkeypatch):
    """nside 16: 2 000 rectangles of 0.05 .. 0.9 by 0.02 .. 0.5 degrees (a pixel is 3.7 degrees across), most of which hold no pixel
    centre, through ``rectangle_polygons``' 2-D form; the same bits by either launch shape."""
    import heracles_amd as hx

    nside = 16
    polygons = mp.random_rectangles(2000, 31, length=(0.05, 0.9), width=(0.02, 0.5))
    want = mp.mask_polygons(np.ones(12 * nside * nside), polygons)  # (asserts validity and the gap)
    assert 0 < np.count_nonzero(want == 0) < 500
    lon, lat = np.stack([p[0] for p in polygons]), np.stack([p[1] for p in polygons])
    got = hx.mask_polygons(nside, lon, lat)
    print(f"{np.count_nonzero(got != want)} pixels differ, {np.count_nonzero(want == 0)} are cleared, gap {mp.gap(nside, polygons[:200]):.3g} (first 200)")
    assert got.tobytes() == want.tobytes()
    monkeypatch.setenv("HX_MASK_WIDE", "1")
    assert hx.mask_polygons(nside, lon, lat).tobytes() == want.tobytes()


def test_union_values_and_sentinels(cases):
    """nside 32, both launch shapes in one call: ``value = 1.0`` on zeros builds the union; ``value = 0.0`` on a non-binary mask leaves
    the bits of every outside pixel alone; NaN sentinels around the map buffer keep their bits."""
    import torch

    import heracles_amd as hx

    nside = 32
    npix = 12 * nside * nside
    polygons, hit, _ = cases[nside]
    lon, lat, offsets = mp.flatten(polygons)
    union = hit.any(axis=0)
    assert 0 < np.count_nonzero(union) < npix
    got = hx.mask_polygons(np.zeros(npix), lon, lat, offsets, value=1.0)
    assert got.tobytes() == np.where(union, 1.0, 0.0).tobytes()
    assert hx.mask_polygons(nside, lon, lat, offsets, value=1.0).tobytes() == got.tobytes()  # an int nside starts from zeros then
    start = np.random.default_rng(5).uniform(0.1, 1.0, npix)
    start[::7] = -0.0
    want = np.where(union, 0.0, start)
    for value, expect in ((0.0, want), (0.375, np.where(union, 0.375, start))):
        buf = torch.full((npix + 64,), float("nan"), dtype=torch.float64, device="cuda")
        bits = buf.view(torch.int64).clone()
        view = buf[32:32 + npix]
        view.copy_(torch.from_numpy(start))
        assert hx.mask_polygons(view, lon, lat, offsets, value=value) is view
        assert view.cpu().numpy().tobytes() == expect.tobytes()
        after = buf.view(torch.int64)
        assert torch.equal(after[:32], bits[:32]) and torch.equal(after[32 + npix:], bits[32 + npix:])
    assert hx.mask_polygons(start, np.zeros((0, 4)), np.zeros((0, 4))).tobytes() == start.tobytes()  # no polygon: nothing written


# ---- kinds of array ----------------------------------------------------------------------------------------------------------------------

def test_types_follow_the_input(cases):
    import torch

    import heracles_amd as hx

    nside, npix = 8, 768
    polygons, _, want = cases[nside]
    lon, lat, offsets = mp.flatten(polygons)
    given = np.ones(npix)
    host = hx.mask_polygons(given, lon, lat, offsets)
    assert isinstance(host, np.ndarray) and host is not given and (given == 1).all() and host.tobytes() == want.tobytes()
    t = torch.ones(npix, dtype=torch.float64, device="cuda")
    assert hx.mask_polygons(t, lon, lat, offsets) is t and t.is_cuda and t.cpu().numpy().tobytes() == want.tobytes()
    d = hx.DeviceArray(torch.ones(npix, dtype=torch.float64, device="cuda"), {"nside": nside})
    dlon, dlat, doff = (torch.from_numpy(x).cuda() for x in (lon, lat, offsets))
    assert hx.mask_polygons(d, dlon, dlat, doff) is d and d.tensor.is_cuda and torch.equal(d.tensor, t)  # vertices as CUDA tensors
    fresh = hx.mask_polygons(nside, dlon, dlat, doff, device="cuda")
    assert fresh.is_cuda and torch.equal(fresh, t)
    with pytest.raises(ValueError, match="in place"):
        hx.mask_polygons(torch.ones(npix, dtype=torch.float32, device="cuda"), lon, lat, offsets)
    # rectangle_polygons with tensors stays on the device and agrees with its numpy form to the last bits of a degree
    rng = np.random.default_rng(3)
    clon, clat = rng.uniform(0, 360, 50), rng.uniform(-80, 80, 50)
    rl, rb = hx.rectangle_polygons(torch.from_numpy(clon).cuda(), torch.from_numpy(clat).cuda(), 7.0, 3.0, 25.0)
    hl, hb = hx.rectangle_polygons(clon, clat, 7.0, 3.0, 25.0)
    assert rl.is_cuda and rb.is_cuda and rl.shape == rb.shape == (50, 4)
    assert np.abs(rl.cpu().numpy() - hl).max() <= 64 * 2.0**-44 and np.abs(rb.cpu().numpy() - hb).max() <= 64 * 2.0**-44


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------

def test_errors_name_the_polygon_or_pixel_and_leave_the_map_untouched():
    import torch

    import heracles_amd as hx
    from heracles_amd import masks

    nside, npix = 8, 768
    good = np.random.default_rng(9).uniform(0.05, 1.0, npix)
    squares = [(np.array([10.0, 20.0, 20.0, 10.0]) + 30 * k, np.array([-5.0, -5.0, 5.0, 5.0])) for k in range(4)]
    lon, lat, offsets = mp.flatten(squares)

    def call(mask, lon, lat, offsets, value=0.0, nside=nside, on_device=False):
        work = mask.copy()
        args = [np.ascontiguousarray(lon, dtype=np.float64), np.ascontiguousarray(lat, dtype=np.float64), np.ascontiguousarray(offsets, dtype=np.int64)]
        if on_device:
            work = torch.from_numpy(work).cuda()
            args = [torch.from_numpy(a).cuda() for a in args]
        with pytest.raises(hx.HxError) as err:
            masks._mask_polygons(nside, work, len(offsets) - 1, args[2], args[0], args[1], value)
        assert (work.cpu().numpy() if on_device else work).tobytes() == mask.tobytes()  # nothing written
        return str(err.value)

    def changed(a, index, value):
        a = np.array(a, dtype=np.float64)
        a[index] = value
        return a

    for on_device in (False, True):
        kw = {"on_device": on_device}
        # coordinates: the first such polygon is named
        assert "polygon 2" in call(good, changed(lon, [9, 14], np.nan), lat, offsets, **kw)
        assert "polygon 0" in call(good, changed(lon, 3, np.inf), lat, offsets, **kw)
        assert "polygon 1" in call(good, lon, changed(lat, [6, 13], np.nan), offsets, **kw)
        assert "polygon 3" in call(good, lon, changed(lat, 12, -np.inf), offsets, **kw)
        assert "polygon 1" in call(good, lon, changed(lat, 5, 90.5), offsets, **kw)
        assert "polygon 2" in call(good, lon, changed(lat, 10, -91.0), offsets, **kw)
        # vertex counts and offsets
        assert "polygon 1" in call(good, lon[:14], lat[:14], [0, 4, 6, 10, 14], **kw)  # 2 vertices
        big = mp.flatten([squares[0], mp.regular_ngon(40.0, 30.0, 20.0, 65), squares[1]])
        assert "polygon 1" in call(good, *big, **kw)  # 65 vertices
        assert "polygon 0" in call(good, lon, lat, [1, 4, 8, 12, 16], **kw)  # does not start at 0
        assert "polygon 1" in call(good, lon, lat, [0, 4, 3, 12, 16], **kw)  # decreases
        assert "polygon 2" in call(good, lon, lat, [0, 4, 8, 8, 12], **kw)  # an empty polygon
        # shapes that are not convex polygons
        message = call(good, changed(lon, 6, 13.0 + 30), changed(lat, 6, -2.0), offsets, **kw)  # a reflex vertex in polygon 1
        assert "polygon 1" in message and "convex" in message
        assert "polygon 3" in call(good, changed(lon, 14, lon[13]), changed(lat, 14, lat[13]), offsets, **kw)  # a repeated vertex
        assert "polygon 0" in call(good, changed(lon, [0, 1, 2], [10.0, 15.0, 20.0]), changed(lat, [0, 1, 2], 0.0), offsets, **kw)  # a collinear triple
        # the value and the mask
        for value in (np.nan, np.inf, -np.inf):
            assert "value" in call(good, lon, lat, offsets, value=value, **kw)
        assert "pixel 301" in call(changed(good, [301, 500], np.nan), lon, lat, offsets, **kw)
        assert "pixel 77" in call(changed(good, [77, 600], [-np.inf, np.inf]), lon, lat, offsets, **kw)
    for n in (0, 8193, -4):
        assert "nside" in call(good, lon, lat, offsets, nside=n)
    with pytest.raises(hx.HxError, match="null"):
        masks._mask_polygons(nside, None, 4, offsets, lon, lat, 0.0)
    for null in range(3):
        args = [offsets, lon, lat]
        args[null] = None
        with pytest.raises(hx.HxError, match="null"):
            masks._mask_polygons(nside, good.copy(), 4, *args, 0.0)
    # the public call: ValueError before the library is reached, HxError from it
    with pytest.raises(ValueError, match="HEALPix"):
        hx.mask_polygons(np.ones(100), lon, lat, offsets)
    with pytest.raises(ValueError, match="offsets end"):
        hx.mask_polygons(good, lon, lat, offsets[:-1])
    with pytest.raises(hx.HxError, match="polygon 2"):
        hx.mask_polygons(good, changed(lon, 8, np.nan).reshape(4, 4), lat.reshape(4, 4))
    with pytest.raises(hx.HxError, match="polygon 0"):
        hx.mask_polygons(good, lon.reshape(8, 2), lat.reshape(8, 2))


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

def test_end_to_end_mask_feeds_the_mask_spectra_without_leaving_hbm():
    import torch

    import heracles_amd as hx

    nside, lmax = 32, 24
    rng = np.random.default_rng(8)
    lon, lat = torch.from_numpy(rng.uniform(0, 360, 40)).cuda(), torch.from_numpy(np.degrees(np.arcsin(rng.uniform(-0.9, 0.9, 40)))).cuda()
    angle = torch.from_numpy(rng.uniform(0, 180, 40)).cuda()
    mask = hx.apodize_mask(hx.mask_polygons(hx.mask_discs(nside, lon, lat, 4.0, device="cuda"), *hx.rectangle_polygons(lon, lat, 30.0, 2.5, angle)), 5.0)
    assert mask.is_cuda and mask.shape == (12 * nside * nside,) and bool(torch.isfinite(mask).all()) and 0 < float(mask.mean()) < 1
    discs_only = hx.apodize_mask(hx.mask_discs(nside, lon, lat, 4.0, device="cuda"), 5.0)
    assert float(mask.mean()) < float(discs_only.mean())  # the spikes took pixels of their own
    fields = {"POS": hx.Positions(None, mask="VIS")}
    mask_cls = hx.mask_product_cls({("VIS", 1): mask}, fields, lmax=2 * lmax)
    assert len(mask_cls) == 1
    w = np.asarray(next(iter(mask_cls.values())))
    assert w.shape == (2 * lmax + 1,) and np.isfinite(w).all()
