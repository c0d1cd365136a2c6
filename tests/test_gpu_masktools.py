"""``hx.mask_discs`` / ``hx.mask_distance`` / ``hx.apodize_mask`` on the device against the brute-force restatement of the rule
(tests/masktools_reference.py), at nside 1, 8, 12, 16 and 32: discs holding either pole, across phi = 0, on the cap / belt transition
ring and on the equator (where the ring shift alternates); a one-pixel hole in ring 1 (4 pixels); a hole whose nearest masked pixel
lies across the phi wrap; nothing and everything masked; max_distance = 180 degrees; a non-binary mask.

Discs are compared exactly -- the test first shows that no pixel / disc pair of its inputs lies within 1e-9 (relative, in h) of an
edge.  The distance obeys |H - H_ref| <= 64 2^-53 (sqrt(2 H_ref) + H_ref) and the tapers |out - out_ref| <= 256 2^-53 |mask| /
sqrt(h(aposize)) (derivations: masktools_reference.distance_bound, taper_bound).  Measured worst error / bound ratios on the device:
distance 0.038, tapers 0.0099."""

import numpy as np
import pytest

import masktools_reference as mr

pytestmark = pytest.mark.gpu

NSIDES = (1, 8, 12, 16, 32)


def _discs(nside):
    """The named discs and twelve random ones of 3 .. 20 degrees (the seeds of tests/test_masktools_host.py)."""
    lon, lat, radius = mr.named_discs(nside)
    rlon, rlat, rrad = mr.random_discs(12, 200 + nside)
    return np.concatenate([lon, rlon]), np.concatenate([lat, rlat]), np.concatenate([radius, rrad])


@pytest.fixture(scope="module")
def disc_cases():
    """{nside: (lon, lat, radius, reference mask from ones)}, computed once; no pixel on an edge."""
    out = {}
    for nside in NSIDES:
        lon, lat, radius = _discs(nside)
        gap = mr.disc_gap(nside, lon, lat, radius)
        assert gap >= 1e-9, (nside, gap)
        out[nside] = (lon, lat, radius, mr.mask_discs(np.ones(12 * nside * nside), lon, lat, radius))
    return out


@pytest.fixture(scope="module")
def hole_cases():
    """{(nside, name): (mask, H of the full minimum without a cap)}, computed once."""
    out = {}
    for nside in NSIDES:
        for name, mask in mr.hole_masks(nside).items():
            out[nside, name] = (mask, mr.mask_h(mask, 180.0))
    return out


def _h_ref(full, mask, degrees):
    H = np.minimum(full, mr.angle_h(degrees))
    H[mask <= 0] = 0.0
    return H


# ---- discs -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nside", NSIDES)
def test_discs_equal_the_reference_on_every_pixel(disc_cases, nside, monkeypatch):
    import torch

    import heracles_amd as hx

    lon, lat, radius, want = disc_cases[nside]
    got = hx.mask_discs(np.ones(want.size), lon, lat, radius)
    print(f"nside {nside}: {np.count_nonzero(got != want)} of {want.size} pixels differ, {np.count_nonzero(want == 0)} are cleared")
    assert got.tobytes() == want.tobytes()
    assert hx.mask_discs(nside, lon, lat, radius).tobytes() == want.tobytes()  # an int nside starts from ones
    assert hx.mask_discs(np.ones(want.size), lon, lat, radius).tobytes() == got.tobytes()  # two runs
    # a call split into two halves of the disc list, in place on the device, the second half first
    t = torch.ones(want.size, dtype=torch.float64, device="cuda")
    half = lon.size // 2
    assert hx.mask_discs(t, torch.from_numpy(lon[half:]).cuda(), torch.from_numpy(lat[half:]).cuda(), torch.from_numpy(radius[half:]).cuda()) is t
    hx.mask_discs(t, lon[:half], lat[:half], radius[:half])
    assert t.is_cuda and t.cpu().numpy().tobytes() == want.tobytes()
    # the other launch shape: every disc down the work-group-per-disc path
    monkeypatch.setenv("HX_MASK_WIDE", "1")
    wide = hx.mask_discs(np.ones(want.size), lon, lat, radius)
    assert wide.tobytes() == want.tobytes()


def test_discs_of_both_launch_shapes_in_one_call_keep_other_values_and_their_surroundings():
    """nside 32: two discs large enough for a work-group of their own (60 and 95 degrees, the second holding a pole) among the small
    ones; a non-binary start mask keeps its values outside the discs; NaN sentinels around the map buffer keep their bits."""
    import torch

    import heracles_amd as hx

    nside = 32
    npix = 12 * nside * nside
    lon, lat, radius = _discs(nside)
    lon, lat, radius = np.concatenate([lon, [301.3, 77.7]]), np.concatenate([lat, [-41.9, 21.3]]), np.concatenate([radius, [60.0, 95.0]])
    assert mr.disc_gap(nside, lon, lat, radius) >= 1e-9
    assert 6 * nside**2 * mr.angle_h(60.0) > 512 > 6 * nside**2 * mr.angle_h(20.0)  # (WIDE_MIN of hx_masktools.h)
    start = np.random.default_rng(5).uniform(0.1, 1.0, npix)
    want = mr.mask_discs(start, lon, lat, radius)
    assert 0 < np.count_nonzero(want) < npix
    buf = torch.full((npix + 64,), float("nan"), dtype=torch.float64, device="cuda")
    bits = buf.view(torch.int64).clone()
    view = buf[32:32 + npix]
    view.copy_(torch.from_numpy(start))
    hx.mask_discs(view, lon, lat, radius)
    assert view.cpu().numpy().tobytes() == want.tobytes()
    after = buf.view(torch.int64)
    assert torch.equal(after[:32], bits[:32]) and torch.equal(after[32 + npix:], bits[32 + npix:])
    # one radius for all, radius 0 (accepted, not pinned), no disc at all
    one = hx.mask_discs(start, lon, lat, 7.5)
    assert one.tobytes() == mr.mask_discs(start, lon, lat, 7.5).tobytes() and mr.disc_gap(nside, lon, lat, 7.5) >= 1e-9
    zero = hx.mask_discs(start, lon, lat, 0.0)
    assert ((zero == start) | (zero == 0)).all()
    assert hx.mask_discs(start, [], [], 1.0).tobytes() == start.tobytes()


# ---- distance ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nside", NSIDES)
def test_distance_matches_the_full_minimum(hole_cases, nside):
    import torch

    import heracles_amd as hx
    from heracles_amd import masks

    worst = 0.0
    for (n, name), (mask, full) in hole_cases.items():
        if n != nside:
            continue
        for degrees in (25.0, 180.0):
            want = _h_ref(full, mask, degrees)
            H = np.empty_like(mask)
            masks._mask_distance(nside, mask, degrees, H)
            err, bound = np.abs(H - want), mr.distance_bound(want)
            ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
            print(f"nside {nside}, {name}, cap {degrees}: worst |H - H_ref| / bound = {ratio:.3g}")
            worst = max(worst, ratio)
            assert (err <= bound).all(), (name, degrees, int(np.argmax(err - bound)))
            assert (H[mask <= 0] == 0).all()
            if not (mask <= 0).any():
                assert (H == mr.angle_h(degrees)).all()
            # the public call: the angle in degrees, in the kind of array it was given; two runs agree in every bit
            t = torch.from_numpy(mask).cuda()
            a, b = hx.mask_distance(t, degrees), hx.mask_distance(t, degrees)
            assert a.is_cuda and a.device == t.device and torch.equal(a, b)
            angle = hx.mask_distance(mask, degrees)
            assert isinstance(angle, np.ndarray)
            np.testing.assert_allclose(angle, np.degrees(2.0 * np.arcsin(np.minimum(np.sqrt(H * 0.5), 1.0))), rtol=0, atol=1e-12)
            np.testing.assert_allclose(a.cpu().numpy(), angle, rtol=0, atol=1e-10)
            assert angle.max() <= degrees * (1 + 1e-12) and (angle[mask <= 0] == 0).all()
    print(f"nside {nside}: worst |H - H_ref| / bound over all masks = {worst:.3g}")


# ---- tapers ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nside", NSIDES)
def test_tapers_match_the_reference(hole_cases, nside):
    import torch

    import heracles_amd as hx
    from heracles_amd import masks

    worst = 0.0
    for (n, name), (mask, full) in hole_cases.items():
        if n != nside:
            continue
        for aposize in (10.0, 25.0):
            for kind in ("C1", "C2"):
                want = mr.apodize(mask, aposize, kind, H=_h_ref(full, mask, aposize))
                got = hx.apodize_mask(mask, aposize, kind)
                assert isinstance(got, np.ndarray)
                err, bound = np.abs(got - want), mr.taper_bound(mask, aposize)
                ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
                worst = max(worst, ratio)
                assert (err <= bound).all(), (name, aposize, kind, int(np.argmax(err - bound)))
                assert (got[mask <= 0] == 0).all() and not np.signbit(got[mask <= 0]).any()
                assert (got <= np.maximum(mask, 0)).all() and (got >= 0).all()
                # out aliasing mask, on the device and on the host: the same bits
                t = torch.from_numpy(mask).cuda()
                masks._mask_taper(nside, t, aposize, masks.KINDS[kind], t)
                assert t.cpu().numpy().tobytes() == got.tobytes()
                h = mask.copy()
                masks._mask_taper(nside, h, aposize, masks.KINDS[kind], h)
                assert h.tobytes() == got.tobytes()
    print(f"nside {nside}: worst |out - out_ref| / bound over all masks, sizes and kinds = {worst:.3g}")


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_outputs_untouched():
    import torch

    import heracles_amd as hx
    from heracles_amd import masks

    nside, npix = 8, 768
    good = mr.hole_masks(nside)["non-binary with scattered holes"]
    lon, lat = np.array([10.0, 20.0, 30.0, 40.0]), np.array([5.0, -5.0, 15.0, 60.0])

    def taper(mask, aposize=10.0, kind=1, nside=nside, on_device=False, distance=False, null=None):
        out = np.full(npix, -7.0)
        if on_device:
            mask, out = torch.from_numpy(mask).cuda(), torch.from_numpy(out).cuda()
        args = [mask, out]
        if null is not None:
            args[null] = None
        with pytest.raises(hx.HxError) as err:
            if distance:
                masks._mask_distance(nside, args[0], aposize, args[1])
            else:
                masks._mask_taper(nside, args[0], aposize, kind, args[1])
        assert ((out.cpu().numpy() if on_device else out) == -7).all()
        return str(err.value)

    def discs(mask, lon, lat, radius, nside=nside, on_device=False):
        work = mask.copy()
        if on_device:
            work = torch.from_numpy(work).cuda()
        with pytest.raises(hx.HxError) as err:
            masks._mask_discs(nside, work, len(lon), lon, lat, radius, 0.0)
        assert (work.cpu().numpy() if on_device else work).tobytes() == mask.tobytes()
        return str(err.value)

    for on_device in (False, True):
        bad = good.copy()
        bad[[301, 500]] = np.nan
        assert "pixel 301" in taper(bad, on_device=on_device)
        assert "pixel 301" in taper(bad, on_device=on_device, distance=True)
        assert "pixel 301" in discs(bad, lon, lat, np.full(4, 3.0), on_device=on_device)
        bad = good.copy()
        bad[77], bad[600] = -np.inf, np.inf
        assert "pixel 77" in taper(bad, on_device=on_device)
        for aposize in (0.0, -2.0, 180.5, float("nan")):
            assert "degrees" in taper(good, aposize=aposize, on_device=on_device)
            assert "degrees" in taper(good, aposize=aposize, on_device=on_device, distance=True)
        for kind in (0, 3, -1):
            assert "kind" in taper(good, kind=kind, on_device=on_device)
        assert "disc 2" in discs(good, lon, np.array([5.0, -5.0, 90.5, -91.0]), np.full(4, 3.0), on_device=on_device)
        assert "disc 1" in discs(good, lon, lat, np.array([3.0, -1e-9, 3.0, 181.0]), on_device=on_device)
        assert "disc 3" in discs(good, lon, lat, np.array([3.0, 3.0, 3.0, np.nan]), on_device=on_device)
        assert "disc 0" in discs(good, np.array([np.nan, 1.0, np.inf, 2.0]), lat, np.full(4, 3.0), on_device=on_device)
        for null in (0, 1):
            assert "null" in taper(good, on_device=on_device, null=null)
            assert "null" in taper(good, on_device=on_device, null=null, distance=True)
    for n in (0, 8193, -4):
        assert "nside" in taper(good, nside=n)
        assert "nside" in taper(good, nside=n, distance=True)
        assert "nside" in discs(good, lon, lat, np.full(4, 3.0), nside=n)
    with pytest.raises(hx.HxError, match="null"):
        masks._mask_discs(nside, None, 4, lon, lat, None, 3.0)
    with pytest.raises(hx.HxError, match="null"):
        masks._mask_discs(nside, good.copy(), 4, None, lat, None, 3.0)
    # the public calls: ValueError before the library is reached
    for bad in (np.ones(100), np.ones(0)):
        with pytest.raises(ValueError, match="HEALPix"):
            hx.apodize_mask(bad, 2.0)
        with pytest.raises(ValueError, match="HEALPix"):
            hx.mask_discs(bad, lon, lat, 1.0)
    with pytest.raises(ValueError, match="nside"):
        hx.mask_discs(8193, lon, lat, 1.0)
    with pytest.raises(ValueError, match="kind"):
        hx.apodize_mask(good, 2.0, kind="Smooth")
    for aposize in (0.0, 181.0):
        with pytest.raises(ValueError, match="aposize"):
            hx.apodize_mask(good, aposize)
    with pytest.raises(hx.HxError, match="disc 1"):
        hx.mask_discs(good, lon, [0.0, 95.0, 0.0, 0.0], 1.0)


def test_types_follow_the_input():
    import torch

    import heracles_amd as hx

    nside, npix = 8, 768
    lon, lat, radius = _discs(nside)
    given = np.ones(npix)
    host = hx.mask_discs(given, lon, lat, radius)
    assert isinstance(host, np.ndarray) and host is not given and (given == 1).all()
    t = torch.ones(npix, dtype=torch.float64, device="cuda")
    assert hx.mask_discs(t, lon, lat, radius) is t and t.is_cuda and t.cpu().numpy().tobytes() == host.tobytes()
    d = hx.DeviceArray(torch.ones(npix, dtype=torch.float64, device="cuda"), {"nside": nside})
    assert hx.mask_discs(d, lon, lat, radius) is d and torch.equal(d.tensor, t)
    fresh = hx.mask_discs(nside, lon, lat, radius, device="cuda")
    assert fresh.is_cuda and torch.equal(fresh, t)
    with pytest.raises(ValueError, match="in place"):
        hx.mask_discs(torch.ones(npix, dtype=torch.float32, device="cuda"), lon, lat, radius)
    before = t.clone()
    apod = hx.apodize_mask(t, 10.0)
    assert apod.is_cuda and apod.device == t.device and apod is not t and torch.equal(t, before)  # (the input is read, never written)
    assert apod.cpu().numpy().tobytes() == hx.apodize_mask(host, 10.0).tobytes()
    assert torch.equal(hx.apodize_mask(d, 10.0), apod)


def test_end_to_end_mask_feeds_the_mixing_matrix_without_leaving_hbm():
    import torch

    import heracles_amd as hx

    nside, lmax = 32, 24
    rng = np.random.default_rng(8)
    lon, lat = torch.from_numpy(rng.uniform(0, 360, 40)).cuda(), torch.from_numpy(np.degrees(np.arcsin(rng.uniform(-1, 1, 40)))).cuda()
    mask = hx.apodize_mask(hx.mask_discs(nside, lon, lat, 6.0, device="cuda"), 5.0, "C2")
    assert mask.is_cuda and mask.shape == (12 * nside * nside,) and bool(torch.isfinite(mask).all()) and 0 < float(mask.mean()) < 1
    fields = {"POS": hx.Positions(None, mask="VIS")}
    mask_cls = hx.mask_product_cls({("VIS", 1): mask}, fields, lmax=2 * lmax)
    assert len(mask_cls) == 1
    w = np.asarray(next(iter(mask_cls.values())))
    assert w.shape == (2 * lmax + 1,) and np.isfinite(w).all()
    mm = hx.mixmat(w, lmax, lmax, 2 * lmax)
    assert mm.shape == (lmax + 1, lmax + 1) and np.isfinite(mm).all()
