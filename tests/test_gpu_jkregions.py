"""``hx.jackknife_regions`` / ``hx_jk_regions`` on the device against the numpy restatement of the rule
(tests/jkregions_reference.py).  The comparison of labels is exact: tests/test_jkregions_host.py shows that the reference's labels on
the parity inputs do not move when every axis is perturbed by 1e-9, seven orders above the rounding differences between the two
implementations.  The sizes are the smallest at which each kernel meets its edges: footprints below a wave, just below and just above
one 4096-key sort tile, several tiles with segments across tile and scan-tile (2048) edges, an nside that is no power of two."""

import types

import numpy as np
import pytest

import jkregions_reference as jr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parity():
    """{(nside, njk): (weight, reference labels, region weights, axes)}, computed once."""
    out = {}
    for nside, njk in ((32, 13), (64, 50)):
        w = jr.parity_weight(nside)
        out[nside, njk] = (w,) + jr.regions(nside, w, njk)
    return out


@pytest.mark.parametrize("nside,njk,count", [(32, 13, 4398), (64, 50, 17557)])
def test_parity_with_the_reference_is_exact(parity, nside, njk, count):
    import heracles_amd as hx

    w, labels, rw, axes = parity[nside, njk]
    assert np.count_nonzero(w > 0) == count
    got, info = hx.jackknife_regions(w, njk, return_info=True)
    assert got.dtype == np.int32 and got.shape == w.shape
    print(f"nside {nside}, njk {njk}: {np.count_nonzero(got != labels)} labels differ, axes differ by {np.abs(info['axes'] - axes).max():.3g}, "
          f"region weights by {np.abs(info['weights'] / rw - 1).max():.3g} (relative)")
    assert (got == labels).all()
    assert np.abs(info["axes"] - axes).max() <= 1e-10
    np.testing.assert_allclose(info["weights"], rw, rtol=1e-12)
    jr.check_invariants(w, got, njk)


SMALL = {
    "cap of 45 pixels, nside 16, njk 37": lambda: (16, jr.cap_weight(16, 0.97), 37),
    "cap at nside 24, njk 7": lambda: (24, jr.cap_weight(24, 0.97), 7),
    "njk 1": lambda: (32, jr.parity_weight(32), 1),
    "njk 2": lambda: (32, jr.parity_weight(32), 2),
    "4096 pixels": lambda: (64, jr.first_pixels_weight(64, 4096), 9),
    "4097 pixels": lambda: (64, jr.first_pixels_weight(64, 4097), 9),
}


@pytest.mark.parametrize("case", list(SMALL))
def test_sizes_where_the_kernels_can_go_wrong(case):
    import heracles_amd as hx

    nside, w, njk = SMALL[case]()
    if case.startswith("cap of 45"):
        assert np.count_nonzero(w) == 45
    if "pixels" in case and "cap" not in case:
        assert np.count_nonzero(w) == int(case.split()[0])
    labels, rw, axes = jr.regions(nside, w, njk)
    got, info = hx.jackknife_regions(w, njk, return_info=True)
    print(f"{case}: {np.count_nonzero(got != labels)} labels differ")
    assert (got == labels).all()
    assert info["axes"].shape == (njk - 1, 3) and info["weights"].shape == (njk,)
    if njk > 1:
        assert np.abs(info["axes"] - axes).max() <= 1e-10
    np.testing.assert_allclose(info["weights"], rw, rtol=1e-12)


def test_clamp_keeps_every_region_populated():
    import heracles_amd as hx

    w = jr.clamp_weight(16)
    labels, _, _ = jr.regions(16, w, 7)
    got = hx.jackknife_regions(w, 7)
    assert (np.bincount(got, minlength=8)[1:] > 0).all()
    assert ((got == 0) == (w <= 0)).all()
    assert (got == labels).all()


def test_degenerate_axis_full_sky_gives_a_valid_partition():
    """Full sky, uniform weights: the covariance is a multiple of the identity and the first axis is whatever the solver returns;
    the result is still a partition into regions of equal weight -- here exactly 1024 pixels each.  No parity."""
    import heracles_amd as hx

    w = np.ones(12 * 32 * 32)
    got, info = hx.jackknife_regions(w, 12, return_info=True)
    assert got.min() == 1 and got.max() == 12
    assert (np.bincount(got, minlength=13)[1:] == 1024).all()
    np.testing.assert_allclose(info["weights"], 1024.0, rtol=1e-12)
    assert np.abs(np.linalg.norm(info["axes"], axis=1) - 1).max() <= 1e-14


def test_two_calls_agree_in_every_bit(parity):
    import torch

    import heracles_amd as hx

    w = torch.from_numpy(parity[64, 50][0]).cuda()
    a, ia = hx.jackknife_regions(w, 50, return_info=True)
    b, ib = hx.jackknife_regions(w, 50, return_info=True)
    assert torch.equal(a, b)
    assert ia["axes"].tobytes() == ib["axes"].tobytes()
    assert torch.equal(ia["weights"], ib["weights"])


def test_types_follow_the_input(parity):
    import torch

    import heracles_amd as hx

    w, labels, rw, _ = parity[32, 13]
    t = torch.from_numpy(w).cuda()
    got, info = hx.jackknife_regions(t, 13, return_info=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int32 and got.device == t.device
    assert info["weights"].is_cuda and isinstance(info["axes"], np.ndarray)
    host = hx.jackknife_regions(w, 13)
    assert isinstance(host, np.ndarray) and host.dtype == np.int32
    assert (got.cpu().numpy() == host).all() and (host == labels).all()
    same = hx.jackknife_regions(hx.DeviceArray(t, {"nside": 32}), 13)
    assert torch.equal(same, got)
    assert torch.equal(t, torch.from_numpy(w).cuda())  # (the input is read, never written)


def test_errors_leave_the_output_untouched():
    import torch

    import heracles_amd as hx
    from heracles_amd import regions

    nside, npix = 8, 768
    good = jr.cap_weight(nside, 0.5)

    def call(weight, njk, nside=nside, on_device=False):
        """``hx_jk_regions`` on a prefilled output: the error, and whether the output kept its fill."""
        labels = np.full(npix, -7, dtype=np.int32)
        rw, axes = np.full(max(njk, 1), -7.0), np.full((max(njk, 2) - 1, 3), -7.0)
        if on_device:
            weight, labels = torch.from_numpy(weight).cuda(), torch.from_numpy(labels).cuda()
        with pytest.raises(hx.HxError) as err:
            regions._jk_regions(nside, weight, njk, labels, rw, axes)
        out = labels.cpu().numpy() if on_device else labels
        assert (out == -7).all() and (rw == -7).all() and (axes == -7).all()
        return str(err.value)

    for on_device in (False, True):
        bad = good.copy()
        bad[[301, 500]] = np.nan
        assert "pixel 301" in call(bad, 3, on_device=on_device)
        bad = good.copy()
        bad[77], bad[600] = -1e-300, np.inf
        assert "pixel 77" in call(bad, 3, on_device=on_device)
        assert "fewer" in call(jr.first_pixels_weight(nside, 5), 6, on_device=on_device)
        assert "njk" in call(good, 0, on_device=on_device)
        assert "njk" in call(good, 4097, on_device=on_device)
    assert "nside" in call(good, 3, nside=0)
    assert "nside" in call(good, 3, nside=8193)
    # the public call: ValueError before the library is reached, HxError from it
    for njk in (0, 4097):
        with pytest.raises(ValueError, match="njk"):
            hx.jackknife_regions(good, njk)
    with pytest.raises(ValueError, match="HEALPix"):
        hx.jackknife_regions(np.ones(100), 2)
    with pytest.raises(hx.HxError, match="fewer"):
        hx.jackknife_regions(jr.first_pixels_weight(nside, 5), 6)
    # five pixels are enough for five regions
    assert (np.bincount(hx.jackknife_regions(jr.first_pixels_weight(nside, 5), 5))[1:] == 1).all()


def test_end_to_end_regions_feed_jackknife_cls():
    """The tutorial's flow: visibility -> regions -> delete-1 jackknife spectra, with the region map as numpy and as a CUDA tensor."""
    import torch

    import heracles_amd as hx

    nside, lmax, njk = 32, 48, 6
    npix = 12 * nside**2
    rng = np.random.default_rng(31)
    vis = jr.parity_weight(nside)
    mapper = hx.HipHealpixMapper(nside, lmax, deconvolve=False, niter=0)
    fields = {"POS": types.SimpleNamespace(spin=0, mapper_or_error=mapper, mask="VIS"),
              "SHE": types.SimpleNamespace(spin=2, mapper_or_error=mapper, mask="WHT")}
    data, vmaps = {}, {}
    for name, shape in (("POS", (npix,)), ("SHE", (2, npix))):
        m = np.ascontiguousarray(rng.standard_normal(shape) * (vis > 0))
        m.dtype = np.dtype(m.dtype, metadata={"spin": fields[name].spin, "nside": nside, "kernel": "healpix", "bias": 0.1})
        data[name, 1] = m
        v = vis.copy()
        v.dtype = np.dtype(v.dtype, metadata={"spin": 0, "nside": nside, "kernel": "healpix"})
        vmaps[fields[name].mask, 1] = v
    jk_host = hx.jackknife_regions(vis, njk)
    jk_dev = hx.jackknife_regions(torch.from_numpy(vis).cuda(), njk)
    assert jk_dev.is_cuda and (jk_dev.cpu().numpy() == jk_host).all()
    a = hx.jackknife_cls(data, vmaps, jk_host, fields, nd=1)
    b = hx.jackknife_cls(data, vmaps, jk_dev, fields, nd=1)
    assert list(a) == list(b) == [(k,) for k in range(1, njk + 1)]
    for regions_ in a:
        assert list(a[regions_]) == list(b[regions_])
        for key in a[regions_]:
            np.testing.assert_array_equal(np.asarray(a[regions_][key].array), np.asarray(b[regions_][key].array))
    ra = hx.region_alms(fields, data, jk_dev)
    assert ra.njk == njk
    assert hx.jackknife.jackknife_fsky(jk_dev, 2) == hx.jackknife.jackknife_fsky(jk_host, 2)
