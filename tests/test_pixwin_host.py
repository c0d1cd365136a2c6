"""Host-side logic of the pixel windows: the window files (write / read / find), the argument checks of ``compute_pixel_window``,
its cache, and how the mapper resolves ``pixwin="compute"``.  No GPU: the window itself is pinned in tests/test_gpu_pixwin.py."""

import os

import numpy as np
import pytest


def test_exported():
    import heracles_amd
    from heracles_amd import pixwin

    for name in ("compute_pixel_window", "write_pixel_window", "read_pixel_window", "find_window_file"):
        assert name in heracles_amd.__all__
        assert getattr(heracles_amd, name) is getattr(pixwin, name)
    assert "hx_pixel_window" in heracles_amd._lib.SYMBOLS and "hx_pixel_window_rings" in heracles_amd._lib.SYMBOLS


def test_file_round_trip(tmp_path):
    from heracles_amd import fits, pixwin

    nside, lmax = 8, 32
    rng = np.random.default_rng(7)
    pw_t, pw_p = 1.0 - rng.random(lmax + 1) * 0.5, 1.0 - rng.random(lmax + 1) * 0.5
    assert pixwin.window_filename(nside) == "pixel_window_n0008.fits"
    path = tmp_path / pixwin.window_filename(nside)
    pixwin.write_pixel_window(path, nside, pw_t, pw_p)
    assert os.path.getsize(path) % fits.BLOCK == 0
    t, p = pixwin.read_pixel_window(path)
    np.testing.assert_array_equal(t, pw_t)  # bit for bit: doubles on disk
    np.testing.assert_array_equal(p, pw_p)
    # the layout is healpy's: one binary table, the columns TEMPERATURE and POLARIZATION, one row per l
    hdus = fits._scan(os.fspath(path))
    assert len(hdus) == 2
    h = hdus[1][0]
    assert h["XTENSION"] == "BINTABLE" and h["TFIELDS"] == 2 and h["NAXIS2"] == lmax + 1 and h["NAXIS1"] == 16
    assert (h["TTYPE1"], h["TTYPE2"]) == ("TEMPERATURE", "POLARIZATION") and h["NSIDE"] == nside
    raw = np.fromfile(path, dtype=">f8", count=2 * (lmax + 1), offset=hdus[1][1]).reshape(lmax + 1, 2)
    np.testing.assert_array_equal(raw[:, 0], pw_t)
    np.testing.assert_array_equal(raw[:, 1], pw_p)
    # overwriting replaces the file
    pixwin.write_pixel_window(path, nside, pw_p, pw_t)
    np.testing.assert_array_equal(pixwin.read_pixel_window(path)[0], pw_p)


def test_read_single_precision_and_swapped_columns(tmp_path):
    """Columns are found by name, in either order, as float32 ('E') as well."""
    from heracles_amd import fits, pixwin

    n = 5
    t = np.linspace(1.0, 0.5, n).astype(np.float32)
    p = np.linspace(0.9, 0.4, n).astype(np.float32)
    path = os.fspath(tmp_path / "w.fits")
    fits._new_file(path, True)
    cards = [fits._card("XTENSION", "BINTABLE"), fits._card("BITPIX", 8), fits._card("NAXIS", 2), fits._card("NAXIS1", 8), fits._card("NAXIS2", n),
             fits._card("PCOUNT", 0), fits._card("GCOUNT", 1), fits._card("TFIELDS", 2), fits._card("TTYPE1", "POLARIZATION"), fits._card("TFORM1", "1E"),
             fits._card("TTYPE2", "TEMPERATURE"), fits._card("TFORM2", "1E")]
    payload = np.stack([p, t], axis=1).astype(">f4").tobytes()
    with open(path, "ab") as f:
        f.write(fits._header_bytes(cards))
        f.write(payload + b"\0" * (-len(payload) % fits.BLOCK))
    rt, rp = pixwin.read_pixel_window(path)
    assert rt.dtype == np.float64
    np.testing.assert_array_equal(rt, t.astype(np.float64))
    np.testing.assert_array_equal(rp, p.astype(np.float64))


def test_find_window_file(tmp_path):
    from heracles_amd import pixwin

    assert pixwin.find_window_file(None, 8) is None
    assert pixwin.find_window_file(tmp_path, 8) is None
    path = tmp_path / "pixel_window_n0008.fits"
    pixwin.write_pixel_window(path, 8, np.ones(33), np.ones(33))
    assert pixwin.find_window_file(tmp_path, 8) == os.fspath(path)
    assert pixwin.find_window_file(os.fspath(tmp_path), 16) is None
    assert pixwin.find_window_file(path, 8) == os.fspath(path)
    assert pixwin.find_window_file(path, 16) is None  # a path to another resolution's file (or to a weight file) is not a window of this one
    # load: cut at lmax, refused if the table is too short
    t, p = pixwin.load_pixel_window(tmp_path, 8, 20)
    assert t.shape == p.shape == (21,)
    with pytest.raises(ValueError, match="ends at l = 32"):
        pixwin.load_pixel_window(tmp_path, 8, 33)
    pixwin.release_computed()


def test_write_refuses_mismatched_arrays(tmp_path):
    from heracles_amd import pixwin

    with pytest.raises(ValueError):
        pixwin.write_pixel_window(tmp_path / "a.fits", 8, np.ones(5), np.ones(6))
    with pytest.raises(ValueError):
        pixwin.write_pixel_window(tmp_path / "a.fits", 8, np.ones((2, 5)), np.ones((2, 5)))
    with pytest.raises(ValueError):
        pixwin.write_pixel_window(tmp_path / "a.fits", 0, np.ones(5), np.ones(5))


@pytest.mark.parametrize("kw", [dict(nside=0), dict(nside=8193), dict(nside=2.5), dict(nside=8, lmax=-1), dict(nside=8, lmax=33), dict(nside=1, lmax=5),
                                dict(nside=8, spin=-1), dict(nside=8, lmax=4, spin=5), dict(nside=8, spin=(0, -2)), dict(nside=8, spin=1.5),
                                dict(nside=8, lmax=10, spin=(0, 11)), dict(nside=8, spin=True)])
def test_bad_arguments_are_refused_before_the_gpu(kw):
    from heracles_amd import pixwin

    with pytest.raises(ValueError):
        pixwin.compute_pixel_window(**kw)
    with pytest.raises(ValueError):
        pixwin.compute_pixel_window(**kw, device="cuda", rings=True)


def test_band_limit_message():
    from heracles_amd import pixwin

    with pytest.raises(ValueError, match="4 nside = 32"):
        pixwin.compute_pixel_window(8, 33)


def test_key_and_defaults():
    from heracles_amd import pixwin

    assert pixwin._key(8, None, 0) == (8, 23, (0,), True)
    assert pixwin._key(np.int64(8), 23, np.int64(0)) == (8, 23, (0,), True)
    assert pixwin._key(3, 12, (0, 2)) == (3, 12, (0, 2), False)  # any integer nside, up to 4 nside
    assert pixwin._key(8, 32, [1]) == (8, 32, (1,), False)


def test_cached_results_are_served_and_released():
    """A cached entry is returned without a computation (none is possible here), as a copy the caller may change; a tuple of spin
    weights gives a tuple; release_caches() drops the entries."""
    import heracles_amd
    from heracles_amd import pixwin

    w0, w2, rows = np.linspace(1.0, 0.5, 24), np.linspace(1.0, 0.4, 24), np.arange(16.0 * 24).reshape(16, 24)
    pixwin._computed[(8, 23, 0, None, False)] = w0
    pixwin._computed[(8, 23, 2, None, False)] = w2
    pixwin._computed[(8, 23, 0, None, True)] = rows
    try:
        got = pixwin.compute_pixel_window(8)
        np.testing.assert_array_equal(got, w0)
        got[0] = -1.0
        assert pixwin.compute_pixel_window(8, 23, 0)[0] == 1.0
        pair = pixwin.compute_pixel_window(8, spin=(0, 2))
        assert isinstance(pair, tuple) and len(pair) == 2
        np.testing.assert_array_equal(pair[1], w2)
        np.testing.assert_array_equal(pixwin.compute_pixel_window(8, rings=True), rows)
    finally:
        heracles_amd.release_caches()
    assert not pixwin._computed and not pixwin._files


def test_mapper_resolves_compute(tmp_path):
    """``pixwin="compute"`` / ``{s: "compute"}``: the computed window of that spin weight (served from the cache here), a window file
    under ``datapath`` ahead of it for spin 0 and 2; ``pixel_window(..., "compute")`` is the pair of spin 0 and 2."""
    import heracles_amd
    from heracles_amd import mapper, pixwin

    nside, lmax = 8, 12
    w = {s: np.linspace(1.0, 0.5 + 0.1 * s, lmax + 1) for s in (0, 1, 2)}
    try:
        for s in w:
            pixwin._computed[(nside, lmax, s, None, False)] = w[s]
        m = heracles_amd.HipHealpixMapper(nside, lmax, pixwin="compute")
        assert m.pixwin == "compute"
        for s in w:
            fl = m._fl(s)
            np.testing.assert_array_equal(fl[:s], 1.0)
            np.testing.assert_array_equal(fl[s:], 1.0 / w[s][s:])
        m1 = heracles_amd.HipHealpixMapper(nside, lmax, pixwin={1: "compute"})
        np.testing.assert_array_equal(m1._fl(1)[1:], 1.0 / w[1][1:])
        p0, p2 = mapper.pixel_window(nside, lmax, "compute")
        np.testing.assert_array_equal(p0, w[0])
        np.testing.assert_array_equal(p2, w[2])
        p0, p2 = mapper.pixel_window(nside, lmax, {0: "compute", 2: w[1]})
        np.testing.assert_array_equal(p0, w[0])
        np.testing.assert_array_equal(p2, w[1])
        # a window file under datapath goes first, for spin 0 and 2 only
        ft, fp = np.full(lmax + 1, 0.75), np.full(lmax + 1, 0.25)
        pixwin.write_pixel_window(tmp_path / pixwin.window_filename(nside), nside, ft, fp)
        mf = heracles_amd.HipHealpixMapper(nside, lmax, pixwin="compute", datapath=tmp_path)
        np.testing.assert_array_equal(mf._fl(0), 1.0 / ft)
        np.testing.assert_array_equal(mf._fl(2)[2:], 1.0 / fp[2:])
        np.testing.assert_array_equal(mf._fl(1)[1:], 1.0 / w[1][1:])
        np.testing.assert_array_equal(mapper.pixel_window(nside, lmax, "compute", tmp_path)[1], fp)
        # without deconvolution nothing is resolved
        assert heracles_amd.HipHealpixMapper(nside, lmax, pixwin="compute", deconvolve=False)._fl(0) is None
    finally:
        heracles_amd.release_caches()


def test_without_compute_everything_resolves_as_before():
    """No "compute": a weight other than 0 and 2 without a window is still the error it was."""
    import heracles_amd

    m = heracles_amd.HipHealpixMapper(8, 12, pixwin=(np.ones(13), np.ones(13)))
    with pytest.raises(ValueError, match="no pixel window for spin-1 fields"):
        m._fl(1)
    np.testing.assert_array_equal(m._fl(0), np.ones(13))
    m = heracles_amd.HipHealpixMapper(8, 12, pixwin={1: np.full(13, 0.5)})
    np.testing.assert_array_equal(m._fl(1), np.r_[1.0, np.full(12, 2.0)])
