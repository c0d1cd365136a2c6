"""map_catalogs on the MI355X: parity with the reference's fields (tests/golden/reference_fields.npz), device columns and device maps,
repeatability, the shared sort against separate map_values calls, the catalogue -> spectra chain with its shot-noise bias, and a
full-size catalogue (10^8 rows at nside 4096)."""

import math
import warnings

import numpy as np
import pytest

import heracles_amd as hx

from fields_cases import catalogs, fields, given_nbar, load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load()


def _check_meta(md, wmd, where):
    assert set(md) == set(wmd), where
    for k, v in wmd.items():
        if isinstance(v, float):
            assert md[k] == pytest.approx(v, rel=1e-12), (where, k)
        else:
            assert md[k] == v, (where, k)


def test_golden_parity(golden):
    g, settings, meta, warns = golden
    cats = catalogs(g, settings)
    flds = fields(settings)
    got = {}
    for cname, cat in cats.items():
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got.update(hx.map_catalogs(flds, {cname: cat}))
        assert sorted(str(r.message) for r in rec if issubclass(r.category, UserWarning)) == warns[cname]
    assert [list(k) for k in got] == settings["keys"]
    for (fname, cname), m in got.items():
        want = g[f"map/{fname}/{cname}"]
        assert isinstance(m, np.ndarray) and m.shape == want.shape, fname
        if given_nbar(settings, fname) or fname.startswith("VIS"):
            np.testing.assert_array_equal(m, want, err_msg=f"{fname} {cname}")
        else:
            np.testing.assert_allclose(m, want, rtol=0, atol=1e-13 * np.abs(want).max(), err_msg=f"{fname} {cname}")
        _check_meta(dict(m.dtype.metadata), meta[f"{fname}/{cname}"], (fname, cname))


def _device_catalog(cat):
    import torch

    cols = {k: torch.as_tensor(v, device="cuda") for k, v in cat.cols.items()}
    # (the visibility stays a numpy array: its mean, fsky, is then numpy's, as for the host catalogue)
    return hx.ArrayCatalog(cols, page_size=cat.page_size, visibility=cat.visibility, metadata=cat.metadata)


def test_device_columns_and_device_maps(golden):
    g, settings, meta, _ = golden
    cats = catalogs(g, settings)
    flds = fields(settings)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host = hx.map_catalogs(flds, cats)
        dev = hx.map_catalogs(flds, {k: _device_catalog(c) for k, c in cats.items()}, device="cuda")
        again = hx.map_catalogs(flds, {k: _device_catalog(c) for k, c in cats.items()}, device="cuda")
    assert list(dev) == list(host)
    for k, m in dev.items():
        assert isinstance(m, hx.DeviceArray) and m.tensor.is_cuda, k
        np.testing.assert_array_equal(m.tensor.cpu().numpy(), host[k], err_msg=str(k))
        np.testing.assert_array_equal(m.tensor.cpu().numpy(), again[k].tensor.cpu().numpy(), err_msg=str(k))
        assert dict(m.dtype.metadata) == dict(host[k].dtype.metadata)


def test_repeatable(golden):
    g, settings, _, _ = golden
    flds = fields(settings)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = hx.map_catalogs(flds, catalogs(g, settings))
        b = hx.map_catalogs(flds, catalogs(g, settings))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
        assert a[k].dtype.metadata == b[k].dtype.metadata


def test_shared_sort_equals_separate_map_values():
    """One sort per page for four fields of one resolution == one map_values call per field and page on device maps, bit for bit:
    POS through nbar = 1 (no rounding), the others through the same division by wbar."""
    import torch

    rng = np.random.default_rng(7)
    nside, n, page = 64, 300_000, 70_000
    lon, lat = rng.uniform(0, 360, n), np.degrees(np.arcsin(rng.uniform(-1, 1, n)))
    w = rng.uniform(0.1, 3.0, n)
    w[rng.random(n) < 0.1] = 0.0
    v, e1, e2 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    v[w == 0] = np.nan
    cat = hx.ArrayCatalog({"lon": lon, "lat": lat, "w": w, "v": v, "e1": e1, "e2": e2}, page_size=page)
    m = hx.HipHealpixMapper(nside, 2 * nside, deconvolve=False)
    flds = {"POS": hx.Positions(m, "lon", "lat", "w", overdensity=False, nbar=1.0), "VAL": hx.ScalarField(m, "lon", "lat", "v", "w"),
            "SHE": hx.Shears(m, "lon", "lat", "e1", "e2", "w"), "WHT": hx.Weights(m, "lon", "lat", "w")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = hx.map_catalogs(flds, {0: cat}, device="cuda")
    npix = 12 * nside**2
    sep = {k: torch.zeros((2, npix) if k == "SHE" else npix, dtype=torch.float64, device="cuda") for k in flds}
    for s in range(0, n, page):
        sl = slice(s, s + page)
        keep = w[sl] != 0
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
        m.map_values(dev(lon[sl]), dev(lat[sl]), sep["POS"], dev(w[sl]))
        kl, kb, kw = dev(lon[sl][keep]), dev(lat[sl][keep]), w[sl][keep]
        m.map_values(kl, kb, sep["VAL"], dev(v[sl][keep] * kw))
        m.map_values(kl, kb, sep["SHE"], dev(np.array([e1[sl][keep] * kw, e2[sl][keep] * kw])))
        m.map_values(kl, kb, sep["WHT"], dev(kw))
    torch.testing.assert_close(got["POS", 0].tensor, sep["POS"], rtol=0, atol=0)
    for k in ("VAL", "SHE", "WHT"):
        wbar = got[k, 0].dtype.metadata["wbar"]
        # (numpy divides; torch's division by a scalar multiplies by the reciprocal)
        np.testing.assert_array_equal(got[k, 0].tensor.cpu().numpy(), sep[k].cpu().numpy() / wbar, err_msg=k)


def test_chain_to_spectra_with_bias(golden):
    """map_catalogs(device) -> transform(device) -> angular_power_spectra(debias=True) == the same chain on numpy maps, with the
    shot-noise bias fsky musq / dens attached and subtracted."""
    g, settings, _, _ = golden
    cats = catalogs(g, settings)
    flds = {k: v for k, v in fields(settings).items() if k in ("POSW", "SHE", "WHTU", "VALU")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dmaps = hx.map_catalogs(flds, cats, device="cuda")
        hmaps = hx.map_catalogs(flds, cats)
        dalms = hx.transform(flds, dmaps, device="cuda")
        halms = hx.transform(flds, hmaps)
    for k in dalms:
        assert isinstance(dalms[k], hx.DeviceArray)
        md = dict(dalms[k].dtype.metadata)
        assert md == dict(halms[k].dtype.metadata)
        assert "dens" in md and md["deconv"] is False
    dcls = hx.angular_power_spectra(dalms, debias=True)
    hcls = hx.angular_power_spectra(halms, debias=True)
    assert list(dcls) == list(hcls)
    nbias = 0
    for k in hcls:
        a, b = np.asarray(dcls[k].array if hasattr(dcls[k], "array") else dcls[k]), np.asarray(hcls[k].array)
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-14 * np.abs(b).max())
        md = hcls[k].array.dtype.metadata
        assert dict(dcls[k].array.dtype.metadata) == dict(md)
        if "bias" in md:
            f, i = k[0], k[2]
            mm = hmaps[f, i].dtype.metadata
            want = mm["fsky"] * mm["musq"] / mm["dens"] * (0.5 if flds[f].spin == 2 else 1.0)
            assert md["bias"] == pytest.approx(want, rel=1e-14) and md["bias"] != 0
            nbias += 1
    assert nbias >= 4


def test_full_size_catalogue():
    """10^8 rows at nside 4096, POS + SHE + WHT from one catalogue of device columns (pages of 10^7): map sums against math.fsum of the
    weighted values over wbar, moments against long-double sums."""
    import torch

    n, nside, page = 100_000_000, 4096, 10_000_000
    gen = torch.Generator(device="cuda").manual_seed(5)
    u = lambda lo, hi: torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * (hi - lo) + lo
    lon = u(0.0, 360.0)
    lat = torch.rad2deg(torch.asin(u(-1.0, 1.0)))
    w = u(0.5, 1.5)
    w[torch.rand(n, device="cuda", generator=gen) < 0.01] = 0.0
    e1, e2 = u(-0.5, 0.5), u(-0.5, 0.5)
    vis = torch.ones(12 * nside**2, dtype=torch.float64, device="cuda")
    cat = hx.ArrayCatalog({"lon": lon, "lat": lat, "w": w, "e1": e1, "e2": e2}, page_size=page, visibility=vis)
    m = hx.HipHealpixMapper(nside, 2 * nside, deconvolve=False)
    flds = {"POS": hx.Positions(m, "lon", "lat", "w"), "SHE": hx.Shears(m, "lon", "lat", "e1", "e2", "w"),
            "WHT": hx.Weights(m, "lon", "lat", "w")}
    out = hx.map_catalogs(flds, {0: cat}, device="cuda")
    hw = w.cpu().numpy()
    keep = hw != 0
    kw = hw[keep]
    ld = np.longdouble
    sw, sw2 = np.sum(kw, dtype=ld), np.sum(kw.astype(ld) ** 2)
    ngal = int(keep.sum())
    fsky = 1.0
    wbar = float(ngal / (4 * np.pi * fsky) * (sw / ngal) * m.area)
    she, wht, pos = out["SHE", 0], out["WHT", 0], out["POS", 0]
    assert wht.dtype.metadata["wbar"] == pytest.approx(wbar, rel=1e-12)
    assert she.dtype.metadata["dens"] == pytest.approx(float(ngal / (4 * np.pi) / ((sw2 / ngal) / (sw / ngal) ** 2)), rel=1e-12)
    g1 = (e1.cpu().numpy()[keep] * kw)
    g2 = (e2.cpu().numpy()[keep] * kw)
    var = (np.sum(g1.astype(ld) ** 2) + np.sum(g2.astype(ld) ** 2)) / ngal
    assert she.dtype.metadata["musq"] == pytest.approx(float(var / (sw2 / ngal)), rel=1e-12)
    fs = lambda t: float(np.sum(t.cpu().numpy(), dtype=ld))
    assert fs(wht.tensor) == pytest.approx(math.fsum(kw) / wbar, rel=1e-12)
    assert fs(she.tensor[0]) == pytest.approx(math.fsum(g1) / wbar, rel=1e-10, abs=1e-6)
    assert fs(she.tensor[1]) == pytest.approx(math.fsum(g2) / wbar, rel=1e-10, abs=1e-6)
    nbar = float(np.sum(hw, dtype=ld) / fsky / (12 * nside**2))
    assert pos.dtype.metadata["nbar"] == pytest.approx(nbar, rel=1e-12)
    # overdensity with unit visibility: sum(map) = sum(w) / nbar - npix = 0 up to rounding
    assert abs(fs(pos.tensor)) <= 1e-4


@pytest.mark.parametrize("nside", [1024, 4096])  # 24 and 28 key bits with the sentinel: three full passes, four passes
def test_one_catalogue_order_exact_at_three_and_four_sort_passes(nside):
    """map_catalogs on device maps against the sequential loop (ordered_sum_cases.py): the page sort of hx_catmap_page, where rows of
    weight 0 take the sentinel key npix, and k_cat_run_add.  Expected: the rows with w != 0 in catalogue order across two pages of
    unequal size, np.add.at of w and of e * w, divided by the result's wbar with numpy's `/` (wbar itself is pinned elsewhere)."""
    import ordered_sum_cases as osc
    from heracles_amd.mapper import ang2pix_ring
    from oracle import hxoracle

    rng, lon, lat = osc.rows(nside + 2)
    w = rng.choice([0.0, 0.5, 1.0, 2.0], osc.N, p=[0.1, 0.2, 0.5, 0.2])
    e = osc.values(rng, (2, osc.N))
    ipix = hxoracle.ang2pix_ring(nside, lon, lat)
    np.testing.assert_array_equal(ang2pix_ring(nside, lon, lat), ipix)
    keep = w != 0
    upix, she = osc.reference(ipix[keep], e[:, keep] * w[keep])
    upix_w, wht = osc.sequential(ipix[keep], w[keep])
    np.testing.assert_array_equal(upix_w, upix)
    cat = hx.ArrayCatalog({"lon": lon, "lat": lat, "w": w, "e1": e[0], "e2": e[1]}, page_size=120_000)
    m = hx.HipHealpixMapper(nside, 2, deconvolve=False)
    flds = {"WHT": hx.Weights(m, "lon", "lat", "w"), "SHE": hx.Shears(m, "lon", "lat", "e1", "e2", "w")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = hx.map_catalogs(flds, {0: cat}, device="cuda")
    for name, want in (("WHT", wht), ("SHE", she)):
        wbar = got[name, 0].dtype.metadata["wbar"]
        osc.check_maps(got[name, 0].tensor, upix, want / wbar, 0.0, f"{name} nside {nside}")
