"""catalog_alms on the GPU (hx_catalm_*: the field rules of hx_catmap in front of the point transform's resident grids) against the
reference's map_catalogs with its DiscreteMapper (tests/golden/reference_discrete.npz) and against the oracle's direct sum.

Floating point: every comparison of alms with the oracle allows 1e-11 of `scale`, the largest |alm| after normalisation and before the
visibility is subtracted -- the bound of tests/test_gpu_pointsht.py against the same oracle, for its reason (the error of a non-uniform
FFT goes with sum |v_p|, not with the single alm; the overdensity monopole cancels against the visibility, so max |want| itself would
be about 25 times too small a yardstick there).  Two GPU runs of the same rows differ only by the order of the hardware float64 atomics
that fill the grids: they are compared at 1e-13 of `scale`, never bitwise.  Metadata floats: rel 1e-12."""

import warnings

import numpy as np
import pytest

from discrete_cases import catalogs, check_meta, fields, load, to_point
from oracle import hxoracle as ho

pytestmark = pytest.mark.gpu

FOUR_PI = 4 * np.pi


def _close(got, want, tol, scale, where=None):
    got = got.numpy() if hasattr(got, "tensor") else np.asarray(got)
    assert got.shape == want.shape, where
    err = np.abs(got - np.asarray(want)).max()
    print(f"{where}: max error {err:.3e} = {err / scale:.3e} of scale {scale:.3e} (allowed {tol:.0e})")
    assert err <= tol * scale, where


def _vis_alm(rng, lmax, fsky=0.7):
    vis = 0.05 * (rng.standard_normal(ho.nlm(lmax)) + 1j * rng.standard_normal(ho.nlm(lmax)))
    vis[: lmax + 1] = vis[: lmax + 1].real
    vis[0] = fsky * FOUR_PI**0.5
    return vis


def _direct(lon, lat, rows, lmax, spin=0):
    theta, phi = to_point(lon, lat)
    return ho.points2alm(theta, phi, np.asarray(rows), lmax, spin=spin)


# ---- 1. golden parity -----------------------------------------------------------------------------------------------------------------

def test_golden_parity():
    import heracles_amd as hx

    g, settings, meta, warns = load()
    cats = catalogs(g, settings)
    flds = fields(settings)
    got = {}
    for cname, cat in cats.items():
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got.update(hx.catalog_alms(flds, {cname: cat}))
        assert sorted(str(r.message) for r in rec) == warns[cname]
    assert [list(k) for k in got] == settings["keys"]
    for (fname, cname), a in got.items():
        assert isinstance(a, np.ndarray) and a.dtype == np.complex128
        _close(a, g[f"alm/{fname}/{cname}"], 1e-11, float(g[f"scale/{fname}/{cname}"]), (fname, cname))
        check_meta(dict(a.dtype.metadata), meta[f"{fname}/{cname}"], (fname, cname))


# ---- 2. accumulation across pages, two groups and two transforms in one context ---------------------------------------------------------

@pytest.mark.parametrize("tiles", ["0", "1"])
@pytest.mark.parametrize("lmax", [31, 48])  # 31: the smallest oversampling (n1 / (2 lmax + 1) = 2.03)
def test_pages_accumulate_against_direct_sum(lmax, tiles, monkeypatch):
    import heracles_amd as hx

    monkeypatch.setenv("HX_NUFFT_TILES", tiles)
    other = 79 - lmax
    rng = np.random.default_rng(lmax)
    n = 3000  # four pages of 700 and one of 200
    c = {"lon": rng.uniform(-180, 540, n), "lat": np.degrees(np.arcsin(rng.uniform(-1, 1, n))),
         "lon2": rng.uniform(0, 360, n), "lat2": np.degrees(np.arcsin(rng.uniform(-1, 1, n))),
         "w": rng.uniform(0.5, 1.5, n), "g1": rng.normal(0, 0.3, n), "g2": rng.normal(0, 0.3, n), "t": rng.uniform(0.5, 1.5, n)}
    zero = rng.random(n) < 0.1
    c["w"][zero] = 0.0
    c["g1"][zero] = np.nan
    vis = _vis_alm(rng, lmax)
    cat = hx.ArrayCatalog(c, page_size=700, visibility=vis)
    m, m2 = hx.HipDiscreteMapper(lmax), hx.HipDiscreteMapper(other)
    flds = {"POS": hx.Positions(m, "lon", "lat"), "SHE": hx.Shears(m, "lon", "lat", "g1", "g2", "w"),
            "WHT": hx.Weights(m, "lon", "lat", "w"), "T": hx.ScalarField(m2, "lon2", "lat2", "t", "w")}
    got = hx.catalog_alms(flds, {0: cat})
    k = ~zero
    fsky, ngal = 0.7, k.sum()
    wbar = ngal / (FOUR_PI * fsky) * c["w"][k].mean()
    nbar = n / fsky / FOUR_PI
    before = {
        "POS": _direct(c["lon"], c["lat"], [np.ones(n)], lmax)[0] / nbar,
        "SHE": _direct(c["lon"][k], c["lat"][k], [c["g1"][k] * c["w"][k], c["g2"][k] * c["w"][k]], lmax, spin=2) / wbar,
        "WHT": _direct(c["lon"][k], c["lat"][k], [c["w"][k]], lmax)[0] / wbar,
        "T": _direct(c["lon2"][k], c["lat2"][k], [c["t"][k] * c["w"][k]], other)[0] / wbar,
    }
    for name, b in before.items():
        want = b - vis if name == "POS" else b
        _close(got[name, 0], want, 1e-11, np.abs(b).max(), name)
    md = dict(got["SHE", 0].dtype.metadata)
    assert (md["geometry"], md["kernel"], md["lmax"], md["spin"]) == ("discrete", "none", lmax, 2)
    assert md["wbar"] == pytest.approx(wbar, rel=1e-12) and md["fsky"] == pytest.approx(fsky, rel=1e-12)
    assert got["POS", 0].dtype.metadata["nbar"] == pytest.approx(nbar, rel=1e-12)


# ---- 3. poles and seam ----------------------------------------------------------------------------------------------------------------

def test_poles_and_seam():
    import heracles_amd as hx

    lmax = 40
    lat = np.array([90.0, -90.0, 89.9999999, -89.9999999, 0.0, 0.0, 45.0, 45.0, -30.0, -30.0, 10.0, -90.0])
    lon = np.array([0.0, 360.0, -1e-13, 720.25, 0.0, 360.0, -1e-13, 359.9999999999, 720.25, -179.5, 540.0, 123.0])
    n = lat.size
    v1, v2 = np.arange(1.0, n + 1), np.arange(2.0 * n, n, -1.0)
    cat = hx.ArrayCatalog({"lon": lon, "lat": lat, "a": v1, "b": v2}, page_size=5)
    m = hx.HipDiscreteMapper(lmax)
    got = hx.catalog_alms({"S": hx.ScalarField(m, "lon", "lat", "a"), "G": hx.Shears(m, "lon", "lat", "a", "b")}, {0: cat})
    wbar = n / FOUR_PI
    for name, rows, spin in (("S", [v1], 0), ("G", [v1, v2], 2)):
        want = _direct(lon, lat, rows, lmax, spin=spin) / wbar
        _close(got[name, 0], want[0] if spin == 0 else want, 1e-11, np.abs(want).max(), name)


# ---- 4. the tile path and the direct path add into one grid -------------------------------------------------------------------------

def test_mixed_spread_paths_into_one_grid(monkeypatch):
    import heracles_amd as hx

    monkeypatch.delenv("HX_NUFFT_TILES", raising=False)
    rng = np.random.default_rng(4)
    lmax, n = 48, 450_000  # one page of 400 000 rows (tiles, by size), then one of 50 000 (one thread per point)
    lon, lat = rng.uniform(0, 360, n), np.degrees(np.arcsin(rng.uniform(-1, 1, n)))
    crowd = rng.random(n) < 0.5  # half of the rows inside one square degree: a lost update would show
    lon[crowd], lat[crowd] = 100.0 + rng.uniform(0, 1, crowd.sum()), 30.0 + rng.uniform(0, 1, crowd.sum())
    w, v = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    cat = hx.ArrayCatalog({"lon": lon, "lat": lat, "v": v, "w": w}, page_size=400_000)
    got = hx.catalog_alms({"S": hx.ScalarField(hx.HipDiscreteMapper(lmax), "lon", "lat", "v", "w")}, {0: cat})
    want = _direct(lon, lat, [v * w], lmax)[0] / (n / FOUR_PI * w.mean())
    _close(got["S", 0], want, 1e-11, np.abs(want).max(), "S")


# ---- 5 .. 8 share one catalogue --------------------------------------------------------------------------------------------------------

def _survey(rng, n):
    c = {"lon": rng.uniform(-180, 540, n), "lat": np.degrees(np.arcsin(rng.uniform(-1, 1, n))), "w": rng.uniform(0.5, 1.5, n),
         "g1": rng.normal(0, 0.3, n), "g2": rng.normal(0, 0.3, n), "tom": rng.integers(0, 3, n).astype(np.float64)}
    c["w"][rng.random(n) < 0.1] = 0.0
    return c


def _survey_fields(hx, lmax, lon="lon", lat="lat", g1="g1", g2="g2", w="w", overdensity=True):
    m = hx.HipDiscreteMapper(lmax)
    return {"POS": hx.Positions(m, lon, lat, overdensity=overdensity), "SHE": hx.Shears(m, lon, lat, g1, g2, w),
            "WHT": hx.Weights(m, lon, lat, w)}


def _scale(a, vis=None):
    a = a.numpy() if hasattr(a, "tensor") else np.asarray(a)
    return np.abs(a if vis is None else a + vis).max()


def test_device_columns_and_device_results():
    import torch

    import heracles_amd as hx

    rng = np.random.default_rng(5)
    lmax = 32
    c = _survey(rng, 2000)
    vis = _vis_alm(rng, lmax)
    flds = _survey_fields(hx, lmax)
    host = hx.catalog_alms(flds, {"h": hx.ArrayCatalog(c, page_size=600, visibility=vis)})
    dcat = hx.ArrayCatalog({k: torch.as_tensor(v).cuda() for k, v in c.items()}, page_size=600, visibility=torch.as_tensor(vis).cuda())
    dev = hx.catalog_alms(flds, {"h": dcat}, device="cuda")
    assert list(dev) == list(host)
    for key, a in dev.items():
        assert isinstance(a, hx.DeviceArray) and a.tensor.is_cuda and a.tensor.dtype == torch.complex128
        assert a.shape == host[key].shape
        assert dict(a.dtype.metadata) == dict(host[key].dtype.metadata)
        _close(a, host[key], 1e-13, _scale(host[key], vis if key[0] == "POS" else None), key)


@pytest.mark.parametrize("source", ["array", "fits"])
def test_views_and_filters(source, tmp_path):
    """A view and a filtered base are read through their own iteration: the alms of exactly the rows they keep."""
    import heracles_amd as hx
    from fits_table_cases import decode, write_catalog_file

    names = ["RA", "DEC", "W", "G1", "G2", "TOM_BIN_ID"]

    def edit(r):
        r["G1"][::7] = np.nan
        r["G2"][3::11] = np.nan
        r["W"][::14] = 0

    rows = write_catalog_file(tmp_path / "cat.fits", 3000, edit=edit)
    c = decode(rows, names)
    base = hx.FitsCatalog(tmp_path / "cat.fits", page_size=700) if source == "fits" else hx.ArrayCatalog(c, page_size=700)
    base.add_filter(hx.InvalidValueFilter("G1", "G2", weight="W", warn=False))
    flds = _survey_fields(hx, 32, "RA", "DEC", "G1", "G2", "W", overdensity=False)
    passes = ~((np.isnan(c["G1"]) | np.isnan(c["G2"])) & (c["W"] != 0))
    for cat, keep in ((base.where("TOM_BIN_ID == 1"), passes & (c["TOM_BIN_ID"] == 1)), (base, passes)):
        exact = hx.ArrayCatalog({k: v[keep] for k, v in c.items()}, page_size=700)
        got, want = hx.catalog_alms(flds, {0: cat}), hx.catalog_alms(flds, {0: exact})
        for key in want:
            _close(got[key], want[key], 1e-13, _scale(want[key]), (source, int(keep.sum()), key))
            check_meta(dict(got[key].dtype.metadata), dict(want[key].dtype.metadata), key)


def test_chain_to_debiased_spectra():
    """catalog_alms(device="cuda") -> transform -> angular_power_spectra(debias=True) against the oracle's alm2cl of the same alms less
    the bias.  The bound of 1e-12 is relative in the max norm over the spectrum (max |got - want| <= 1e-12 max |want|), not entry by
    entry: the rounding error of a C_l is relative to the sum of |a_lm|^2 behind it, while a debiased or an EB entry is a difference
    that cancels to any degree, so it has no relative accuracy of its own."""
    import heracles_amd as hx

    rng = np.random.default_rng(7)
    lmax = 32
    c = _survey(rng, 2000)
    flds = _survey_fields(hx, lmax)
    cat = hx.ArrayCatalog(c, page_size=600, visibility=_vis_alm(rng, lmax))
    alms = hx.transform(flds, hx.catalog_alms(flds, {0: cat}, device="cuda"))
    assert all(isinstance(a, hx.DeviceArray) for a in alms.values())
    cls = hx.angular_power_spectra(alms, debias=True)
    for name, spin in (("POS", 0), ("SHE", 2), ("WHT", 0)):
        a = alms[name, 0]
        md = a.dtype.metadata
        want = ho.alm2cl(a.numpy())
        bias = md["fsky"] * md["musq"] / md["dens"]
        if spin == 2:
            want[0, 0, 2:] -= 0.5 * bias
            want[1, 1, 2:] -= 0.5 * bias
        else:
            want -= bias
        got = np.asarray(cls[name, name, 0, 0])
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name
        assert cls[name, name, 0, 0].dtype.metadata["bias"] == pytest.approx(bias * (0.5 if spin == 2 else 1.0), rel=1e-12)


def test_budget_split(monkeypatch):
    import heracles_amd as hx
    from heracles_amd import mapping as mp

    rng = np.random.default_rng(8)
    lmax = 32  # n1 = 256: 524288 bytes per grid; the scratch of the finishing transform is 16 * 33 * (256 + 384) = 337920
    c = _survey(rng, 2000)
    vis = _vis_alm(rng, lmax)
    flds = _survey_fields(hx, lmax)  # four components: POS 1, SHE 2, WHT 1

    class Counting(hx.ArrayCatalog):
        reads = 0

        def __iter__(self):
            self.reads += 1
            return super().__iter__()

    cat = Counting(c, page_size=600, visibility=vis)
    whole = hx.catalog_alms(flds, {0: cat})
    assert cat.reads == 1
    monkeypatch.setattr(mp, "_map_budget", lambda device: 3 * 524288 + 337920)  # POS + SHE, then WHT
    cat.reads = 0
    split = hx.catalog_alms(flds, {0: cat})
    assert cat.reads == 2 and list(split) == list(whole)
    for key in whole:
        _close(split[key], whole[key], 1e-13, _scale(whole[key], vis if key[0] == "POS" else None), key)
        assert dict(split[key].dtype.metadata) == dict(whole[key].dtype.metadata)
