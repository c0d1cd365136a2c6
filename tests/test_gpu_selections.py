"""Views of one catalogue mapped in one pass (hx_catmap_*_sel) on the MI355X: every view's maps against the per-catalogue path fed with
exactly the view's rows (bit for bit where nbar is given), compiled predicates against the same selection as masks, device against host
columns, repeatability, a forced split, errors, the spectra chain, and 10^8 rows in 13 bins at nside 4096."""

import warnings

import numpy as np
import pytest

import heracles_amd as hx
from heracles_amd import mapping as mp
from heracles_amd.mapper import ang2pix_ring

pytestmark = pytest.mark.gpu

NSIDE = 32


def _columns(n, seed=7, nbins=4):
    rng = np.random.default_rng(seed)
    cols = {
        "RA": rng.uniform(0, 360, n),
        "DEC": np.degrees(np.arcsin(rng.uniform(-1, 1, n))),
        "E1": rng.normal(0, 0.3, n),
        "E2": rng.normal(0, 0.3, n),
        "W": rng.choice([0.0, 0.5, 1.0, 2.0], n, p=[0.1, 0.2, 0.5, 0.2]),
        "TOM_BIN_ID": rng.integers(0, nbins, n).astype(np.int64),
        "Z": rng.uniform(0, 2, n),
    }
    return cols


def _fields(nside=NSIDE, nbar=None):
    m = hx.HipHealpixMapper(nside, 2 * nside, deconvolve=False)
    return {
        "POS": hx.Positions(m, "RA", "DEC", overdensity=False, nbar=nbar),
        "SHE": hx.Shears(m, "RA", "DEC", "E1", "-E2", "W"),
        "WHT": hx.Weights(m, "RA", "DEC", "W"),
    }


def _rows_of(cols, keep):
    return {k: v[keep] for k, v in cols.items()}


def _apply_filters(cols, filters):
    """The filters' rule restated on whole columns (heracles/catalog/filters.py)."""
    keep = np.ones(len(cols["RA"]), bool)
    for f in filters:
        if isinstance(f, hx.InvalidValueFilter):
            bad = np.zeros_like(keep)
            for c in f.columns:
                bad |= np.isnan(cols[c])
            if f.weight is not None:
                bad &= cols[f.weight] != 0
            keep &= ~bad
        else:
            fp = f.footprint.cpu().numpy() if hasattr(f.footprint, "data_ptr") else np.asarray(f.footprint)
            ipix = ang2pix_ring(f.nside, cols[f.lonlat[0]][keep], cols[f.lonlat[1]][keep]) if keep.any() else np.zeros(0, int)
            sub = np.flatnonzero(keep)
            keep[sub[fp[ipix] == 0]] = False
    return keep


def _per_view(fields, cols, masks, filters, page_size, vis=None):
    """Each view as a catalogue holding exactly its rows, mapped through the per-catalogue path."""
    out = {}
    for j, keep in masks.items():
        sub = _rows_of(cols, keep)
        sub = _rows_of(sub, _apply_filters(sub, filters))
        cat = hx.ArrayCatalog(sub, page_size=page_size, visibility=None if vis is None else vis.get(j))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out.update(hx.map_catalogs(fields, {j: cat}))
    return out


def _compare(got, want, fields, exact_pos):
    assert list(got) == list(want)
    for key, m in got.items():
        w = want[key]
        m = np.asarray(m)
        if key[0] == "POS" and exact_pos:
            np.testing.assert_array_equal(m, w, err_msg=str(key))
        else:
            np.testing.assert_allclose(m, w, rtol=0, atol=1e-13 * max(np.abs(w).max(), 1e-300), err_msg=str(key))
        for k, v in w.dtype.metadata.items():
            if isinstance(v, float):
                assert m.dtype.metadata[k] == pytest.approx(v, rel=1e-12, abs=1e-300, nan_ok=True), (key, k)
            else:
                assert m.dtype.metadata[k] == v, (key, k)


@pytest.mark.parametrize("overlap", [False, True])
def test_one_pass_equals_per_view(overlap):
    n = 50_000
    cols = _columns(n)
    cols["E1"][17] = np.nan  # a NaN in a row with weight 0: the weighted filter keeps it, the fields drop it
    cols["W"][17] = 0.0
    cols["Z"][::97] = np.nan
    fields = _fields(nbar=3.0)
    base = hx.ArrayCatalog(cols, page_size=7_001)
    base.add_filter(hx.InvalidValueFilter("E1", "E2", weight="W", warn=False))
    base.add_filter(hx.InvalidValueFilter("Z"))
    views = {str(k): base.where(f"TOM_BIN_ID=={k}") for k in range(4)}
    masks = {str(k): cols["TOM_BIN_ID"] == k for k in range(4)}
    if overlap:
        views["all"] = base
        masks["all"] = np.ones(n, bool)
        views["hiz"] = base.where(cols["Z"] > 1.0)["TOM_BIN_ID < 3"]
        masks["hiz"] = (cols["Z"] > 1.0) & (cols["TOM_BIN_ID"] < 3)
        views["none"] = base.where("TOM_BIN_ID > 99")
        masks["none"] = np.zeros(n, bool)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = hx.map_catalogs(fields, views)
    assert "WARNING: catalog contains invalid values" in {str(r.message) for r in rec}
    want = _per_view(fields, cols, masks, base.filters, 7_001)
    _compare(got, want, fields, exact_pos=True)


def test_predicates_equal_masks_and_device_columns():
    import torch

    n = 40_000
    cols = _columns(n, seed=3)
    fields = _fields(nbar=2.0)
    base = hx.ArrayCatalog(cols, page_size=9_000)
    a = hx.map_catalogs(fields, {k: base[f"(TOM_BIN_ID=={k}) & (Z >= 0.5)"] for k in range(4)})
    b = hx.map_catalogs(fields, {k: base[(cols["TOM_BIN_ID"] == k) & (cols["Z"] >= 0.5)] for k in range(4)})
    dcols = {k: torch.as_tensor(v.astype(np.float64), device="cuda") for k, v in cols.items()}
    dbase = hx.ArrayCatalog(dcols, page_size=9_000)
    c = hx.map_catalogs(fields, {k: dbase[f"(TOM_BIN_ID=={k}) & (Z >= 0.5)"] for k in range(4)})
    d = hx.map_catalogs(fields, {k: dbase[(dcols["TOM_BIN_ID"] == k) & (dcols["Z"] >= 0.5)] for k in range(4)})
    e = hx.map_catalogs(fields, {k: base[f"(TOM_BIN_ID=={k}) & (Z >= 0.5)"] for k in range(4)})  # a second run
    for key in a:
        for other in (b, c, d, e):
            np.testing.assert_array_equal(np.asarray(other[key]), np.asarray(a[key]), err_msg=str(key))
            assert dict(other[key].dtype.metadata) == dict(a[key].dtype.metadata)


def test_forced_split_equals_one_pass(monkeypatch):
    n = 30_000
    cols = _columns(n, seed=11, nbins=5)
    fields = _fields(nbar=1.0)
    base = hx.ArrayCatalog(cols, page_size=4_096)
    views = {k: base[f"TOM_BIN_ID=={k}"] for k in range(5)}
    one = hx.map_catalogs(fields, views)
    passes = []
    real = mp._CatMapSel
    monkeypatch.setattr(mp, "_CatMapSel", lambda *a, **k: passes.append(a[3]) or real(*a, **k))
    per_view = 8 * 4 * 12 * NSIDE**2  # POS, SHE (two rows) and WHT
    monkeypatch.setattr(mp, "_map_budget", lambda device: 2 * per_view)
    split = hx.map_catalogs(fields, views)
    assert passes == [2, 2, 1]
    for key in one:
        np.testing.assert_array_equal(np.asarray(split[key]), np.asarray(one[key]), err_msg=str(key))


def test_footprint_visibility_and_device_maps():
    import torch

    n = 30_000
    cols = _columns(n, seed=5, nbins=3)
    fp = np.zeros(12 * 8**2)
    fp[: len(fp) // 2] = 1.0  # the northern half (RING order) at nside 8
    base = hx.ArrayCatalog(cols, page_size=6_000)
    base.add_filter(hx.FootprintFilter(torch.as_tensor(fp, device="cuda"), "RA", "DEC"))
    m16 = hx.HipHealpixMapper(16, 32, deconvolve=False)
    fields = {"POS": hx.Positions(m16, "RA", "DEC", overdensity=True), "VIS": hx.Visibility(m16), **{k: v for k, v in _fields(16).items() if k != "POS"}}
    vis = {0: np.full(12 * 16**2, 0.5), 1: np.full(12 * 8**2, 0.25), 2: None}
    views = {}
    for k in range(3):
        views[k] = base.where(f"TOM_BIN_ID=={k}", visibility=vis[k])
    base.visibility = np.full(12 * 16**2, 0.75)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = hx.map_catalogs(fields, views, device="cuda")
    texts = {str(r.message) for r in rec}
    assert "positions and visibility have different size" in texts and "changing size of visibility map" in texts
    masks = {k: cols["TOM_BIN_ID"] == k for k in range(3)}
    want = {}
    for k, keep in masks.items():
        sub = _rows_of(cols, keep)
        sub = _rows_of(sub, _apply_filters(sub, base.filters))
        cat = hx.ArrayCatalog(sub, page_size=6_000, visibility=views[k].visibility)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want.update(hx.map_catalogs(fields, {k: cat}))
    assert list(got) == list(want)
    for key, m in got.items():
        assert isinstance(m, hx.DeviceArray)
        w = want[key]
        np.testing.assert_allclose(m.tensor.cpu().numpy(), w, rtol=0, atol=1e-13 * np.abs(w).max(), err_msg=str(key))
        for kk, v in w.dtype.metadata.items():
            if isinstance(v, float):
                assert m.dtype.metadata[kk] == pytest.approx(v, rel=1e-12), (key, kk)


def test_errors_follow_the_views():
    n = 5_000
    cols = _columns(n, seed=2, nbins=2)
    cols["TOM_BIN_ID"][10] = 1
    cols["DEC"][10] = 95.0
    outside = np.flatnonzero(cols["TOM_BIN_ID"] == 0)[0]
    cols["E1"][outside] = np.nan
    cols["W"][outside] = 1.0
    base = hx.ArrayCatalog(cols, page_size=1_000)
    fields = _fields()
    # a NaN in a row outside every view raises nothing; the invalid latitude of bin 1 raises in its turn
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = hx.map_catalogs(fields, {"a": base["TOM_BIN_ID==1"][cols["RA"] < -1]})
    assert list(got) == [("POS", "a"), ("SHE", "a"), ("WHT", "a")]
    with pytest.raises(ValueError, match="latitude outside"):
        hx.map_catalogs(fields, {"b": base["TOM_BIN_ID==1"]})
    with pytest.raises(ValueError, match='invalid values in column "E1"'):
        hx.map_catalogs(fields, {"c": base["TOM_BIN_ID==0"], "d": base["TOM_BIN_ID==1"]})


def test_chain_to_spectra():
    n = 60_000
    cols = _columns(n, seed=9, nbins=3)
    base = hx.ArrayCatalog(cols, page_size=20_000, visibility=np.ones(12 * NSIDE**2))
    fields = {"POS": hx.Positions(hx.HipHealpixMapper(NSIDE, 2 * NSIDE, deconvolve=False), "RA", "DEC")}
    views = {k: base[f"TOM_BIN_ID=={k}"] for k in range(3)}
    maps = hx.map_catalogs(fields, views, device="cuda")
    alms = hx.transform(fields, maps, device="cuda")
    cls = hx.angular_power_spectra(alms, debias=True)
    want_maps = _per_view(fields, cols, {k: cols["TOM_BIN_ID"] == k for k in range(3)}, [], 20_000,
                          vis={k: np.ones(12 * NSIDE**2) for k in range(3)})
    want = hx.angular_power_spectra(hx.transform(fields, want_maps), debias=True)
    assert set(cls) == set(want)
    for key in want:
        a, b = np.asarray(cls[key]), np.asarray(want[key])
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-12 * np.abs(b).max(), err_msg=str(key))


def test_full_size_thirteen_bins():
    import torch

    n, nside, nbins = 100_000_000, 4096, 13
    g = torch.Generator(device="cuda").manual_seed(1)
    u = torch.rand(n, device="cuda", dtype=torch.float64, generator=g)
    cols = {
        "RA": 360.0 * torch.rand(n, device="cuda", dtype=torch.float64, generator=g),
        "DEC": torch.rad2deg(torch.asin(2.0 * u - 1.0)),
        "E1": 0.3 * torch.randn(n, device="cuda", dtype=torch.float64, generator=g),
        "E2": 0.3 * torch.randn(n, device="cuda", dtype=torch.float64, generator=g),
        "W": torch.rand(n, device="cuda", dtype=torch.float64, generator=g),
        "TOM_BIN_ID": torch.randint(0, nbins, (n,), device="cuda", generator=g).to(torch.float64),
    }
    del u
    m = hx.HipHealpixMapper(nside, 2, deconvolve=False)
    fields = {"POS": hx.Positions(m, "RA", "DEC", overdensity=False, nbar=1.0), "SHE": hx.Shears(m, "RA", "DEC", "E1", "E2", "W"),
              "WHT": hx.Weights(m, "RA", "DEC", "W")}
    base = hx.ArrayCatalog(cols, page_size=n)
    got = hx.map_catalogs(fields, {k: base[f"TOM_BIN_ID=={k}"] for k in range(nbins)}, device="cuda")
    rng = np.random.default_rng(0)
    pix = torch.as_tensor(rng.integers(0, 12 * nside**2, 4096), device="cuda")
    samples = {key: (v.tensor[..., pix].cpu().numpy(), dict(v.dtype.metadata)) for key, v in got.items()}
    del got
    torch.cuda.empty_cache()
    for k in (0, 7, 12):
        keep = cols["TOM_BIN_ID"] == k
        sub = {c: v[keep].contiguous() for c, v in cols.items()}
        want = hx.map_catalogs(fields, {k: hx.ArrayCatalog(sub, page_size=n)}, device="cuda")
        for name in fields:
            got_s, md = samples[name, k]
            w = want[name, k].tensor[..., pix].cpu().numpy()
            if name == "POS":
                np.testing.assert_array_equal(got_s, w)
            else:
                np.testing.assert_allclose(got_s, w, rtol=0, atol=1e-13 * max(np.abs(w).max(), 1e-300))
            for kk, v in want[name, k].dtype.metadata.items():
                if isinstance(v, float):
                    assert md[kk] == pytest.approx(v, rel=1e-12), (name, k, kk)
        del want, sub
        torch.cuda.empty_cache()


def test_fallback_strings_and_nan_comparisons_on_the_device():
    n = 20_000
    cols = _columns(n, seed=13)
    cols["Z"][::13] = np.nan  # no filter: `!=` keeps these rows, the other comparisons drop them
    fields = _fields(nbar=2.0)
    base = hx.ArrayCatalog(cols, page_size=6_000)
    exprs = {"or": "(TOM_BIN_ID==0) | (TOM_BIN_ID==2)", "ne": "Z != 1.0", "eq": "Z == Z", "lt": "(Z < 1.0) & (TOM_BIN_ID != 1)",
             "ge": "Z >= 1.0"}
    assert mp._compile_predicate(exprs["or"], mp._dtypes(base)) is None and mp._compile_predicate(exprs["ne"], mp._dtypes(base))
    got = hx.map_catalogs(fields, {k: base[e] for k, e in exprs.items()})
    want = _per_view(fields, cols, {k: eval(e, None, dict(cols)) for k, e in exprs.items()}, [], 6_000)
    _compare(got, want, fields, exact_pos=True)


def test_wide_keys_use_the_64_bit_sort():
    import torch

    n, nside, nbins = 2_000_000, 4096, 22  # 22 (12 nside^2 + 1) > 2^32
    cols = _columns(n, seed=17, nbins=nbins)
    m = hx.HipHealpixMapper(nside, 2, deconvolve=False)
    fields = {"POS": hx.Positions(m, "RA", "DEC", overdensity=False, nbar=1.0)}
    base = hx.ArrayCatalog(cols, page_size=n)
    got = hx.map_catalogs(fields, {k: base[f"TOM_BIN_ID=={k}"] for k in range(nbins)}, device="cuda")
    for k in (0, 11, 21):
        keep = cols["TOM_BIN_ID"] == k
        want = hx.map_catalogs(fields, {k: hx.ArrayCatalog(_rows_of(cols, keep), page_size=n)}, device="cuda")
        assert torch.equal(got["POS", k].tensor, want["POS", k].tensor), k
        del want


# ---- ordered sums of views at production key widths (ordered_sum_cases.py) ---------------------------------------------------------------
def _ordered_view_catalogue(nside, seed, nbins, weights):
    import ordered_sum_cases as osc
    from oracle import hxoracle

    rng, lon, lat = osc.rows(seed)
    cols = {"RA": lon, "DEC": lat, "W": weights(rng), "E1": osc.values(rng, osc.N), "E2": osc.values(rng, osc.N),
            "TOM_BIN_ID": rng.integers(0, nbins, osc.N).astype(np.int64)}
    ipix = hxoracle.ang2pix_ring(nside, lon, lat)
    np.testing.assert_array_equal(ang2pix_ring(nside, lon, lat), ipix)
    return cols, ipix


def _record_passes(monkeypatch):
    """The number of views of every hx_catmap_sel pass, as test_forced_split_equals_one_pass records them: the key width of a pass
    depends on all its views being in it."""
    passes = []
    real = mp._CatMapSel
    monkeypatch.setattr(mp, "_CatMapSel", lambda *a, **k: passes.append(a[3]) or real(*a, **k))
    return passes


def test_views_order_exact_at_four_sort_passes(monkeypatch):
    """Six views at nside 1024: the keys sel * (npix + 1) + pix go up to 75 497 478, 27 bits, the narrow sort with four passes.  Every
    view's WHT and SHE maps against the sequential loop over exactly that view's rows with w != 0, in catalogue order across two
    pages, divided by the view's wbar with numpy's `/`."""
    import ordered_sum_cases as osc

    nside, nbins = 1024, 5
    cols, ipix = _ordered_view_catalogue(nside, 31, nbins, lambda rng: rng.choice([0.0, 0.5, 1.0, 2.0], osc.N, p=[0.1, 0.2, 0.5, 0.2]))
    m = hx.HipHealpixMapper(nside, 2, deconvolve=False)
    fields = {"WHT": hx.Weights(m, "RA", "DEC", "W"), "SHE": hx.Shears(m, "RA", "DEC", "E1", "E2", "W")}
    base = hx.ArrayCatalog(cols, page_size=120_000)
    views = {k: base[f"TOM_BIN_ID=={k}"] for k in range(nbins)}
    masks = {k: cols["TOM_BIN_ID"] == k for k in range(nbins)}
    views["low"] = base["TOM_BIN_ID < 3"]  # overlaps bins 0, 1 and 2
    masks["low"] = cols["TOM_BIN_ID"] < 3
    passes = _record_passes(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = hx.map_catalogs(fields, views, device="cuda")
    assert passes == [len(views)] and set(got) == {(f, k) for k in views for f in fields}
    for k, mask in masks.items():
        keep = mask & (cols["W"] != 0)
        w = cols["W"][keep]
        upix, she = osc.reference(ipix[keep], np.array([cols["E1"][keep] * w, cols["E2"][keep] * w]))
        _, wht = osc.sequential(ipix[keep], w)
        for name, want in (("WHT", wht), ("SHE", she)):
            wbar = got[name, k].dtype.metadata["wbar"]
            osc.check_maps(got[name, k].tensor, upix, want / wbar, 0.0, f"{name} view {k}")


def test_views_order_exact_with_64_bit_keys(monkeypatch):
    """22 views at nside 4096: 22 (12 nside^2 + 1) > 2^32, so the (view, pixel) keys keep 64 bits through five passes.  The views overlap
    (view k holds every row but those of bin k), so that each gives a pixel enough rows for their order to matter; the weights are
    spread over 16 decades.  Every view against the sequential loop at its touched pixels; in all 22 maps every other pixel is 0."""
    import torch

    import ordered_sum_cases as osc

    nside, nbins = 4096, 22
    cols, ipix = _ordered_view_catalogue(nside, 37, nbins, lambda rng: osc.values(rng, osc.N))
    cols = {k: cols[k] for k in ("RA", "DEC", "W", "TOM_BIN_ID")}
    m = hx.HipHealpixMapper(nside, 2, deconvolve=False)
    fields = {"WHT": hx.Weights(m, "RA", "DEC", "W")}
    base = hx.ArrayCatalog(cols, page_size=osc.N)
    torch.cuda.empty_cache()  # 35 GB of maps in ONE pass: what earlier tests left cached counts against the budget of a pass
    passes = _record_passes(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = hx.map_catalogs(fields, {k: base[f"TOM_BIN_ID!={k}"] for k in range(nbins)}, device="cuda")
    assert passes == [nbins] and list(got) == [("WHT", k) for k in range(nbins)]
    try:
        for k in range(nbins):
            keep = (cols["TOM_BIN_ID"] != k) & (cols["W"] != 0)
            wbar = got["WHT", k].dtype.metadata["wbar"]
            # (the input conditions are asserted for views 0, 11 and 21; the others get the same exact comparison without them)
            upix, wht = (osc.reference if k in (0, 11, 21) else osc.sequential)(ipix[keep], cols["W"][keep])
            osc.check_maps(got["WHT", k].tensor, upix, wht / wbar, 0.0, f"view {k}")
    finally:
        del got
        torch.cuda.empty_cache()
