"""Field types, get_masks, ArrayCatalog and the map_catalogs driver on the host: the hx_catmap context is replaced by a numpy
restatement (the oracle's in-order map_values, moments with np.sum), so keys, order, include / exclude, progress, errors, warnings,
normalisation and metadata are checked against the reference's outputs (tests/golden/reference_fields.npz) without a GPU."""

import warnings

import numpy as np
import pytest

import heracles_amd as hx
from heracles_amd import mapping as mp

from fields_cases import catalogs, fields, given_nbar, load
from oracle import hxoracle as ho


class NpCatMap:
    """numpy stand-in for mapping._CatMap (hx_catmap_*)."""

    created = 0

    def __init__(self, page_size, ncols, desc, maps):
        NpCatMap.created += 1
        self.desc = np.asarray(desc, dtype=int).reshape(-1, 7)
        self.maps = maps
        self.mom = np.zeros((len(maps), 4))
        self.bad = np.zeros((len(maps), 6), dtype=np.int64)

    def page(self, n, cols):
        for f, (kind, ns, lo, la, v, im, w) in enumerate(self.desc):
            wv = cols[w] if w >= 0 else np.ones(n)
            keep = np.ones(n, bool) if kind == mp._POSITIONS else wv != 0
            sel = [cols[c][keep] if c >= 0 else None for c in (lo, la, v, im)]
            ww = wv[keep]
            for k, a in enumerate(sel + [ww]):
                if a is not None:
                    self.bad[f, k] += np.isnan(a).sum()
            lon, lat = sel[0], sel[1]
            ok = np.isfinite(lon) & (np.abs(lat) <= 90)
            self.bad[f, 5] += (~ok).sum()
            rows = [ww] if kind in (mp._POSITIONS, mp._WEIGHTS) else [sel[2] * ww] if kind == mp._SCALAR else [sel[2] * ww, sel[3] * ww]
            m = self.maps[f].reshape(len(rows), -1)
            ho.map_values(ns, lon[ok], lat[ok], m, np.array([r[ok] for r in rows]))
            sq = sum(r * r for r in rows) if kind in (mp._SCALAR, mp._COMPLEX) else np.zeros(1)
            self.mom[f] += [keep.sum(), ww.sum(), (ww * ww).sum(), sq.sum()]

    def moments(self):
        return self.mom, self.bad

    def finish(self, f, norm, vis):
        self.maps[f] /= norm
        if vis is not None:
            self.maps[f] -= vis

    def close(self):
        pass


def np_visibility(catalog, nside, device, message):
    vis = np.asarray(catalog.visibility, dtype=np.float64)
    if vis.size != 12 * nside**2:
        warnings.warn(message)
        vis = ho.ud_grade(vis, nside)
    return vis.copy()


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setattr(mp, "_CatMap", NpCatMap)
    monkeypatch.setattr(mp, "_new_map", lambda nrow, npix, device: np.zeros((nrow, npix) if nrow > 1 else npix))
    monkeypatch.setattr(mp, "_device_of", lambda device: "cpu")
    monkeypatch.setattr(mp, "_visibility_on", np_visibility)


@pytest.fixture(scope="module")
def golden():
    return load()


# ---- fields ---------------------------------------------------------------------------------------------------------------------------

def test_column_parsing_and_errors():
    m = hx.HipHealpixMapper(8, 12)
    assert hx.Positions(m, "ra", "dec").columns == ("ra", "dec", None)
    assert hx.Spin2Field(m, "ra", "dec", "g1", "g2", "w").columns == ("ra", "dec", "g1", "g2", "w")
    assert hx.Visibility(m).columns is None
    with pytest.raises(ValueError) as e:
        hx.Positions(m, "ra")
    assert str(e.value) == "field of type 'Positions' accepts 2 to 3 columns (longitude, latitude, [weight]), received 1"
    with pytest.raises(ValueError) as e:
        hx.ScalarField(m, "a", "b", "c", "d", "e")
    assert str(e.value) == "field of type 'ScalarField' accepts 3 to 4 columns (longitude, latitude, value, [weight]), received 5"
    with pytest.raises(ValueError) as e:
        hx.Visibility(m, "a")
    assert str(e.value) == "field of type 'Visibility' accepts 0 columns, received 1"
    with pytest.raises(ValueError, match="^no mapper for field$"):
        hx.Weights(None, "a", "b").mapper_or_error
    with pytest.raises(ValueError, match="^no columns for field$"):
        hx.Weights(m).columns_or_error

    class Custom(hx.Field):
        uses = "x", "[y]", "[z]"

    assert Custom(m, "a").columns == ("a", None, None)
    with pytest.raises(ValueError) as e:
        Custom(m).spin
    assert str(e.value) == "field of type 'Custom' has undefined spin weight"


def test_spin_mask_and_aliases():
    m = hx.HipHealpixMapper(8, 12)
    assert hx.Shears is hx.Spin2Field and hx.Ellipticities is hx.Spin2Field
    assert [f(m).spin for f in (hx.Positions, hx.ScalarField, hx.ComplexField, hx.Spin2Field, hx.Visibility, hx.Weights)] == [0, 0, 0, 2, 0, 0]
    p = hx.Positions(m, "a", "b", nbar=3.0, overdensity=False, mask="V")
    assert (p.mask, p.nbar, p.overdensity, p.mapper) == ("V", 3.0, False, m)
    p.nbar = 4.0
    assert p.nbar == 4.0


def test_get_masks():
    m = hx.HipHealpixMapper(8, 12)
    fields = {"POS": hx.Positions(m, "a", "b", mask="V"), "SHE": hx.Shears(m, "a", "b", "c", "d", mask="W"), "X": hx.Weights(m, "a", "b")}
    assert hx.get_masks(fields) == ["V", "W"]
    assert hx.get_masks(fields, comb=2) == [("V", "V"), ("V", "W"), ("W", "W")]
    assert hx.get_masks(fields, comb=2, include=[("POS", "SHE")]) == [("V", "W")]
    assert hx.get_masks(fields, exclude=[("SHE",)]) == ["V"]
    assert hx.get_masks(fields, include=[("SHE_E",)], append_eb=True) == ["W"]
    assert hx.get_masks(fields, include=[("SHE_E",)]) == []
    assert hx.get_masks(fields, comb=2, include=[("POS", "SHE_B")], append_eb=True) == [("V", "W")]


# ---- catalogue --------------------------------------------------------------------------------------------------------------------

def test_array_catalog():
    rng = np.random.default_rng(1)
    arr = np.zeros(25, dtype=[("lon", "f8"), ("lat", "f8"), ("w", "f8")])
    arr["lon"] = rng.uniform(0, 360, 25)
    cat = hx.ArrayCatalog(arr, page_size=10, metadata={"catalog": "x", "z": 1})
    assert cat.size == 25 and cat.fsky is None and dict(cat.metadata) == {"catalog": "x", "z": 1}
    assert [p.size for p in cat] == [10, 10, 5]
    cat.visibility = np.array([0.0, 1.0, 1.0, 0.5])
    assert cat.fsky == 0.625
    assert dict(hx.ArrayCatalog({"a": np.ones(3)}).metadata) == {"catalog": None}
    page = next(iter(hx.ArrayCatalog({"a": np.array([1.0, np.nan, 2.0]), "b": np.arange(3.0)})))
    with pytest.raises(ValueError, match='invalid values in column "a"'):
        page.get("a")
    np.testing.assert_array_equal(page["-b"], [-0.0, -1.0, -2.0])
    page.delete(page["a"] != page["a"])
    assert page.size == 2 and page.get("a").tolist() == [1.0, 2.0]
    with pytest.raises(ValueError, match="inconsistent row length"):
        hx.ArrayCatalog({"a": np.ones(3), "b": np.ones(2)})


# ---- map_catalogs ---------------------------------------------------------------------------------------------------------------------

def test_golden_parity_host(host, golden):
    g, settings, meta, warns = golden
    cats = catalogs(g, settings)
    flds = fields(settings)
    got = {}
    for cname, cat in cats.items():
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got.update(hx.map_catalogs(flds, {cname: cat}))
        assert sorted(str(r.message) for r in rec) == warns[cname]
    assert [list(k) for k in got] == settings["keys"]
    for (fname, cname), m in got.items():
        want = g[f"map/{fname}/{cname}"]
        assert isinstance(m, np.ndarray) and m.shape == want.shape
        if given_nbar(settings, fname):
            np.testing.assert_array_equal(m, want)
        else:
            np.testing.assert_allclose(m, want, rtol=0, atol=1e-13 * np.abs(want).max())
        md, wmd = dict(m.dtype.metadata), meta[f"{fname}/{cname}"]
        assert set(md) == set(wmd)
        for k, v in wmd.items():
            if isinstance(v, float):
                assert md[k] == pytest.approx(v, rel=1e-12), (fname, cname, k)
            else:
                assert md[k] == v, (fname, cname, k)


def test_keys_order_filters_progress_and_out(host, golden):
    g, settings, _, _ = golden
    cats = catalogs(g, settings)
    flds = fields(settings)

    class Progress:
        def __init__(self):
            self.calls = []

        def update(self, current, total):
            self.calls.append((current, total))

    prog = Progress()
    out = {}
    res = hx.map_catalogs(flds, cats, out=out, include=[("POS",), ("SHE", "cat2"), ("VIS",)], exclude=[("VIS", "cat1")],
                          progress=prog, parallel=True)
    assert res is out
    assert list(out) == [("POS", "cat1"), ("POS", "cat2"), ("SHE", "cat2"), ("VIS", "cat2")]
    total = len(flds) * len(cats)
    assert prog.calls == [(0, total), (1, total), (2, total), (3, total), (4, total)]
    both = hx.map_catalogs(flds, cats)
    assert list(both) == [(f, c) for c in cats for f in flds]
    assert isinstance(both, hx.TocDict)


def test_one_pass_per_catalogue(host, golden):
    g, settings, _, _ = golden
    cats = catalogs(g, settings)
    flds = {k: v for k, v in fields(settings).items() if k in ("POS", "SHE", "WHT", "VAL")}
    NpCatMap.created = 0
    hx.map_catalogs(flds, cats)
    assert NpCatMap.created == 2 and all(c.pages_read == 1 for c in cats.values())


def test_errors(host, golden):
    g, settings, _, _ = golden
    cats = catalogs(g, settings)
    m = hx.HipHealpixMapper(8, 12)
    novis = {"c": cats["cat1"]}
    cats["cat1"].visibility = None
    with pytest.raises(ValueError, match="^cannot compute density contrast: no visibility in catalog$"):
        hx.map_catalogs({"P": hx.Positions(m, "lon", "lat")}, novis)
    with pytest.raises(ValueError, match="^no visibility in catalog$"):
        hx.map_catalogs({"V": hx.Visibility(m)}, novis)
    assert cats["cat1"].pages_read == 0
    hx.map_catalogs({"P": hx.Positions(m, "lon", "lat", overdensity=False)}, novis)  # fsky = 1 without a visibility
    with pytest.raises(ValueError, match="^no mapper for field$"):
        hx.map_catalogs({"W": hx.Weights(None, "lon", "lat")}, novis)
    with pytest.raises(ValueError, match="^no columns for field$"):
        hx.map_catalogs({"W": hx.Weights(m)}, novis)
    with pytest.raises(TypeError, match="'dict'"):
        hx.map_catalogs({"W": {}}, novis)

    class OtherMapper:
        nside = 8

    with pytest.raises(NotImplementedError, match="OtherMapper"):
        hx.map_catalogs({"W": hx.Weights(OtherMapper(), "lon", "lat")}, novis)
    with pytest.raises(NotImplementedError, match="HipDiscreteMapper"):
        hx.map_catalogs({"W": hx.Weights(hx.HipDiscreteMapper(12), "lon", "lat")}, novis)
    # NaN on a row the field keeps: the reference's page.get error
    with pytest.raises(ValueError, match='^invalid values in column "val"$'):
        hx.map_catalogs({"S": hx.ScalarField(m, "lon", "lat", "val")}, novis)
    cats["cat2"].cols["lat"][5] = 91.0
    with pytest.raises(ValueError, match="latitude outside"):
        hx.map_catalogs({"W": hx.Weights(m, "lon", "lat", "w")}, {"c": cats["cat2"]})


def test_reference_field_objects(host, golden):
    """Objects of the reference's classes are recognised by class name along the MRO and read through their properties."""
    g, settings, meta, _ = golden
    cats = catalogs(g, settings)
    ours = fields(settings)

    def stand_in(name, f):
        base = type(name if name != "Spin2Field" else "ComplexField", (), {})
        cls = type(name, (base,), {})
        obj = cls()
        obj.mapper, obj.columns, obj.spin = f.mapper, f.columns, f.spin
        if isinstance(f, hx.Positions):
            obj.overdensity, obj.nbar = f.overdensity, f.nbar
        return obj

    theirs = {k: stand_in(type(f).__name__, f) for k, f in ours.items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = hx.map_catalogs(ours, {"cat1": cats["cat1"]})
        b = hx.map_catalogs(theirs, {"cat1": cats["cat1"]})
    assert list(a) == list(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
        assert dict(a[k].dtype.metadata) == dict(b[k].dtype.metadata)


def test_chunks_respect_context_limits():
    m8, m16 = hx.HipHealpixMapper(8, 12), hx.HipHealpixMapper(16, 24)
    items = [mp._Item((f"F{i}", 0), None, mp._SCALAR, m8 if i % 2 else m16, ("lon", "lat"), f"v{i}", None, "w") for i in range(19)]
    chunks = list(mp._chunks(items))
    assert [it for c, _ in chunks for it in c] == items
    for chunk, cols in chunks:
        assert len(chunk) <= mp._MAX_FIELDS and len(cols) <= mp._MAX_COLUMNS
        assert len({(it.mapper.nside, *it.lonlat) for it in chunk}) <= mp._MAX_GROUPS
        assert all(c in cols for it in chunk for c in (*it.lonlat, it.value, it.weight))
