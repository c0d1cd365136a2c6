"""The catalog_alms driver on the host: the hx_catalm context is replaced by a numpy restatement on the oracle's direct sum
(discrete_cases.NpCatAlm), so keys, order, include / exclude, progress, errors, warnings, normalisation, metadata and the split into
passes are checked against the reference's outputs with its DiscreteMapper (tests/golden/reference_discrete.npz) without a GPU."""

import warnings

import numpy as np
import pytest

import heracles_amd as hx
from heracles_amd import mapping as mp

from discrete_cases import NpCatAlm, catalogs, check_meta, fields, host_patches, load


@pytest.fixture
def host(monkeypatch):
    host_patches(monkeypatch)


@pytest.fixture(scope="module")
def golden():
    return load()


def test_golden_parity_host(host, golden):
    g, settings, meta, warns = golden
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
        want = g[f"alm/{fname}/{cname}"]
        assert isinstance(a, np.ndarray) and a.shape == want.shape and a.dtype == np.complex128
        np.testing.assert_allclose(a, want, rtol=0, atol=1e-13 * float(g[f"scale/{fname}/{cname}"]))
        check_meta(dict(a.dtype.metadata), meta[f"{fname}/{cname}"], (fname, cname))


def test_complex64_mapper_casts_at_the_end(host, golden):
    g, settings, meta, _ = golden
    cats = catalogs(g, settings, only=["cat2"])
    flds = {k: v for k, v in fields(settings, dtype=np.complex64).items() if k in ("SHE", "WHT", "VIS")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = hx.catalog_alms(flds, cats)
    for (fname, cname), a in got.items():
        want = g[f"alm/{fname}/{cname}"]
        assert a.dtype == np.complex64 and a.shape == want.shape
        # float32 rounding of a float64 result: 2^-24 of each part
        np.testing.assert_allclose(a, want, rtol=0, atol=1.2e-7 * np.abs(want).max())
        check_meta(dict(a.dtype.metadata), meta[f"{fname}/{cname}"], (fname, cname))


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
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = hx.catalog_alms(flds, cats, out=out, include=[("POS",), ("SHE", "cat2"), ("VIS",)], exclude=[("VIS", "cat1")], progress=prog)
        both = hx.catalog_alms(flds, cats)
    assert res is out
    assert list(out) == [("POS", "cat1"), ("POS", "cat2"), ("SHE", "cat2"), ("VIS", "cat2")]
    total = len(flds) * len(cats)
    assert prog.calls == [(0, total), (1, total), (2, total), (3, total), (4, total)]
    assert list(both) == [(f, c) for c in cats for f in flds]
    assert isinstance(both, hx.TocDict)


def test_one_pass_per_catalogue_and_budget_split(host, golden, monkeypatch):
    g, settings, _, _ = golden
    flds = {k: v for k, v in fields(settings).items() if k in ("POS", "SHE", "WHT", "VAL")}  # two band limits: two groups
    cats = catalogs(g, settings)
    NpCatAlm.created = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        whole = hx.catalog_alms(flds, cats)
    assert NpCatAlm.created == 2 and all(c.pages_read == 1 for c in cats.values())
    # lmax 12: grids of 64^2 float64 = 32768 bytes per component, scratch 16 * 13 * (64 + 96) = 33280: one field fits 80000, two do not
    two = {k: flds[k] for k in ("POS", "WHT")}
    monkeypatch.setattr(mp, "_map_budget", lambda device: 80000)
    cats = catalogs(g, settings, only=["cat1"])
    NpCatAlm.created = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        split = hx.catalog_alms(two, cats)
    assert NpCatAlm.created == 2 and cats["cat1"].pages_read == 2
    for k in split:
        np.testing.assert_array_equal(split[k], whole[k])
    monkeypatch.setattr(mp, "_map_budget", lambda device: 60000)
    with pytest.raises(MemoryError, match="'POS'.*32768.*33280.*60000"):
        hx.catalog_alms(two, cats)


def test_errors(host, golden):
    g, settings, _, _ = golden
    cats = catalogs(g, settings)
    m = hx.HipDiscreteMapper(12)
    cat1 = cats["cat1"]
    novis = {"c": cat1}
    vis = cat1.visibility
    cat1.visibility = None
    with pytest.raises(ValueError, match="^cannot compute density contrast: no visibility in catalog$"):
        hx.catalog_alms({"P": hx.Positions(m, "lon", "lat")}, novis)
    with pytest.raises(ValueError, match="^no visibility in catalog$"):
        hx.catalog_alms({"V": hx.Visibility(m)}, novis)
    with pytest.raises(ValueError, match="^no mapper for field$"):
        hx.catalog_alms({"W": hx.Weights(None, "lon", "lat")}, novis)
    with pytest.raises(ValueError, match="^no columns for field$"):
        hx.catalog_alms({"W": hx.Weights(m)}, novis)
    with pytest.raises(TypeError, match="'dict'"):
        hx.catalog_alms({"W": {}}, novis)

    class OtherMapper:
        lmax = 12

    with pytest.raises(NotImplementedError, match="OtherMapper"):
        hx.catalog_alms({"W": hx.Weights(OtherMapper(), "lon", "lat")}, novis)
    with pytest.raises(NotImplementedError, match="map_catalogs"):
        hx.catalog_alms({"W": hx.Weights(hx.HipHealpixMapper(8, 12), "lon", "lat")}, novis)
    # a visibility that is a map, where a field reads it
    cat1.visibility = np.ones(12 * 8 * 8)
    with pytest.raises(ValueError, match="alms"):
        hx.catalog_alms({"P": hx.Positions(m, "lon", "lat")}, novis)
    with pytest.raises(ValueError, match="alms"):
        hx.catalog_alms({"V": hx.Visibility(m)}, novis)
    assert cat1.pages_read == 0
    hx.catalog_alms({"W": hx.Weights(m, "lon", "lat", "w")}, novis)  # (fsky is its mean: no field reads it as alms)
    cat1.visibility = None
    hx.catalog_alms({"P": hx.Positions(m, "lon", "lat", overdensity=False)}, novis)  # fsky = 1 without a visibility
    cat1.visibility = vis
    # map_catalogs keeps refusing the discrete mapper, and now says where to go
    with pytest.raises(NotImplementedError, match="HipDiscreteMapper.*catalog_alms"):
        hx.map_catalogs({"W": hx.Weights(m, "lon", "lat")}, novis)
    # NaN on a row the field keeps: the reference's page.get error
    with pytest.raises(ValueError, match='^invalid values in column "val"$'):
        hx.catalog_alms({"S": hx.ScalarField(m, "lon", "lat", "val")}, novis)
    cats["cat2"].cols["lat"][5] = 91.0
    with pytest.raises(ValueError, match="latitude outside"):
        hx.catalog_alms({"W": hx.Weights(m, "lon", "lat", "w")}, {"c": cats["cat2"]})


def test_fsky_of_a_complex_visibility():
    vis = np.zeros(91, dtype=complex)
    vis[0] = 0.7 * (4 * np.pi) ** 0.5
    vis[5] = 3.0 + 1.0j
    cat = hx.ArrayCatalog({"a": np.ones(3)}, visibility=vis)
    assert cat.fsky == pytest.approx(0.7, rel=1e-15)
    import torch

    cat.visibility = torch.as_tensor(vis)
    assert cat.fsky == pytest.approx(0.7, rel=1e-15)
    cat.visibility = np.array([0.0, 1.0, 1.0, 0.5])  # a map: the mean, as before
    assert cat.fsky == 0.625
    assert cat.where(np.array([True, False, True])).fsky == 0.625


def test_transform_passes_alms_and_metadata_through(host, golden):
    """HipDiscreteMapper.transform is the identity: numpy alms and DeviceArrays come back as they are, metadata included."""
    import torch

    g, settings, _, _ = golden
    cats = catalogs(g, settings, only=["cat2"])
    flds = {k: v for k, v in fields(settings).items() if k in ("SHE", "WHT")}
    alms = hx.catalog_alms(flds, cats)
    wrapped = {k: hx.DeviceArray(torch.as_tensor(np.array(a)), dict(a.dtype.metadata)) for k, a in alms.items()}
    for data in (alms, wrapped):
        out = hx.transform(flds, data)
        assert list(out) == list(data)
        for k in data:
            assert out[k] is data[k]
            assert dict(out[k].dtype.metadata) == dict(alms[k].dtype.metadata)
    assert out["SHE", "cat2"].dtype.metadata["spin"] == 2


def test_chunks_group_by_band_limit():
    m12, m24 = hx.HipDiscreteMapper(12), hx.HipDiscreteMapper(24)
    items = [mp._Item((f"F{i}", 0), None, mp._SCALAR, m12 if i % 2 else m24, ("lon", "lat"), f"v{i}", None, "w") for i in range(19)]
    chunks = list(mp._chunks(items, fits=lambda fs: len(fs) <= 3))
    assert [it for c, _ in chunks for it in c] == items
    assert all(len(c) <= 3 for c, _ in chunks)
    for chunk, cols in mp._chunks(items):
        assert len(chunk) <= mp._MAX_FIELDS and len(cols) <= mp._MAX_COLUMNS
        assert len({(it.mapper.lmax, *it.lonlat) for it in chunk}) <= mp._MAX_GROUPS
