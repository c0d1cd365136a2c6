"""Catalogue views, selections and filters on the host, the predicate compiler of the one-pass path, and the map_catalogs driver of that
path with the hx_catmap_sel context replaced by a numpy stand-in: keys, progress, one read of the base per pass, the split under a lowered
budget, and the per-catalogue path for what the one-pass path does not take."""

import warnings

import numpy as np
import pytest

import heracles_amd as hx
from heracles_amd import mapping as mp


def _cols(n=20, seed=1):
    rng = np.random.default_rng(seed)
    return {"RA": rng.uniform(0, 360, n), "DEC": rng.uniform(-60, 60, n), "W": rng.uniform(0.5, 1, n),
            "BIN": rng.integers(0, 3, n), "Z": rng.uniform(0, 2, n)}


def _rows(pages, name):
    return np.concatenate([p[name] for p in pages]) if pages else np.zeros(0)


# ---- views and selections ----------------------------------------------------------------------------------------------------------


def test_where_and_getitem_select_rows_in_order():
    cols = _cols()
    cat = hx.ArrayCatalog(cols, page_size=4, metadata={"catalog": "cat"})
    view = cat.where("BIN == 1")
    assert isinstance(view, hx.CatalogView) and view.base is cat and view.selection == "BIN == 1"
    assert view.metadata == cat.metadata and view.label == "cat" and view.names == cat.names and view.page_size == 4
    keep = cols["BIN"] == 1
    assert view.size == keep.sum()
    pages = list(view)
    assert [p.size for p in pages] == [min(4, keep.sum() - i) for i in range(0, keep.sum(), 4)]
    np.testing.assert_array_equal(_rows(pages, "RA"), cols["RA"][keep])
    # masks, tuples and views of views join with &
    both = keep & (cols["Z"] > 1)
    for v in (cat[(keep, "Z > 1")], cat[keep]["Z > 1"], view[cols["Z"] > 1], cat.where(["BIN == 1", cols["Z"] > 1])):
        np.testing.assert_array_equal(_rows(list(v), "Z"), cols["Z"][both])
    np.testing.assert_array_equal(_rows(list(view.select(cols["Z"] > 1)), "Z"), cols["Z"][both])
    np.testing.assert_array_equal(_rows(list(cat.select("BIN == 2")), "RA"), cols["RA"][cols["BIN"] == 2])


def test_selection_forms_that_are_refused():
    cat = hx.ArrayCatalog(_cols(), page_size=4)
    for bad in (np.arange(3), [0, 1], 3, None, np.ones(20, dtype=np.int8)):
        with pytest.raises(TypeError):
            cat.where(bad)
    with pytest.raises(ValueError):
        cat.where(np.ones(5, bool))


def test_view_visibility_and_fsky():
    cat = hx.ArrayCatalog(_cols(), visibility=np.full(12, 0.5))
    view = cat["BIN == 0"]
    assert view.visibility is cat.visibility and view.fsky == 0.5
    v2 = cat.where("BIN == 0", visibility=np.full(12, 0.25))
    assert v2.fsky == 0.25
    v2.fsky = 0.3
    assert v2.fsky == 0.3
    v2.visibility = None
    assert v2.visibility is cat.visibility and v2.fsky == 0.5
    v3 = cat.where("BIN == 0", visibility=np.full(12, 0.1))["Z > 1"]  # a sub-view keeps its parent's visibility
    assert v3.fsky == pytest.approx(0.1) and v3.selection == ("BIN == 0", "Z > 1")


def test_invalid_value_filter():
    cols = _cols()
    cols["Z"][[2, 5, 9]] = np.nan
    cols["W"][5] = 0.0
    f = hx.InvalidValueFilter("Z", weight="W")
    assert repr(f) == "InvalidValueFilter('Z', weight='W', warn=True)"
    cat = hx.ArrayCatalog(cols, page_size=8)
    cat.add_filter(f)
    assert cat.filters == [f]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        pages = list(cat)
    assert {str(r.message) for r in rec} == {"WARNING: catalog contains invalid values"}
    keep = np.ones(20, bool)
    keep[[2, 9]] = False
    np.testing.assert_array_equal(_rows(pages, "RA"), cols["RA"][keep])
    cat.filters = [hx.InvalidValueFilter("Z", warn=False)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert sum(p.size for p in cat) == 17


def test_footprint_filter_takes_nside_from_size():
    f = hx.FootprintFilter(np.ones(12 * 4**2), "RA", "DEC")
    assert f.nside == 4 and f.lonlat == ("RA", "DEC") and repr(f) == "FootprintFilter(..., 'RA', 'DEC')"
    with pytest.raises(ValueError):
        hx.FootprintFilter(np.ones(100), "RA", "DEC")


# ---- the predicate compiler ----------------------------------------------------------------------------------------------------------

DT = {"BIN": np.dtype(np.int64), "Z": np.dtype(np.float64), "F32": np.dtype(np.float32), "FLAG": np.dtype(bool)}


@pytest.mark.parametrize("expr, terms", [
    ("BIN==0", [("BIN", 0, 0.0)]),
    ("(BIN != 2) & (Z < 1.5)", [("BIN", 1, 2.0), ("Z", 2, 1.5)]),
    ("(Z <= -1) & (Z > -2e3) & (BIN >= 1)", [("Z", 3, -1.0), ("Z", 4, -2000.0), ("BIN", 5, 1.0)]),
    ("BIN == 0.5", [("BIN", 0, 0.5)]),
])
def test_predicates_that_compile(expr, terms):
    assert mp._compile_predicate(expr, DT) == terms


@pytest.mark.parametrize("expr", [
    "BIN == 0 | BIN == 1", "(BIN == 0) | (BIN == 1)", "0 == BIN", "BIN == Z", "1 < Z < 2", "F32 > 0.1", "FLAG == 1", "X == 1",
    "abs(Z) < 1", "BIN == 2**60", "not valid python(", "BIN in (1, 2)", "~(BIN == 1)",
])
def test_predicates_that_fall_back(expr):
    assert mp._compile_predicate(expr, DT) is None


def test_compiled_comparisons_follow_numpy_on_nan():
    z = np.array([0.0, 1.0, np.nan, 2.0])
    ops = {0: np.equal, 1: np.not_equal, 2: np.less, 3: np.less_equal, 4: np.greater, 5: np.greater_equal}
    for expr in ("Z == 1", "Z != 1", "Z < 1", "Z <= 1", "Z > 1", "Z >= 1"):
        ((name, op, value),) = mp._compile_predicate(expr, DT)
        np.testing.assert_array_equal(ops[op](z, value), eval(expr, None, {"Z": z}))
    assert bool(np.nan != 1.0) and not bool(np.nan == 1.0)


# ---- the one-pass driver with a numpy stand-in ---------------------------------------------------------------------------------------


class NpCatMapSel:
    """Records what the driver hands to hx_catmap_sel; maps the rows of each selection with numpy (positions only)."""

    instances = []

    def __init__(self, page_size, ncols, desc, nsel, preds, pval, filters, footprints, maps):
        NpCatMapSel.instances.append(self)
        self.desc, self.nsel, self.preds, self.pval, self.filters = np.asarray(desc).reshape(-1, 7), nsel, preds, pval, filters
        self.maps, self.pages = maps, []
        self.nfield = len(self.desc)
        self.mom = np.zeros((nsel, self.nfield, 4))

    def page(self, n, cols, mask):
        self.pages.append(n)
        member = np.ones((self.nsel, n), bool) if mask is None else (mask[None, :] >> np.arange(self.nsel, dtype=np.uint32)[:, None]) & 1 == 1
        ops = [np.equal, np.not_equal, np.less, np.less_equal, np.greater, np.greater_equal]
        for (s, c, op), v in zip(self.preds, self.pval):
            member[s] &= ops[op](cols[c], v)
        for s in range(self.nsel):
            for f, (kind, ns, lo, la, *_rest) in enumerate(self.desc):
                m = member[s]
                self.mom[s, f] += [m.sum(), m.sum(), m.sum(), 0.0]
                lon, lat = cols[lo][m], cols[la][m]
                phi, theta = np.radians(lon), np.radians(90 - lat)
                pix = (np.floor(theta / np.pi * 0.999 * 12 * ns * ns)).astype(int)  # any fixed pixelisation will do here
                np.add.at(self.maps[s * self.nfield + f].reshape(-1), pix, 1.0)

    def moments(self):
        return self.mom, np.zeros((self.nsel, self.nfield, 6), np.int64), np.zeros((self.nsel, len(self.filters) + 1), np.int64)

    def finish(self, s, f, norm, vis):
        self.maps[s * self.nfield + f] /= norm

    def close(self):
        pass


@pytest.fixture
def host(monkeypatch):
    NpCatMapSel.instances = []
    monkeypatch.setattr(mp, "_CatMapSel", NpCatMapSel)
    monkeypatch.setattr(mp, "_new_map", lambda nrow, npix, device: np.zeros((nrow, npix) if nrow > 1 else npix))
    monkeypatch.setattr(mp, "_device_of", lambda device: "cpu")
    monkeypatch.setattr(mp, "_map_budget", lambda device: 1 << 40)


class Progress:
    def __init__(self):
        self.calls = []

    def update(self, current, total):
        self.calls.append((current, total))


def _fields():
    m = hx.HipHealpixMapper(2, 4, deconvolve=False)
    return {"POS": hx.Positions(m, "RA", "DEC", overdensity=False, nbar=1.0), "CNT": hx.Positions(m, "RA", "DEC", overdensity=False)}


def test_one_read_of_the_base_for_all_views(host):
    cols = _cols(n=50)
    cat = hx.ArrayCatalog(cols, page_size=16)
    views = {k: cat[f"BIN == {k}"] for k in range(3)}
    views["mask"] = cat[cols["Z"] > 1]
    views["all"] = cat
    prog = Progress()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = hx.map_catalogs(_fields(), views, progress=prog)
    (ctx,) = NpCatMapSel.instances
    assert ctx.pages == [16, 16, 16, 2] and ctx.nsel == 5
    assert [s for s, _, _ in ctx.preds] == [0, 1, 2] and ctx.pval == [0.0, 1.0, 2.0]
    assert list(out) == [(f, j) for j in views for f in ("POS", "CNT")]
    assert prog.calls == [(i, 10) for i in range(11)]
    for j, keep in {0: cols["BIN"] == 0, "mask": cols["Z"] > 1, "all": np.ones(50, bool)}.items():
        assert out["CNT", j].dtype.metadata["nbar"] == pytest.approx(keep.sum() / 48)


def test_split_under_a_lowered_budget(host, monkeypatch):
    cat = hx.ArrayCatalog(_cols(n=30), page_size=8)
    per_view = 2 * 8 * 12 * 2**2
    monkeypatch.setattr(mp, "_map_budget", lambda device: 2 * per_view + 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = hx.map_catalogs(_fields(), {k: cat[f"BIN == {k % 3}"] for k in range(5)}, include=[("POS",), ("CNT",)])
    assert [c.nsel for c in NpCatMapSel.instances] == [2, 2, 1]
    assert all(c.pages == [8, 8, 8, 6] for c in NpCatMapSel.instances)
    assert list(out) == [(f, k) for k in range(5) for f in ("POS", "CNT")]


def test_include_exclude_and_errors_in_order(host):
    cat = hx.ArrayCatalog(_cols(n=30), page_size=8)
    fields = {**_fields(), "OD": hx.Positions(hx.HipHealpixMapper(2, 4, deconvolve=False), "RA", "DEC")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = hx.map_catalogs(fields, {"a": cat["BIN == 0"], "b": cat["BIN == 1"]}, exclude=[("OD",)])
        assert list(out) == [("POS", "a"), ("CNT", "a"), ("POS", "b"), ("CNT", "b")]
        got = {}
        with pytest.raises(ValueError, match="cannot compute density contrast: no visibility in catalog"):
            hx.map_catalogs(fields, {"a": cat["BIN == 0"], "b": cat["BIN == 1"]}, out=got, include=[("POS",), ("OD", "b")])
        assert list(got) == [("POS", "a")]


def test_unknown_filters_keep_the_per_view_path(host, monkeypatch):
    cat = hx.ArrayCatalog(_cols(n=30), page_size=8)
    cat.add_filter(lambda page: None)
    assert mp._sel_base(cat["BIN == 0"]) is None
    plain = hx.ArrayCatalog(_cols(n=30), page_size=8)
    assert mp._plan_groups(_fields(), {"x": plain}, None, None) == {}
    assert set(mp._plan_groups(_fields(), {"x": plain, "y": plain["BIN == 1"]}, None, None)) == {"x", "y"}


def test_context_limits_split_or_fall_back(host):
    """Predicates beyond _MAX_PREDICATES split the pass, filters beyond _MAX_FILTERS (or checking no column) take the per-catalogue
    path, and predicate columns that would crowd out a field become mask terms."""
    cols = _cols(n=40)
    for k in range(6):
        cols[f"C{k}"] = np.arange(40.0) + k
    cat = hx.ArrayCatalog(cols, page_size=16)
    for _ in range(4):
        cat.add_filter(hx.InvalidValueFilter("Z", warn=False))
    views = {k: cat[f"(BIN == {k % 3}) & (Z >= 0.5) & (Z < 1.5)"] for k in range(22)}  # 66 predicates
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = hx.map_catalogs(_fields(), views)
    assert [c.nsel for c in NpCatMapSel.instances] == [21, 1]
    assert all(len(c.preds) <= mp._MAX_PREDICATES and len(c.filters) <= mp._MAX_FILTERS for c in NpCatMapSel.instances)
    assert list(out) == [(f, k) for k in range(22) for f in ("POS", "CNT")]
    cat.add_filter(hx.InvalidValueFilter("Z", warn=False))  # a fifth filter
    assert mp._sel_base(cat["BIN == 0"]) is None
    empty = hx.ArrayCatalog(cols, page_size=16)
    empty.add_filter(hx.InvalidValueFilter())
    assert mp._sel_base(empty["BIN == 0"]) is None
    # 14 predicate columns + RA, DEC: the 15th and 16th columns demote the later strings to mask terms
    wide = hx.ArrayCatalog({**cols, **{f"D{k}": np.arange(40.0) for k in range(14)}}, page_size=16)
    NpCatMapSel.instances = []
    views = {k: wide[f"(D{k} >= 0) & (BIN == {k % 3})"] for k in range(14)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hx.map_catalogs(_fields(), views)
    for c in NpCatMapSel.instances:
        assert len(c.desc) and max(c.desc[:, 2:].max(), 0) < mp._MAX_COLUMNS
    assert sum(c.nsel for c in NpCatMapSel.instances) == 14
    terms = mp._sel_terms(views[13], mp._dtypes(wide), [], [])
    assert terms[0]  # on its own a view compiles
