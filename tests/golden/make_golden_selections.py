"""Golden vectors for catalogue views, selections and filters mapped by map_catalogs (heracles/catalog/base.py:204-466,
heracles/catalog/filters.py, heracles/catalog/fits.py:34-36, heracles/mapping.py:61-110).

Run ONCE in the build container (needs /root/reference; never on the GPU box):

    python tests/golden/make_golden_selections.py

The reference is imported through the shim of make_golden_fields.py, with the `healpy` stub given `get_nside` and an `ang2pix` on
the oracle's `ang2pix_ring` that raises healpy's ValueError for an invalid position.  The base catalogue is the reference's
ArrayCatalog; string selections are applied with the reference's `rowfilter` (the rule of its FITS catalogue), masks as the
ArrayCatalog applies them.  Every view is mapped on its own with the reference's map_catalogs; inputs, maps, metadata, warning texts
and errors are stored.
"""

import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_fields as mgf  # noqa: E402

OUT = os.path.join(HERE, "reference_selections.npz")
COLS = ("lon", "lat", "w", "e1", "e2", "TOM_BIN_ID", "Z", "Q")
PAGE = 700
FP_NSIDE = 4

# name, type, nside, columns, keyword arguments
FIELDS = [
    ("POS", "Positions", 16, ["lon", "lat"], {}),
    ("NUM", "Positions", 8, ["lon", "lat"], {"overdensity": False, "nbar": 5.0}),
    ("SHE", "Spin2Field", 16, ["lon", "lat", "e1", "-e2", "w"], {}),
    ("WHT", "Weights", 8, ["lon", "lat", "w"], {}),
    ("VIS", "Visibility", 16, [], {}),
]

# key -> list of selection terms: "s:<expr>" a row-filter string, "m:<expr>" a mask computed from the columns with numpy; "vis"
# per view: None (the base's) or an nside
VIEWS = {
    "b0": (["s:TOM_BIN_ID==0"], 16),
    "b1": (["s:TOM_BIN_ID==1"], 8),
    "b2": (["m:TOM_BIN_ID==2"], None),
    "all": ([], None),
    "vv": (["m:Z > 1", "s:TOM_BIN_ID < 3"], None),
    "or": (["s:(TOM_BIN_ID==0) | (TOM_BIN_ID==3)"], None),
    "ne": (["s:Q != 0.5"], None),
    "lt": (["s:(Q < 0.5) & (TOM_BIN_ID >= 1)"], None),
}
# error cases on a second catalogue without filters: a NaN in bin 3 only; an invalid latitude in bin 2 under a footprint filter
ERR_VIEWS = {"ok": ["s:TOM_BIN_ID==0"], "nan": ["s:TOM_BIN_ID==3"]}


def healpy_stub(ho):
    hp = sys.modules["healpy"]

    def get_nside(m):
        return int(round((len(m) / 12) ** 0.5))

    def ang2pix(nside, lon, lat, lonlat=False):
        lon, lat = np.asarray(lon, dtype=float), np.asarray(lat, dtype=float)
        theta = np.pi / 2 - np.radians(lat)
        if not np.all((theta >= 0) & (theta <= np.pi + 1e-5)):
            raise ValueError("THETA is out of range [0,pi]")
        return ho.ang2pix_ring(nside, lon, lat)

    hp.get_nside, hp.ang2pix = get_nside, ang2pix


def make_columns(rng, n):
    c = {
        "lon": rng.uniform(0.0, 360.0, n),
        "lat": np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))),
        "w": rng.uniform(0.2, 2.0, n),
        "e1": 0.3 * rng.standard_normal(n),
        "e2": 0.3 * rng.standard_normal(n),
        "TOM_BIN_ID": rng.integers(0, 4, n).astype(np.float64),
        "Z": rng.uniform(0.0, 2.0, n),
        "Q": rng.choice([0.0, 0.5, 1.0], n),
    }
    zero = rng.random(n) < 0.08
    c["w"][zero] = 0.0
    c["e1"][zero & (rng.random(n) < 0.5)] = np.nan  # kept by the weighted filter (weight 0), dropped by the fields
    c["e2"][rng.choice(np.flatnonzero(~zero), 6, replace=False)] = np.nan  # removed by the weighted filter
    c["Z"][rng.choice(n, 9, replace=False)] = np.nan  # removed by InvalidValueFilter("Z"), which warns
    c["Q"][rng.choice(n, 40, replace=False)] = np.nan  # no filter: `!=` keeps these rows, `<` drops them
    return c


def reference_catalog(h, cols, filters, vis):
    """The reference's ArrayCatalog, string terms applied with the reference's rowfilter."""
    from heracles.catalog.fits import rowfilter

    arr = np.empty(len(cols["lon"]), dtype=[(k, "f8") for k in COLS])
    for k in COLS:
        arr[k] = cols[k]

    class Cat(h.array.ArrayCatalog):
        def _join(self, *where):
            return tuple(where)

        def _mask(self, selection):
            terms = selection if isinstance(selection, tuple) else (selection,)
            mask = np.ones(len(self._arr), bool)
            for t in terms:
                if isinstance(t, tuple):
                    mask &= self._mask(t)
                elif isinstance(t, str):
                    mask &= rowfilter(self._arr, t)
                else:
                    mask &= t
            return mask

        def _pages(self, selection):
            yield from super()._pages(None if selection is None else self._mask(selection))

        def _size(self, selection):
            return len(self._arr) if selection is None else int(self._mask(selection).sum())

    cat = Cat(arr)
    cat.page_size = PAGE
    cat.visibility = vis
    cat.label = "base"
    for f in filters:
        cat.add_filter(f)
    return cat


def view_of(cat, terms, cols, vis):
    if not terms:
        return cat
    sel = []
    for t in terms:
        kind, expr = t.split(":", 1)
        sel.append(expr if kind == "s" else eval(expr, None, dict(cols)))
    view = cat.where(sel[0], vis)
    for s in sel[1:]:
        view = view[s]
    return view


def main():
    from oracle import hxoracle as ho

    h = mgf.shimmed()
    healpy_stub(ho)
    import importlib

    flt = importlib.import_module("heracles.catalog.filters")
    rng = np.random.default_rng(20261017)
    mappers = {ns: mgf.oracle_mapper(h, ns) for ns in (8, 16)}
    mgf.LMAX.setdefault(8, 12)
    out, meta, warns, errors = {}, {}, {}, {}
    cols = make_columns(rng, 3000)
    for k in COLS:
        out[f"col/{k}"] = cols[k]
    fp = (rng.random(12 * FP_NSIDE**2) < 0.8).astype(np.float64)
    base_vis = rng.uniform(0.5, 1.0, 12 * 16**2)
    out["fp"], out["vis/base"] = fp, base_vis
    filters = [flt.InvalidValueFilter("e1", "e2", weight="w", warn=False), flt.InvalidValueFilter("Z"),
               flt.FootprintFilter(fp, "lon", "lat")]
    cat = reference_catalog(h, cols, filters, base_vis)
    fields = {name: getattr(h.fields, typ)(mappers[ns], *c, **kw) for name, typ, ns, c, kw in FIELDS}
    for key, (terms, vns) in VIEWS.items():
        vis = None
        if vns is not None:
            vis = rng.uniform(0.5, 1.0, 12 * vns**2)
            out[f"vis/{key}"] = vis
        view = view_of(cat, terms, cols, vis)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            maps = h.mapping.map_catalogs(fields, {key: view})
        warns[key] = sorted({str(r.message) for r in rec})
        for (fname, _), m in maps.items():
            out[f"map/{fname}/{key}"] = np.asarray(m, dtype=np.float64)
            md = dict(m.dtype.metadata)
            meta[f"{fname}/{key}"] = {k: (float(v) if isinstance(v, (np.floating, float)) and not isinstance(v, bool) else v)
                                      for k, v in md.items()}
    # errors: a NaN in bin 3 and an invalid latitude in bin 2, no filters; and an invalid latitude seen by a footprint filter
    ecols = {k: v.copy() for k, v in cols.items()}
    ecols["Z"] = np.where(np.isnan(ecols["Z"]), 0.0, ecols["Z"])
    ecols["e1"] = np.where(np.isnan(ecols["e1"]), 0.0, ecols["e1"])
    ecols["e2"] = np.where(np.isnan(ecols["e2"]), 0.0, ecols["e2"])
    in3 = np.flatnonzero(ecols["TOM_BIN_ID"] == 3)
    ecols["e1"][in3[5]] = np.nan
    ecols["w"][in3[5]] = 1.0
    ecols["lat"][np.flatnonzero(ecols["TOM_BIN_ID"] == 2)[9]] = 91.0
    for k in COLS:
        out[f"ecol/{k}"] = ecols[k]
    ecat = reference_catalog(h, ecols, [], None)
    efields = {k: v for k, v in fields.items() if k in ("NUM", "SHE", "WHT")}
    for key, terms in ERR_VIEWS.items():
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                h.mapping.map_catalogs(efields, {key: view_of(ecat, terms, ecols, None)})
            errors[key] = None
        except Exception as e:  # noqa: BLE001
            errors[key] = [type(e).__name__, str(e)]
    fcat = reference_catalog(h, ecols, [flt.FootprintFilter(fp, "lon", "lat")], None)
    try:
        h.mapping.map_catalogs(efields, {"fp": view_of(fcat, ["s:TOM_BIN_ID==2"], ecols, None)})
        errors["fp"] = None
    except Exception as e:  # noqa: BLE001
        errors["fp"] = [type(e).__name__, str(e)]
    settings = {"fields": FIELDS, "views": VIEWS, "err_views": ERR_VIEWS, "page_size": PAGE, "columns": list(COLS),
                "lmax": {str(k): v for k, v in mgf.LMAX.items()}}
    out["settings"] = np.array(json.dumps(settings))
    out["metadata"] = np.array(json.dumps(meta))
    out["warnings"] = np.array(json.dumps(warns))
    out["errors"] = np.array(json.dumps(errors))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; warnings {warns}; errors {errors}")


if __name__ == "__main__":
    main()
