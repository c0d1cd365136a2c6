"""Golden vectors for map_catalogs and the field types (heracles/mapping.py:61-110, heracles/fields.py:197-559).

Run ONCE in the build container (needs /root/reference; never on the GPU box):

    python tests/golden/make_golden_fields.py

`heracles.fields`, `heracles.mapping` and `heracles.catalog.array` are imported through the bare-package shim of make_golden.py with
stub `fitsio` / `healpy` modules and a small asyncio-backed stand-in for `coroutines` (`sleep`, `gather`, `run`).  The mapper is a CPU
mapper built on the oracle: `hxoracle.ang2pix_ring` + `map_values` (the in-order loop) and `ud_grade`, with area = 4 pi / npix and
`create` attaching the metadata HipHealpixMapper attaches.  Only inputs (columns, visibilities, page layout, field settings) and
outputs (maps, metadata, warning texts) are stored.
"""

import asyncio
import importlib
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import ref_modules  # noqa: E402

OUT = os.path.join(HERE, "reference_fields.npz")
LMAX = {8: 12, 16: 24}
COLS = ("lon", "lat", "w", "val", "e1", "e2", "re", "im")

# name, type, nside, columns, keyword arguments
FIELDS = [
    ("POS", "Positions", 8, ["lon", "lat"], {}),
    ("POSW", "Positions", 16, ["lon", "lat", "w"], {"nbar": None}),  # nbar filled in below (close to the estimate: no warning)
    ("NUM", "Positions", 16, ["lon", "lat"], {"overdensity": False, "nbar": 100.0}),
    ("VAL", "ScalarField", 8, ["lon", "lat", "val", "w"], {}),
    ("VALU", "ScalarField", 16, ["lon", "lat", "re"], {}),
    ("SHE", "Spin2Field", 16, ["lon", "lat", "e1", "e2", "w"], {}),
    ("CPX", "ComplexField", 8, ["lon", "lat", "re", "im"], {}),
    ("WHT", "Weights", 8, ["lon", "lat", "w"], {}),
    ("WHTU", "Weights", 16, ["lon", "lat"], {}),
    ("VIS", "Visibility", 8, [], {}),
    ("VIS16", "Visibility", 16, [], {}),
]


def shimmed():
    for name in ("fitsio", "healpy"):
        sys.modules.setdefault(name, types.ModuleType(name))
    co = types.ModuleType("coroutines")

    async def sleep():
        await asyncio.sleep(0)

    async def gather(*aws):
        return await asyncio.gather(*aws)

    co.sleep, co.gather, co.run = sleep, gather, asyncio.run
    sys.modules["coroutines"] = co
    h = ref_modules()
    h.fields = importlib.import_module("heracles.fields")
    h.mapping = importlib.import_module("heracles.mapping")
    h.array = importlib.import_module("heracles.catalog.array")
    h.base = importlib.import_module("heracles.catalog.base")
    return h


def oracle_mapper(h, nside):
    from oracle import hxoracle as ho

    class OracleMapper:
        def __init__(self):
            self.nside, self.lmax, self.deconvolve = nside, LMAX[nside], False

        @property
        def area(self):
            return 4 * np.pi / (12 * nside**2)

        def create(self, *dims, spin=0):
            m = np.zeros((*dims, 12 * nside**2))
            h.core.update_metadata(m, geometry="healpix", kernel="healpix", nside=nside, lmax=self.lmax, deconv=False, spin=spin)
            return m

        def map_values(self, lon, lat, data, values, spin=0):
            ho.map_values(nside, lon, lat, data, values)

        def resample(self, data):
            return ho.ud_grade(data, nside)

    return OracleMapper()


def make_columns(rng, n):
    c = {
        "lon": rng.uniform(0.0, 360.0, n),
        "lat": np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))),
        "w": rng.uniform(0.2, 2.0, n),
        "val": rng.standard_normal(n),
        "e1": 0.3 * rng.standard_normal(n),
        "e2": 0.3 * rng.standard_normal(n),
        "re": rng.standard_normal(n),
        "im": rng.standard_normal(n),
    }
    zero = rng.random(n) < 0.08
    c["w"][zero] = 0.0
    for k in ("val", "e1", "e2"):  # NaN values on zero-weight rows: dropped before anything else
        c[k][zero] = np.nan
    return c


def paged_catalog(h, cols, page_size, empty_after, vis, label):
    """The reference's ArrayCatalog, with one empty page inserted after page `empty_after`."""
    arr = np.empty(len(cols["lon"]), dtype=[(k, "f8") for k in COLS])
    for k in COLS:
        arr[k] = cols[k]

    class Paged(h.array.ArrayCatalog):
        def _pages(self, selection):
            for i, page in enumerate(super()._pages(selection)):
                yield page
                if i == empty_after:
                    yield h.base.CatalogPage({k: np.zeros(0) for k in COLS})

    cat = Paged(arr)
    cat.page_size = page_size
    cat.visibility = vis
    cat.label = label
    return cat


def main():
    h = shimmed()
    rng = np.random.default_rng(20261016)
    mappers = {ns: oracle_mapper(h, ns) for ns in (8, 16)}
    cats = {
        "cat1": dict(n=2500, page_size=700, empty_after=1, vis_nside=16, label="cat1"),
        "cat2": dict(n=1200, page_size=1000, empty_after=0, vis_nside=8, label=None),
    }
    out = {}
    catalogs = {}
    for name, spec in cats.items():
        cols = make_columns(rng, spec["n"])
        vis = rng.uniform(0.5, 1.0, 12 * spec["vis_nside"] ** 2)
        vis[rng.random(vis.size) < 0.2] = 0.0
        catalogs[name] = paged_catalog(h, cols, spec["page_size"], spec["empty_after"], vis, spec["label"])
        for k in COLS:
            out[f"{name}/col/{k}"] = cols[k]
        out[f"{name}/vis"] = vis
    # POSW's nbar: the estimate of cat1, slightly perturbed (bit-exact maps where nbar is given)
    c1 = catalogs["cat1"]
    w = out["cat1/col/w"]
    fields_spec = []
    for name, typ, ns, cols, kw in FIELDS:
        kw = dict(kw)
        if name == "POSW":
            kw["nbar"] = float(len(w) * w.mean() / c1.fsky / (12 * ns**2)) * 1.001
        fields_spec.append([name, typ, ns, cols, kw])
    fields = {name: getattr(h.fields, typ)(mappers[ns], *cols, **kw) for name, typ, ns, cols, kw in fields_spec}
    warns = {}
    maps = {}
    for cname, cat in catalogs.items():
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            maps.update(h.mapping.map_catalogs(fields, {cname: cat}))
        warns[cname] = sorted(str(r.message) for r in rec)
    meta = {}
    for (fname, cname), m in maps.items():
        out[f"map/{fname}/{cname}"] = np.asarray(m, dtype=np.float64)
        md = dict(m.dtype.metadata)
        meta[f"{fname}/{cname}"] = {k: (float(v) if isinstance(v, (np.floating, float)) and not isinstance(v, bool) else v) for k, v in md.items()}
    settings = {"fields": fields_spec, "catalogs": cats, "lmax": {str(k): v for k, v in LMAX.items()}, "columns": list(COLS),
                "keys": [list(k) for k in maps]}
    out["settings"] = np.array(json.dumps(settings))
    out["metadata"] = np.array(json.dumps(meta))
    out["warnings"] = np.array(json.dumps(warns))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(maps)} maps; warnings {warns}")


if __name__ == "__main__":
    main()
