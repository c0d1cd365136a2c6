"""Golden vectors for catalog_alms: the reference's map_catalogs with its DiscreteMapper (heracles/fields.py:197-559 over
heracles/ducc.py:40-162).

Run ONCE in the build container (needs /root/reference; never on the GPU box):

    python tests/golden/make_golden_discrete.py

`heracles.fields`, `heracles.mapping`, `heracles.catalog.array` and `heracles.ducc` are imported through the shim of
make_golden_fields.py, plus a stub `ducc0` whose `sht.adjoint_synthesis_general(map, spin, lmax, loc, epsilon, nthreads)` is the
oracle's direct sum `hxoracle.points2alm(loc[:, 0], loc[:, 1], map, lmax, spin)`.  The reference's own DiscreteMapper does the rest:
`create`, the lon / lat conversion, `resample`.  Only inputs (columns, visibility alms, page layout, field settings) and outputs (alms,
metadata, warning texts, and the scale the error of a comparison goes with) are stored.
"""

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
from make_golden_fields import COLS, paged_catalog, shimmed  # noqa: E402

OUT = os.path.join(HERE, "reference_discrete.npz")
VIS_LMAX = 24

# name, type, lmax, columns, keyword arguments: the cases of reference_fields.npz with lmax 12 / 24 for nside 8 / 16
FIELDS = [
    ("POS", "Positions", 12, ["lon", "lat"], {}),
    ("POSW", "Positions", 24, ["lon", "lat", "w"], {"nbar": None}),  # nbar filled in below (close to the estimate: no warning)
    ("NUM", "Positions", 24, ["lon", "lat"], {"overdensity": False, "nbar": 100.0}),
    ("VAL", "ScalarField", 12, ["lon", "lat", "val", "w"], {}),
    ("VALU", "ScalarField", 24, ["lon", "lat", "re"], {}),
    ("SHE", "Spin2Field", 24, ["lon", "lat", "e1", "e2", "w"], {}),
    ("CPX", "ComplexField", 12, ["lon", "lat", "re", "im"], {}),
    ("WHT", "Weights", 12, ["lon", "lat", "w"], {}),
    ("WHTU", "Weights", 24, ["lon", "lat"], {}),
    ("VIS", "Visibility", 12, [], {}),
    ("VIS24", "Visibility", 24, [], {}),
]


def stub_ducc0():
    from oracle import hxoracle as ho

    ducc0 = types.ModuleType("ducc0")
    ducc0.sht = types.ModuleType("ducc0.sht")

    def adjoint_synthesis_general(*, map, spin, lmax, loc, epsilon, nthreads=0):
        return ho.points2alm(loc[:, 0], loc[:, 1], map, lmax, spin)

    ducc0.sht.adjoint_synthesis_general = adjoint_synthesis_general
    sys.modules["ducc0"], sys.modules["ducc0.sht"] = ducc0, ducc0.sht


def make_columns(rng, n):
    c = {
        "lon": rng.uniform(-180.0, 540.0, n),
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


def visibility_alm(rng, lmax):
    n = (lmax + 1) * (lmax + 2) // 2
    vis = 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    vis[: lmax + 1] = vis[: lmax + 1].real  # m = 0
    vis[0] = 0.7 * (4 * np.pi) ** 0.5
    return vis


def main():
    h = shimmed()
    stub_ducc0()
    ducc = importlib.import_module("heracles.ducc")
    rng = np.random.default_rng(20261017)
    mappers = {lmax: ducc.DiscreteMapper(lmax) for lmax in (12, 24)}
    cats = {
        "cat1": dict(n=2500, page_size=700, empty_after=1, label="cat1"),
        "cat2": dict(n=1200, page_size=1000, empty_after=0, label=None),
    }
    out = {}
    catalogs = {}
    for name, spec in cats.items():
        cols = make_columns(rng, spec["n"])
        vis = visibility_alm(rng, VIS_LMAX)
        catalogs[name] = paged_catalog(h, cols, spec["page_size"], spec["empty_after"], vis, spec["label"])
        for k in COLS:
            out[f"{name}/col/{k}"] = cols[k]
        out[f"{name}/vis"] = vis
    # POSW's nbar: the estimate of cat1 (area = 1: npix = 4 pi), slightly perturbed
    w = out["cat1/col/w"]
    fields_spec = []
    for name, typ, lmax, cols, kw in FIELDS:
        kw = dict(kw)
        if name == "POSW":
            kw["nbar"] = float(len(w) * w.mean() / catalogs["cat1"].fsky / (4 * np.pi)) * 1.001
        fields_spec.append([name, typ, lmax, cols, kw])
    fields = {name: getattr(h.fields, typ)(mappers[lmax], *cols, **kw) for name, typ, lmax, cols, kw in fields_spec}
    warns = {}
    alms = {}
    for cname, cat in catalogs.items():
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            alms.update(h.mapping.map_catalogs(fields, {cname: cat}))
        warns[cname] = sorted(str(r.message) for r in rec)
    meta = {}
    for (fname, cname), a in alms.items():
        a = np.asarray(a, dtype=np.complex128)
        out[f"alm/{fname}/{cname}"] = a
        # the error of a comparison goes with the alm before the visibility is subtracted (the overdensity monopole cancels)
        field = fields[fname]
        before = a
        if type(field).__name__ == "Positions" and field.overdensity:
            before = a + mappers[field.mapper.lmax].resample(out[f"{cname}/vis"])
        out[f"scale/{fname}/{cname}"] = np.float64(np.abs(before).max())
        md = dict(alms[fname, cname].dtype.metadata)
        meta[f"{fname}/{cname}"] = {k: (float(v) if isinstance(v, (np.floating, float)) and not isinstance(v, bool) else v) for k, v in md.items()}
    settings = {"fields": fields_spec, "catalogs": cats, "columns": list(COLS), "keys": [list(k) for k in alms]}
    out["settings"] = np.array(json.dumps(settings))
    out["metadata"] = np.array(json.dumps(meta))
    out["warnings"] = np.array(json.dumps(warns))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(alms)} alms; warnings {warns}")


if __name__ == "__main__":
    main()
