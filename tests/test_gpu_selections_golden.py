"""Views, selections and filters against the reference's own (tests/golden/reference_selections.npz, written by
tests/golden/make_golden_selections.py): every view mapped in one pass, maps bit-exact where nbar is given (else to 1e-13 of max), metadata
to 1e-12, the distinct warning texts per view, and the reference's errors."""

import json
import os
import warnings

import numpy as np
import pytest

import heracles_amd as hx

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_selections.npz")


def _load():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["settings"])), json.loads(str(g["metadata"])), json.loads(str(g["warnings"])), json.loads(str(g["errors"]))


def _view(cat, terms, cols, vis):
    if not terms:
        return cat
    sel = [expr if kind == "s" else eval(expr, None, dict(cols)) for kind, expr in (t.split(":", 1) for t in terms)]
    view = cat.where(sel[0], vis)
    for s in sel[1:]:
        view = view[s]
    return view


def _fields(settings):
    mappers = {ns: hx.HipHealpixMapper(ns, settings["lmax"][str(ns)], deconvolve=False) for ns in (8, 16)}
    return {name: getattr(hx, typ)(mappers[ns], *cols, **kw) for name, typ, ns, cols, kw in settings["fields"]}


@pytest.mark.parametrize("device_columns", [False, True])
def test_views_match_the_reference(device_columns):
    import torch

    g, settings, meta, warns, _ = _load()
    cols = {k: np.array(g[f"col/{k}"]) for k in settings["columns"]}
    data = {k: torch.as_tensor(v, device="cuda") for k, v in cols.items()} if device_columns else cols
    cat = hx.ArrayCatalog(data, page_size=settings["page_size"], visibility=np.array(g["vis/base"]), metadata={"catalog": "base"})
    cat.add_filter(hx.InvalidValueFilter("e1", "e2", weight="w", warn=False))
    cat.add_filter(hx.InvalidValueFilter("Z"))
    cat.add_filter(hx.FootprintFilter(np.array(g["fp"]), "lon", "lat"))
    views = {}
    for key, (terms, vns) in settings["views"].items():
        vis = np.array(g[f"vis/{key}"]) if vns is not None else None
        views[key] = _view(cat, terms, cols if not device_columns else data, vis)
    fields = _fields(settings)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = hx.map_catalogs(fields, views)
    assert sorted({str(r.message) for r in rec}) == sorted({w for ws in warns.values() for w in ws})
    assert list(got) == [(f, k) for k in settings["views"] for f in fields]
    for (fname, key), m in got.items():
        want = g[f"map/{fname}/{key}"]
        if fname in ("NUM", "VIS"):
            np.testing.assert_array_equal(m, want, err_msg=f"{fname} {key}")
        else:
            np.testing.assert_allclose(m, want, rtol=0, atol=1e-13 * np.abs(want).max(), err_msg=f"{fname} {key}")
        md = dict(m.dtype.metadata)
        for k, v in meta[f"{fname}/{key}"].items():
            assert md[k] == (pytest.approx(v, rel=1e-12) if isinstance(v, float) else v), (fname, key, k)
    # the distinct warning texts of each view, mapped on its own
    for key, view in views.items():
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            hx.map_catalogs(fields, {key: view})
        assert sorted({str(r.message) for r in rec}) == warns[key], key


def test_errors_match_the_reference():
    g, settings, _, _, errors = _load()
    cols = {k: np.array(g[f"ecol/{k}"]) for k in settings["columns"]}
    fields = {k: v for k, v in _fields(settings).items() if k in ("NUM", "SHE", "WHT")}
    cat = hx.ArrayCatalog(cols, page_size=settings["page_size"])
    for key, terms in settings["err_views"].items():
        if errors[key] is None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                hx.map_catalogs(fields, {key: _view(cat, terms, cols, None)})
        else:
            with pytest.raises(ValueError, match=errors[key][1]):
                hx.map_catalogs(fields, {key: _view(cat, terms, cols, None)})
    fcat = hx.ArrayCatalog(cols, page_size=settings["page_size"])
    fcat.add_filter(hx.FootprintFilter(np.array(g["fp"]), "lon", "lat"))
    assert errors["fp"][0] == "ValueError"
    with pytest.raises(ValueError, match=r"THETA is out of range \[0,pi\]"):
        hx.map_catalogs(fields, {"fp": fcat["TOM_BIN_ID==2"]})
