"""The cases of tests/golden/reference_fields.npz (written by tests/golden/make_golden_fields.py) rebuilt for heracles_amd: the same
columns, paged the same way (one empty page included), the same visibilities, fields and mappers."""

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fields.npz")


class Page:
    """A page with the reference's protocol (heracles/catalog/base.py:46-136)."""

    def __init__(self, data):
        self.data = data
        self.size = len(next(iter(data.values())))

    def __getitem__(self, col):
        if isinstance(col, (list, tuple)):
            return tuple(self.data[c] for c in col)
        return self.data[col]

    def get(self, *cols):
        for c in cols:
            if np.isnan(self.data[c]).any():
                raise ValueError(f'invalid values in column "{c}"')
        out = [self.data[c] for c in cols]
        return out[0] if len(out) == 1 else out

    def delete(self, where):
        self.data = {k: np.delete(v, where) for k, v in self.data.items()}
        self.size = len(next(iter(self.data.values())))


class PagedCatalog:
    """A user's own catalogue class: only the protocol map_catalogs reads, pages of `page_size` rows, one empty page after page
    `empty_after`."""

    def __init__(self, cols, page_size, empty_after, visibility, label):
        self.cols, self.page_size, self.empty_after, self.visibility = cols, page_size, empty_after, visibility
        self.metadata = {"catalog": label}
        self.size = len(cols["lon"])
        self.pages_read = 0

    @property
    def fsky(self):
        return None if self.visibility is None else self.visibility.mean()

    def __iter__(self):
        self.pages_read += 1
        for i, start in enumerate(range(0, self.size, self.page_size)):
            yield Page({k: v[start : start + self.page_size] for k, v in self.cols.items()})
            if i == self.empty_after:
                yield Page({k: v[:0] for k, v in self.cols.items()})


def load():
    g = np.load(GOLDEN)
    settings = json.loads(str(g["settings"]))
    meta = json.loads(str(g["metadata"]))
    warns = json.loads(str(g["warnings"]))
    return g, settings, meta, warns


def catalogs(g, settings):
    out = {}
    for name, spec in settings["catalogs"].items():
        cols = {k: np.array(g[f"{name}/col/{k}"]) for k in settings["columns"]}
        out[name] = PagedCatalog(cols, spec["page_size"], spec["empty_after"], np.array(g[f"{name}/vis"]), spec["label"])
    return out


def fields(settings, module=None):
    import heracles_amd as hx

    module = module or hx
    mappers = {ns: hx.HipHealpixMapper(ns, settings["lmax"][str(ns)], deconvolve=False) for ns in (8, 16)}
    return {name: getattr(module, typ)(mappers[ns], *cols, **kw) for name, typ, ns, cols, kw in settings["fields"]}


def given_nbar(settings, name):
    for fname, typ, ns, cols, kw in settings["fields"]:
        if fname == name:
            return typ == "Positions" and kw.get("nbar") is not None
    raise KeyError(name)
