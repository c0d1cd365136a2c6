"""The cases of tests/golden/reference_discrete.npz (written by tests/golden/make_golden_discrete.py) rebuilt for heracles_amd: the
same columns, paged the same way (one empty page included), the same visibility alms, fields and band limits; and the numpy stand-in
for the hx_catalm context that the host tests put in its place."""

import json
import os
import warnings

import numpy as np

from fields_cases import PagedCatalog
from oracle import hxoracle as ho

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_discrete.npz")


class AlmCatalog(PagedCatalog):
    """PagedCatalog whose visibility is alms: fsky as heracles/catalog/base.py:36-44."""

    @property
    def fsky(self):
        vis = self.visibility
        if vis is None:
            return None
        return vis[0].real / (4 * np.pi) ** 0.5 if np.iscomplexobj(vis) else vis.mean()


def load():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["settings"])), json.loads(str(g["metadata"])), json.loads(str(g["warnings"]))


def catalogs(g, settings, only=None):
    out = {}
    for name, spec in settings["catalogs"].items():
        if only is not None and name not in only:
            continue
        cols = {k: np.array(g[f"{name}/col/{k}"]) for k in settings["columns"]}
        out[name] = AlmCatalog(cols, spec["page_size"], spec["empty_after"], np.array(g[f"{name}/vis"]), spec["label"])
    return out


def fields(settings, dtype=np.complex128):
    import heracles_amd as hx

    mappers = {lmax: hx.HipDiscreteMapper(lmax, dtype=dtype) for lmax in (12, 24)}
    return {name: getattr(hx, typ)(mappers[lmax], *cols, **kw) for name, typ, lmax, cols, kw in settings["fields"]}


def check_meta(md, want, where):
    import pytest

    assert set(md) == set(want), where
    for k, v in want.items():
        if isinstance(v, float):
            assert md[k] == pytest.approx(v, rel=1e-12), (where, k)
        else:
            assert md[k] == v, (where, k)


def to_point(lon, lat):
    """(theta, phi) of heracles/ducc.py:117-119."""
    return np.radians(90.0 - lat), np.radians(lon % 360.0)


def resample(alm, lmax_out):
    """The alms at band limit ``lmax_out``: every (l, m) both band limits hold is copied, the others are zero.  a_lm sits at
    m (2 L + 1 - m) / 2 + l in the m-major packing of band limit L."""
    src = ho.alm2lmax(alm.shape[-1])
    ell, m = np.tril_indices(min(src, lmax_out) + 1)  # all pairs m <= l <= the smaller band limit
    at = lambda L: m * (2 * L + 1 - m) // 2 + ell
    out = np.zeros((*alm.shape[:-1], ho.nlm(lmax_out)), dtype=np.complex128)
    out[..., at(lmax_out)] = alm[..., at(src)]
    return out


class NpPointSHT:
    """What the driver reads of a PointSHT: the band limit and the grid size (hx_pointsht_create: N = the power of two >= 2 lmax + 2,
    at least 16; n1 = 2 N)."""

    def __init__(self, lmax):
        n = 16
        while n < 2 * lmax + 2:
            n *= 2
        self.lmax, self.ngrid = lmax, 2 * n


class NpCatAlm:
    """numpy stand-in for mapping._CatAlm (hx_catalm_*): the direct sum of the oracle, page by page."""

    created = 0

    def __init__(self, page_size, ncols, desc, shts):
        from heracles_amd import mapping as mp

        NpCatAlm.created += 1
        self.mp = mp
        self.desc = np.asarray(desc, dtype=int).reshape(-1, 7)
        assert [s.lmax for s in shts] == [d[1] for d in self.desc]
        nf = len(self.desc)
        self.points = [[] for _ in range(nf)]  # per field: (theta, phi, value rows) of every page
        self.mom = np.zeros((nf, 4))
        self.bad = np.zeros((nf, 6), dtype=np.int64)

    def page(self, n, cols):
        mp = self.mp
        for f, (kind, lmax, lo, la, v, im, w) in enumerate(self.desc):
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
            vals = np.nan_to_num(np.array([r[ok] for r in rows]))  # (a NaN on a kept row is counted: the caller raises)
            self.points[f].append((*to_point(lon[ok], lat[ok]), vals))
            sq = sum(r * r for r in rows) if kind in (mp._SCALAR, mp._COMPLEX) else np.zeros(1)
            self.mom[f] += [keep.sum(), ww.sum(), (ww * ww).sum(), sq.sum()]

    def moments(self):
        return self.mom, self.bad

    def finish(self, f, spin, norm, vis, alm):
        a = np.zeros(alm.shape, dtype=np.complex128).reshape(-1, alm.shape[-1])
        for theta, phi, vals in self.points[f]:
            a += ho.points2alm(theta, phi, vals, self.desc[f][1], spin=spin)
        a = a / norm
        if vis is not None:
            a = a - vis
        alm[...] = a.reshape(alm.shape)

    def close(self):
        pass


def np_visibility_alm(catalog, lmax, device, message):
    vis = np.asarray(catalog.visibility, dtype=np.complex128)
    if vis.size != ho.nlm(lmax):
        warnings.warn(message)
        vis = resample(vis, lmax)
    return vis.copy()


def host_patches(monkeypatch):
    """Puts the numpy stand-ins in the place of everything in heracles_amd.mapping that touches the GPU for catalog_alms."""
    from heracles_amd import mapping as mp

    monkeypatch.setattr(mp, "_CatAlm", NpCatAlm)
    monkeypatch.setattr(mp, "_new_alm", lambda nrow, nlm, device: np.empty((nrow, nlm) if nrow > 1 else nlm, dtype=np.complex128))
    monkeypatch.setattr(mp, "_device_of", lambda device: "cpu")
    monkeypatch.setattr(mp, "_visibility_alm", np_visibility_alm)
    monkeypatch.setattr(mp, "_point_sht", NpPointSHT)
    monkeypatch.setattr(mp, "_map_budget", lambda device: 1 << 40)
