"""``heracles.map_catalogs`` (heracles/mapping.py:61-110) and ``heracles.transform`` (:113-175) on the GPU.

``map_catalogs`` reads every catalogue page once for all the fields mapped from that catalogue: the page's columns go to one
``hx_catmap`` context (upload, one preparation kernel, one stable pixel sort per resolution, one ordered add into every map), the maps
stay in HBM until the last page, and the field's normalisation runs there too.  Maps, metadata, warnings and errors are those of the
reference's fields (heracles/fields.py:197-559); see ``heracles_amd.fields``.

``transform`` is the reference's as one batched call per mapper.

The reference walks ``data`` -- ``{(field name, bin): map}`` -- and transforms one map at a time (mapping.py:171).  Here the walk
only *plans*: every map becomes a ``_Job`` filed under the mapper that will transform it, and each mapper then receives all of its
maps in a single ``transform_many`` call (``hx_map2alm_list``: one upload pipeline, no stacked host copy).  What a caller of the
reference can observe is kept: the keys of ``out`` in the order of ``data``, a map without ``spin`` metadata taking its field's, and
the two ``ValueError`` messages (unknown field name, spin mismatch), which are the reference's."""

import ctypes as C
import math
import warnings
from dataclasses import dataclass
from typing import Any

import numpy as np

from .core import DeviceArray, TocDict, toc_match, update_metadata

__all__ = ["map_catalogs", "transform"]


@dataclass
class _Job:
    key: tuple
    array: Any
    spin: int
    alm: Any = None


def _declared_spin(array):
    """``spin`` from the dtype metadata of a numpy map; device tensors carry none."""
    meta = getattr(getattr(array, "dtype", None), "metadata", None)
    return None if not meta else meta.get("spin")


def _plan(fields, data, progress):
    """One pass over ``data``: validate every map against its field and file it under its mapper (first-seen order of mappers)."""
    jobs, per_mapper = [], {}
    for n, (key, entry) in enumerate(data.items(), 1):
        if progress is not None:
            progress.update(n, len(data))
        name = key[0]
        if name not in fields:
            raise ValueError(f"unknown field name: {name}")
        field = fields[name]
        array = getattr(entry, "array", entry)
        declared = _declared_spin(array)
        if declared is None:
            if hasattr(getattr(array, "dtype", None), "metadata"):
                update_metadata(array, spin=field.spin)
        elif declared != field.spin:
            raise ValueError(f"spin mismatch for field {name!r}: map has spin {declared}, field has spin {field.spin}")
        job = _Job(key, array, field.spin)
        jobs.append(job)
        mapper = getattr(field, "mapper_or_error", None) or field.mapper
        per_mapper.setdefault(id(mapper), (mapper, []))[1].append(job)
    return jobs, list(per_mapper.values())


def transform(fields, data, *, out=None, progress=None, device=None):
    """Alms of the maps in ``data`` for the ``fields`` they belong to; ``out`` (any mutable mapping) receives ``out[k, i]`` in the
    order of ``data``.  ``device="cuda"`` (not in the reference): the alms stay in HBM as ``DeviceArray``s, which
    ``angular_power_spectra`` takes as they are.  ``DeviceArray`` maps (``map_catalogs(device=...)``) give ``DeviceArray`` alms that
    carry the maps' metadata and ``deconv``, as numpy maps do."""
    if out is None:
        out = TocDict()
    jobs, batches = _plan(fields, data, progress)
    for mapper, batch in batches:
        if hasattr(mapper, "transform_many"):
            extra = {} if device is None else {"device": device}
            alms = mapper.transform_many([j.array for j in batch], [j.spin for j in batch], **extra)
        else:  # a mapper of the reference: map by map, as it does
            alms = [mapper.transform(j.array, spin=j.spin) for j in batch]
        for job, alm in zip(batch, alms):
            job.alm = alm
    for job in jobs:
        out[job.key] = job.alm
    return out


# ---- map_catalogs ---------------------------------------------------------------------------------------------------------------------

# kinds of hx_catmap_create (include/hxsht.h); VISIBILITY needs no pass over the catalogue
_POSITIONS, _SCALAR, _COMPLEX, _WEIGHTS, _VISIBILITY = 0, 1, 2, 3, -1
# the field types of heracles/fields.py, recognised by class name along the MRO (so the reference's own objects are accepted too)
_KINDS = {"Positions": _POSITIONS, "ScalarField": _SCALAR, "ComplexField": _COMPLEX, "Spin2Field": _COMPLEX,
          "Weights": _WEIGHTS, "Visibility": _VISIBILITY}
_MAX_FIELDS, _MAX_GROUPS, _MAX_COLUMNS = 8, 4, 16  # HX_CAT_MAX_* of include/hxsht.h


@dataclass
class _Item:
    key: tuple
    field: Any
    kind: int
    mapper: Any = None
    lonlat: tuple = ()
    value: Any = None  # value / real column
    imag: Any = None
    weight: Any = None


def _kind(field):
    for cls in type(field).__mro__:
        if cls.__name__ in _KINDS:
            return _KINDS[cls.__name__]
    raise TypeError(f"map_catalogs: cannot map a field of type {type(field).__name__!r}: not one of "
                    f"{', '.join(sorted(_KINDS))}")


def _mapper_or_error(field):
    mapper = field.mapper
    if mapper is None:
        raise ValueError("no mapper for field")
    from .mapper import HipHealpixMapper

    if not isinstance(mapper, HipHealpixMapper):
        raise NotImplementedError(f"map_catalogs: mapper of type {type(mapper).__name__!r} is not supported; catalogues are mapped "
                                  "with HipHealpixMapper only (HipDiscreteMapper has no maps)")
    return mapper


def _columns_or_error(field):
    columns = field.columns
    if columns is None:
        raise ValueError("no columns for field")
    return tuple(columns)


def _item(key, field, catalog):
    """The checks each reference field makes before its first page, in its order; raises what it raises."""
    kind = _kind(field)
    if kind == _POSITIONS and field.overdensity and catalog.visibility is None:
        raise ValueError("cannot compute density contrast: no visibility in catalog")
    item = _Item(key, field, kind, _mapper_or_error(field))
    if kind == _VISIBILITY:
        if catalog.visibility is None:
            raise ValueError("no visibility in catalog")
        return item
    cols = _columns_or_error(field)
    item.lonlat, item.weight = tuple(cols[:2]), cols[-1]
    if kind == _SCALAR:
        item.value = cols[2]
    elif kind == _COMPLEX:
        item.value, item.imag = cols[2], cols[3]
    return item


def _chunks(items):
    """Split the fields of one catalogue into contexts of at most _MAX_FIELDS fields, _MAX_GROUPS (nside, lon, lat) groups and
    _MAX_COLUMNS columns (each context reads the catalogue once)."""
    chunk, groups, cols = [], set(), []
    for it in items:
        g = (it.mapper.nside, *it.lonlat)
        need = [c for c in (*it.lonlat, it.value, it.imag, it.weight) if c is not None and c not in cols]
        if chunk and (len(chunk) == _MAX_FIELDS or len(groups | {g}) > _MAX_GROUPS or len(cols) + len(need) > _MAX_COLUMNS):
            yield chunk, cols
            chunk, groups, cols = [], set(), []
            need = [c for c in (*it.lonlat, it.value, it.imag, it.weight) if c is not None and c not in cols]
        chunk.append(it)
        groups.add(g)
        cols.extend(need)
    if chunk:
        yield chunk, cols


def _new_map(nrow, npix, device):
    import torch

    return torch.zeros((nrow, npix) if nrow > 1 else (npix,), dtype=torch.float64, device=device)


def _column(x, device):
    """A page column as the library takes it: a contiguous float64 numpy array, or a device tensor used in place."""
    if hasattr(x, "data_ptr"):
        import torch

        if x.is_cuda:
            return x.to(torch.float64).contiguous()
        x = x.numpy()
    from .mapper import _native

    return np.ascontiguousarray(_native(np.asarray(x)), dtype=np.float64)


class _CatMap:
    """One hx_catmap context: the fields of one catalogue (at most _MAX_FIELDS) and their device maps."""

    def __init__(self, page_size, ncols, desc, maps):
        from . import _lib

        _lib.ensure_init()
        self._L = _lib.load()
        self.maps = maps
        d = np.ascontiguousarray(desc, dtype=np.intc).ravel()
        self._desc = d
        ptrs = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
        for m in maps:  # (torch zero-filled them on its own stream)
            _lib.ptr(m)
        self._h = self._L.hx_catmap_create(int(page_size), int(ncols), len(maps), d.ctypes.data, ptrs)
        if not self._h:
            raise _lib.HxError(_lib.HX_ERR_ARG, self._L.hx_last_error().decode(errors="replace"))
        self._lib = _lib

    def page(self, n, cols):
        ptrs = (C.c_void_p * len(cols))(*[self._lib.ptr(c).value for c in cols])
        self._lib.check(self._L.hx_catmap_page(self._h, int(n), ptrs))

    def moments(self):
        nf = len(self.maps)
        mom, bad = np.empty((nf, 4)), np.empty((nf, 6), dtype=np.int64)
        self._lib.check(self._L.hx_catmap_moments(self._h, mom.ctypes.data, bad.ctypes.data))
        return mom, bad

    def finish(self, f, norm, vis):
        self._lib.check(self._L.hx_catmap_finish(self._h, int(f), float(norm), None if vis is None else self._lib.ptr(vis)))

    def close(self):
        if self._h:
            self._L.hx_catmap_destroy(self._h)
            self._h = None


def _device_of(device):
    import torch

    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _visibility_on(catalog, nside, device, message):
    """The catalogue's visibility as a device map at ``nside``; resampled (hp.ud_grade on the GPU) with the reference's warning when
    its size differs."""
    import torch

    from .mapper import _native, ud_grade

    vis = catalog.visibility
    if not hasattr(vis, "data_ptr"):
        vis = torch.as_tensor(np.ascontiguousarray(_native(np.asarray(vis)), dtype=np.float64))
    vis = vis.to(device=device, dtype=torch.float64).contiguous()
    if vis.numel() != 12 * nside * nside:
        warnings.warn(message)
        vis = ud_grade(vis, nside)
    return vis


_NAN_SLOTS = ("lonlat0", "lonlat1", "value", "imag", "weight")


def _check_page_errors(items, bad):
    """The reference raises in page.get (NaN in a column it reads) and in hp.ang2pix (invalid positions); the first field with
    either, in field order, decides the error."""
    for f, it in enumerate(items):
        names = (it.lonlat[0], it.lonlat[1], it.value, it.imag, it.weight)
        for k in range(5):
            if bad[f, k]:
                raise ValueError(f'invalid values in column "{names[k]}"')
        if bad[f, 5]:
            raise ValueError(f"map_catalogs: {int(bad[f, 5])} positions of field {it.key[0]!r} have a latitude outside [-90, 90] or a "
                             "non-finite coordinate (healpy: THETA is out of range [0,pi])")


def _normalise(it, mom, catalog):
    """Normalisation and bias ingredients with the reference's formulas (heracles/fields.py:271-299, :358-371, :497-509)."""
    n, sw, sw2, sv2 = (float(x) for x in mom)
    ngal = int(n)
    wmean, w2mean, var = (sw / n, sw2 / n, sv2 / n) if ngal else (0.0, 0.0, 0.0)
    fsky = catalog.fsky if catalog.fsky is not None else 1.0
    area = it.mapper.area
    with np.errstate(divide="ignore", invalid="ignore"):
        if it.kind == _POSITIONS:
            npix = 4 * np.pi / area
            nbar = np.float64(ngal) * wmean / fsky / npix
            given = it.field.nbar
            if given is not None:
                sigma = (given / fsky / npix) ** 0.5
                if abs(nbar - given) > 3 * sigma:
                    warnings.warn(f"The provided mean density ({given:g}) differs from the estimated mean density ({nbar:g}) by more "
                                  "than 3 sigma.")
                nbar = given
            dens = (nbar / area) ** 2 / (np.float64(ngal) / (4 * np.pi * fsky)) / w2mean
            return nbar, {"nbar": float(nbar), "musq": 1.0, "dens": float(dens), "fsky": float(fsky)}
        wbar = np.float64(ngal) / (4 * np.pi * fsky) * wmean * area
        musq = 1.0 if it.kind == _WEIGHTS else np.float64(var) / w2mean
        deff = np.float64(w2mean) / wmean**2
        dens = np.float64(ngal) / (4 * np.pi * fsky) / deff
        return wbar, {"wbar": float(wbar), "musq": float(musq), "dens": float(dens), "fsky": float(fsky)}


def _result(it, tensor, catalog, extra, device_out):
    """The map as the caller receives it: the mapper's ``create`` metadata, then the catalogue's, then the field's."""
    spin = it.field.spin
    shape = tuple(tensor.shape)
    if device_out:
        md = dict(it.mapper.create(*shape[:-1], 0, spin=spin).dtype.metadata or {})
        md.update(dict(catalog.metadata))
        md.update(extra)
        return DeviceArray(tensor, md)
    out = it.mapper.create(*shape[:-1], spin=spin)
    if isinstance(tensor, np.ndarray):
        out[...] = tensor
    elif out.dtype == np.float64 and out.flags.c_contiguous:
        from . import _lib

        _lib.copy(out, tensor)
    else:
        out[...] = tensor.cpu().numpy()
    update_metadata(out, **{**dict(catalog.metadata), **extra})
    return out


def _iter_pages(catalog, cap):
    for page in catalog:
        n = int(page.size)
        if n == 0:
            continue
        for start in range(0, n, cap):
            yield page, start, min(n, start + cap)


def _map_catalog(items, catalog, device, device_out):
    """Maps of the ``items`` (already checked, in field order) of one catalogue; {key: map}."""
    results = {}
    for it in items:
        if it.kind == _VISIBILITY:
            nside = it.mapper.nside
            vis = _visibility_on(catalog, nside, device, "changing size of visibility map")
            if catalog.visibility is vis:  # (a device visibility of the right size: the map is a copy, as the reference's out[:] = vis)
                vis = vis.clone()
            results[it.key] = _result(it, vis, catalog, {}, device_out)
    mapped = [it for it in items if it.kind != _VISIBILITY]
    cap = max(1, int(catalog.page_size))
    for chunk, cols in _chunks(mapped):
        index = {c: i for i, c in enumerate(cols)}
        desc, maps = [], []
        for it in chunk:
            ix = lambda c: -1 if c is None else index[c]
            desc.append([it.kind, it.mapper.nside, ix(it.lonlat[0]), ix(it.lonlat[1]), ix(it.value), ix(it.imag), ix(it.weight)])
            maps.append(_new_map(2 if it.kind == _COMPLEX else 1, 12 * it.mapper.nside**2, device))
        ctx = _CatMap(cap, len(cols), desc, maps)
        try:
            for page, start, stop in _iter_pages(catalog, cap):
                arrays = [_column(page[c], device) for c in cols]
                if start or stop != page.size:
                    arrays = [a[start:stop] for a in arrays]
                ctx.page(stop - start, arrays)
                del arrays, page
            mom, bad = ctx.moments()
            _check_page_errors(chunk, bad)
            for f, it in enumerate(chunk):
                norm, extra = _normalise(it, mom[f], catalog)
                vis = None
                if it.kind == _POSITIONS and it.field.overdensity:
                    vis = _visibility_on(catalog, it.mapper.nside, device, "positions and visibility have different size")
                ctx.finish(f, norm, vis)
                results[it.key] = _result(it, ctx.maps[f], catalog, extra, device_out)
        finally:
            ctx.close()
    return results


def map_catalogs(fields, catalogs, *, parallel=False, out=None, include=None, exclude=None, progress=None, device=None):
    """Maps of ``fields`` for every catalogue of ``catalogs``: ``out[field name, catalogue key]`` (any mutable mapping; a ``TocDict``
    by default), in the reference's order, filtered by ``include`` / ``exclude`` (``toc_match``).  ``progress.update(current, total)``
    is called before the first item and after each one.  ``device="cuda"`` (not in the reference): the maps stay in HBM and come back
    as ``DeviceArray``s carrying the metadata, which ``transform(device="cuda")`` passes on to the alms; by default they are numpy
    arrays with dtype metadata, as the reference returns.

    Fields are ``heracles_amd.fields`` objects or the reference's own objects of the same six types; every mapper must be a
    ``HipHealpixMapper``.  ``parallel`` is accepted for compatibility: each catalogue is read once for all its fields either way."""
    if out is None:
        out = TocDict()
    total = len(fields) * len(catalogs)
    current = 0
    if progress is not None:
        progress.update(current, total)
    dev = None
    for j, catalog in catalogs.items():
        items = [_item((i, j), field, catalog) for i, field in fields.items() if toc_match((i, j), include, exclude)]
        if not items:
            continue
        if dev is None:
            dev = _device_of(device)
        results = _map_catalog(items, catalog, dev, device is not None)
        for it in items:
            out[it.key] = results[it.key]
            current += 1
            if progress is not None:
                progress.update(current, total)
        del results
    return out
