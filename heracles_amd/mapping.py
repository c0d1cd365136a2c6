"""``heracles.map_catalogs`` (heracles/mapping.py:61-110) and ``heracles.transform`` (:113-175) on the GPU.

``map_catalogs`` reads every catalogue page once for all the fields mapped from that catalogue: the page's columns go to one
``hx_catmap`` context (upload, one preparation kernel, one stable pixel sort per resolution, one ordered add into every map), the maps
stay in HBM until the last page, and the field's normalisation runs there too.  Maps, metadata, warnings and errors are those of the
reference's fields (heracles/fields.py:197-559); see ``heracles_amd.fields``.

``catalog_alms`` is the other half of the reference's ``map_catalogs``: fields whose mapper is a ``HipDiscreteMapper`` give alms, not
maps (heracles/ducc.py:92-133).  The same page protocol feeds one ``hx_catalm`` context, whose accumulators are the oversampled grids of
the point transform: they stay in HBM from the first page to the last, so the FFT stages and the Legendre analysis run once per field.

``transform`` is the reference's as one batched call per mapper.

The reference walks ``data`` -- ``{(field name, bin): map}`` -- and transforms one map at a time (mapping.py:171).  Here the walk
only *plans*: every map becomes a ``_Job`` filed under the mapper that will transform it, and each mapper then receives all of its
maps in a single ``transform_many`` call (``hx_map2alm_list``: one upload pipeline, no stacked host copy).  What a caller of the
reference can observe is kept: the keys of ``out`` in the order of ``data``, a map without ``spin`` metadata taking its field's, and
the two ``ValueError`` messages (unknown field name, spin mismatch), which are the reference's."""

import ast
import ctypes as C
import math
import warnings
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Any

import numpy as np

from .core import DeviceArray, TocDict, toc_match, update_metadata

__all__ = ["map_catalogs", "catalog_alms", "transform"]


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

    @property
    def columns(self):
        """The columns the field reads, in the order of the reference's ``columns``."""
        return _read((*self.lonlat, self.value, self.imag, self.weight))


def _read(columns):
    """The columns of a field's ``columns`` tuple that name one (an optional column is None)."""
    return tuple(c for c in columns if c is not None)


def _mapped(items):
    """The items that need a pass over the catalogue."""
    return [it for it in items if it.kind != _VISIBILITY]


def _kind(field, who="map_catalogs"):
    for cls in type(field).__mro__:
        if cls.__name__ in _KINDS:
            return _KINDS[cls.__name__]
    raise TypeError(f"{who}: cannot map a field of type {type(field).__name__!r}: not one of "
                    f"{', '.join(sorted(_KINDS))}")


def _mapper_or_error(field):
    mapper = field.mapper
    if mapper is None:
        raise ValueError("no mapper for field")
    from .mapper import HipHealpixMapper

    if not isinstance(mapper, HipHealpixMapper):
        raise NotImplementedError(f"map_catalogs: mapper of type {type(mapper).__name__!r} is not supported; catalogues are mapped "
                                  "with HipHealpixMapper only (HipDiscreteMapper has no maps: catalog_alms gives its alms)")
    return mapper


def _discrete_mapper_or_error(field):
    mapper = field.mapper
    if mapper is None:
        raise ValueError("no mapper for field")
    from .discrete import HipDiscreteMapper
    from .mapper import HipHealpixMapper

    if isinstance(mapper, HipHealpixMapper):
        raise NotImplementedError("catalog_alms: a HipHealpixMapper field has maps: use map_catalogs (and transform) for it")
    if not isinstance(mapper, HipDiscreteMapper):
        raise NotImplementedError(f"catalog_alms: mapper of type {type(mapper).__name__!r} is not supported; alms are accumulated "
                                  "with HipDiscreteMapper only")
    return mapper


def _columns_or_error(field):
    columns = field.columns
    if columns is None:
        raise ValueError("no columns for field")
    return tuple(columns)


def _item(key, field, catalog, mapper_of=_mapper_or_error, who="map_catalogs"):
    """The checks each reference field makes before its first page, in its order; raises what it raises."""
    kind = _kind(field, who)
    if kind == _POSITIONS and field.overdensity and catalog.visibility is None:
        raise ValueError("cannot compute density contrast: no visibility in catalog")
    item = _Item(key, field, kind, mapper_of(field))
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


def _resolution(mapper):
    """What fields must share, next to their position columns, to share a group: the nside of a HEALPix mapper, the lmax of a
    discrete one."""
    nside = getattr(mapper, "nside", None)
    return mapper.lmax if nside is None else nside


def _chunks(items, cols0=(), fits=None, who="map_catalogs"):
    """Split the fields of one catalogue into contexts of at most _MAX_FIELDS fields, _MAX_GROUPS (nside or lmax, lon, lat) groups and
    _MAX_COLUMNS columns (each context reads the catalogue once); ``cols0``: columns every context reads first.  ``fits(fields)``:
    whether these fields may share a context (the memory budget of catalog_alms); it raises for a single field that cannot.
    ``who``: the entry point named in the error."""
    chunk, groups, cols = [], set(), list(cols0)
    for it in items:
        g = (_resolution(it.mapper), *it.lonlat)
        need = lambda: [c for c in it.columns if c not in cols]
        if chunk and (len(chunk) == _MAX_FIELDS or len(groups | {g}) > _MAX_GROUPS or len(cols) + len(need()) > _MAX_COLUMNS
                      or (fits is not None and not fits([*chunk, it]))):
            yield chunk, cols
            chunk, groups, cols = [], set(), list(cols0)
        if len(cols) + len(need()) > _MAX_COLUMNS:
            raise ValueError(f"{who}: field {it.key[0]!r} needs {len(cols) + len(need())} columns in one context (at most "
                             f"{_MAX_COLUMNS})")
        if not chunk and fits is not None:
            fits([it])
        chunk.append(it)
        groups.add(g)
        cols.extend(need())
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


class _Context:
    """What the two contexts share: the library, the device maps (handed over from torch's stream, which zero-filled them) and the
    handle."""

    _destroy = None  # name of the entry point that frees the handle

    def _open(self, maps):
        from . import _lib

        _lib.ensure_init()
        self._lib, self._L, self._h = _lib, _lib.load(), None
        self.maps = maps
        return (C.c_void_p * len(maps))(*[_lib.ptr(m).value for m in maps])

    def _created(self, handle):
        if not handle:
            raise self._lib.HxError(self._lib.HX_ERR_ARG, self._L.hx_last_error().decode(errors="replace"))
        self._h = handle

    def _pointers(self, cols):
        return (C.c_void_p * len(cols))(*[self._lib.ptr(c).value for c in cols])

    def close(self):
        if self._h:
            getattr(self._L, self._destroy)(self._h)
            self._h = None


class _CatMap(_Context):
    """One hx_catmap context: the fields of one catalogue (at most _MAX_FIELDS) and their device maps."""

    _destroy = "hx_catmap_destroy"

    def __init__(self, page_size, ncols, desc, maps):
        ptrs = self._open(maps)
        d = self._desc = np.ascontiguousarray(desc, dtype=np.intc).ravel()
        self._created(self._L.hx_catmap_create(int(page_size), int(ncols), len(maps), d.ctypes.data, ptrs))

    def page(self, n, cols):
        self._lib.check(self._L.hx_catmap_page(self._h, int(n), self._pointers(cols)))

    def moments(self):
        nf = len(self.maps)
        mom, bad = np.empty((nf, 4)), np.empty((nf, 6), dtype=np.int64)
        self._lib.check(self._L.hx_catmap_moments(self._h, mom.ctypes.data, bad.ctypes.data))
        return mom, bad

    def finish(self, f, norm, vis):
        self._lib.check(self._L.hx_catmap_finish(self._h, int(f), float(norm), self._lib.ptr(vis)))


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


def _check_page_errors(items, bad, who="map_catalogs"):
    """The reference raises in page.get (NaN in a column it reads) and in hp.ang2pix (invalid positions); the first field with
    either, in field order, decides the error."""
    for f, it in enumerate(items):
        names = (it.lonlat[0], it.lonlat[1], it.value, it.imag, it.weight)
        for k in range(5):
            if bad[f, k]:
                raise ValueError(f'invalid values in column "{names[k]}"')
        if bad[f, 5]:
            raise ValueError(f"{who}: {int(bad[f, 5])} positions of field {it.key[0]!r} have a latitude outside [-90, 90] or a "
                             "non-finite coordinate" + (" (healpy: THETA is out of range [0,pi])" if who == "map_catalogs" else ""))


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
    elif out.dtype in (np.float64, np.complex128) and out.flags.c_contiguous:
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


def _add_texts(texts, new):
    """Appends the texts of ``new`` not yet in ``texts``, in order."""
    for text in new:
        if text not in texts:
            texts.append(text)


@contextmanager
def _collect(texts):
    """Records the warnings raised inside instead of showing them: their texts go to ``texts``, each once (map_catalogs raises them in
    the catalogue's turn).  ``texts`` None: the warnings are shown as they come."""
    if texts is None:
        yield
        return
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        yield
    _add_texts(texts, (str(w.message) for w in rec))


def _map_visibility(items, catalog, device, device_out, texts=None):
    """{key: map} of the ``Visibility`` items of a catalogue: its visibility at the field's resolution.  ``texts``: where the
    resampling warnings go (_collect)."""
    results = {}
    for it in items:
        if it.kind != _VISIBILITY:
            continue
        with _collect(texts):
            vis = _visibility_on(catalog, it.mapper.nside, device, "changing size of visibility map")
        if catalog.visibility is vis:  # (a device visibility of the right size: the map is a copy, as the reference's out[:] = vis)
            vis = vis.clone()
        results[it.key] = _result(it, vis, catalog, {}, device_out)
    return results


def _context_inputs(chunk, cols, nsel, device):
    """The descriptors of hx_catmap_create (7 ints per field: kind, nside and the indices in ``cols`` of lon, lat, value, imaginary
    part and weight, -1 for none) and the zeroed device maps [nsel][fields] of one context."""
    index = {c: i for i, c in enumerate(cols)}
    ix = lambda c: -1 if c is None else index[c]
    desc = [[it.kind, it.mapper.nside, ix(it.lonlat[0]), ix(it.lonlat[1]), ix(it.value), ix(it.imag), ix(it.weight)] for it in chunk]
    maps = [_new_map(2 if it.kind == _COMPLEX else 1, 12 * it.mapper.nside**2, device) for _ in range(nsel) for it in chunk]
    return desc, maps


def _norm_and_visibility(it, mom, catalog, device):
    """What ``finish`` needs for one field of one catalogue: (norm, visibility map or None), and the metadata of _normalise."""
    norm, extra = _normalise(it, mom, catalog)
    vis = None
    if it.kind == _POSITIONS and it.field.overdensity:
        vis = _visibility_on(catalog, it.mapper.nside, device, "positions and visibility have different size")
    return (norm, vis), extra


def _map_catalog(items, catalog, device, device_out):
    """Maps of the ``items`` (already checked) of one catalogue; {key: map} in the order of the items."""
    results = _map_visibility(items, catalog, device, device_out)
    cap = max(1, int(catalog.page_size))
    for chunk, cols in _chunks(_mapped(items)):
        desc, maps = _context_inputs(chunk, cols, 1, device)
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
                finish, extra = _norm_and_visibility(it, mom[f], catalog, device)
                ctx.finish(f, *finish)
                results[it.key] = _result(it, maps[f], catalog, extra, device_out)
        finally:
            ctx.close()
    return {it.key: results[it.key] for it in items}


# ---- catalog_alms: catalogues to alms through the point transform (hx_catalm_*) --------------------------------------------------------

def _nlm(lmax):
    return (lmax + 1) * (lmax + 2) // 2


def _point_sht(lmax):
    """The point transform behind the fields of one band limit, at the accuracy every column is mapped with."""
    from .discrete import get_point_sht

    return get_point_sht(lmax, 1e-12)


def _new_alm(nrow, nlm, device):
    import torch

    return torch.empty((nrow, nlm) if nrow > 1 else (nlm,), dtype=torch.complex128, device=device)


class _CatAlm(_Context):
    """One hx_catalm context: the fields of one pass over a catalogue, their point transforms (borrowed) and the resident grids."""

    _destroy = "hx_catalm_destroy"

    def __init__(self, page_size, ncols, desc, shts):
        self._open([])
        self.nfield, self._shts = len(shts), list(shts)
        d = self._desc = np.ascontiguousarray(desc, dtype=np.intc).ravel()
        ps = (C.c_void_p * len(shts))(*[s._h for s in shts])
        self._created(self._L.hx_catalm_create(int(page_size), int(ncols), len(shts), d.ctypes.data, ps))

    def page(self, n, cols):
        self._lib.check(self._L.hx_catalm_page(self._h, int(n), self._pointers(cols)))

    def moments(self):
        mom, bad = np.empty((self.nfield, 4)), np.empty((self.nfield, 6), dtype=np.int64)
        self._lib.check(self._L.hx_catalm_moments(self._h, mom.ctypes.data, bad.ctypes.data))
        return mom, bad

    def finish(self, f, spin, norm, vis, alm):
        self._lib.check(self._L.hx_catalm_finish(self._h, int(f), int(spin), float(norm), self._lib.ptr(vis), self._lib.ptr(alm)))


def _is_complex(x):
    return x.is_complex() if hasattr(x, "data_ptr") else np.iscomplexobj(x)


def _alm_item(key, field, catalog):
    """_item for catalog_alms; where the field reads the visibility, it must be alms (complex), as heracles/catalog/base.py:36-44 tells
    a visibility map from visibility alms."""
    it = _item(key, field, catalog, _discrete_mapper_or_error, "catalog_alms")
    if it.kind != _VISIBILITY and (field.spin < 0 or (field.spin > 0 and it.kind != _COMPLEX)):
        # (what hx_catalm_finish would answer with HX_ERR_ARG after the pass over the catalogue)
        raise ValueError(f"catalog_alms: field {key[0]!r} has spin weight {field.spin}: a weight s >= 1 needs the two components of a "
                         "ComplexField, and a negative weight has no transform")
    if (it.kind == _VISIBILITY or (it.kind == _POSITIONS and field.overdensity)) and not _is_complex(catalog.visibility):
        raise ValueError(f"catalog_alms: field {key[0]!r} needs the catalogue's visibility as alms (a complex array); a visibility map "
                         "goes with map_catalogs")
    return it


def _visibility_alm(catalog, lmax, device, message):
    """The catalogue's visibility alms on the device at ``lmax``; re-packed (DiscreteMapper.resample) with the reference's warning when
    their size differs."""
    import torch

    from .discrete import alm_resample
    from .mapper import _native

    vis = catalog.visibility
    if not hasattr(vis, "data_ptr"):
        vis = torch.as_tensor(np.ascontiguousarray(_native(np.asarray(vis)), dtype=np.complex128))
    vis = vis.to(device=device, dtype=torch.complex128).contiguous()
    if vis.numel() != _nlm(lmax):
        warnings.warn(message)
        vis = alm_resample(vis, lmax)
    return vis


def _alm_visibility(items, catalog, device, device_out):
    """{key: alm} of the ``Visibility`` items: a copy of the catalogue's visibility alms at the field's band limit."""
    results = {}
    for it in items:
        if it.kind != _VISIBILITY:
            continue
        vis = _visibility_alm(catalog, it.mapper.lmax, device, "changing size of visibility map")
        if catalog.visibility is vis:
            vis = vis.clone()
        results[it.key] = _result(it, vis, catalog, {}, device_out)
    return results


def _alm_fits(device):
    """``fits`` of _chunks for catalog_alms: the grids of the fields (8 n1^2 bytes per component) within _map_budget less the scratch of
    the finishing transforms (T, U and two components of h per band limit: 16 (lmax + 1) (n1 + 3 n1 / 2) bytes)."""
    def fits(fields):
        grids = sum(8 * (2 if it.kind == _COMPLEX else 1) * _point_sht(it.mapper.lmax).ngrid ** 2 for it in fields)
        scratch = 0
        for lmax in {it.mapper.lmax for it in fields}:
            n1 = _point_sht(lmax).ngrid
            scratch += 16 * (lmax + 1) * (n1 + 3 * n1 // 2)
        budget = _map_budget(device)
        if grids + scratch <= budget:
            return True
        if len(fields) == 1:
            raise MemoryError(f"catalog_alms: field {fields[0].key[0]!r} at lmax {fields[0].mapper.lmax} needs {grids} bytes of grids "
                              f"and {scratch} bytes of transform scratch; {budget} bytes are available")
        return False

    return fits


def _alms_of_catalog(items, catalog, device, device_out):
    """Alms of the ``items`` (already checked) of one catalogue; {key: alm} in the order of the items."""
    results = _alm_visibility(items, catalog, device, device_out)
    cap = max(1, int(catalog.page_size))
    for chunk, cols in _chunks(_mapped(items), fits=_alm_fits(device), who="catalog_alms"):
        index = {c: i for i, c in enumerate(cols)}
        ix = lambda c: -1 if c is None else index[c]
        desc = [[it.kind, it.mapper.lmax, ix(it.lonlat[0]), ix(it.lonlat[1]), ix(it.value), ix(it.imag), ix(it.weight)] for it in chunk]
        ctx = _CatAlm(cap, len(cols), desc, [_point_sht(it.mapper.lmax) for it in chunk])
        try:
            for page, start, stop in _iter_pages(catalog, cap):
                arrays = [_column(page[c], device) for c in cols]
                if start or stop != page.size:
                    arrays = [a[start:stop] for a in arrays]
                ctx.page(stop - start, arrays)
                del arrays, page
            mom, bad = ctx.moments()
            _check_page_errors(chunk, bad, "catalog_alms")
            for f, it in enumerate(chunk):
                norm, extra = _normalise(it, mom[f], catalog)
                vis = None
                if it.kind == _POSITIONS and it.field.overdensity:
                    vis = _visibility_alm(catalog, it.mapper.lmax, device, "positions and visibility have different size")
                alm = _new_alm(2 if it.kind == _COMPLEX else 1, _nlm(it.mapper.lmax), device)
                ctx.finish(f, it.field.spin, norm, vis, alm)
                results[it.key] = _result(it, alm, catalog, extra, device_out)
        finally:
            ctx.close()
    return {it.key: results[it.key] for it in items}


def catalog_alms(fields, catalogs, *, out=None, include=None, exclude=None, progress=None, device=None):
    """Alms of ``fields`` for every catalogue of ``catalogs``, for fields whose mapper is a ``HipDiscreteMapper``: what the reference's
    ``map_catalogs`` returns with a ``DiscreteMapper`` (heracles/fields.py:197-559 over heracles/ducc.py:92-133).  ``out[field name,
    catalogue key]`` receives ``sum_p w_p v_p conj(sY_lm(lon_p, lat_p))`` over the rows the field keeps, divided by ``nbar`` /
    ``wbar`` (``mapper.area`` is 1), less the visibility alms for ``Positions(overdensity=True)``: an array of ``mapper.create(spin=...)``,
    or of ``mapper.create(2, spin=...)`` = (E, B) for a two-component field of any spin weight s >= 1 (``class X(ComplexField,
    spin=s)``) / (real, imaginary) for one of weight 0, carrying the metadata of ``create``,
    of the catalogue and of the field.  ``out``, key order, ``include`` / ``exclude``, ``progress`` and ``device="cuda"``
    (``DeviceArray``s around complex128 tensors) are those of ``map_catalogs``.

    A catalogue's visibility, where a field reads it, is alms here (a complex numpy array or CUDA tensor).  Any object with the page
    protocol is a catalogue; a view is read through its own iteration.  All fields of one catalogue share one pass over its pages, as
    far as the context limits and the memory budget allow (one resident float64 grid of ``PointSHT.ngrid``^2 per component: 2.1 GB up to
    lmax 4095, 8.6 GB above); fields that do not fit go to a further pass, and a single field that cannot fit raises ``MemoryError``.

    Every column is mapped in float64 at epsilon 1e-12, whatever its dtype (the reference asks ducc0 for 1e-5 when the values are
    float32).  The grids are filled with hardware float64 atomics: two runs agree to rounding, not bit for bit."""
    if out is None:
        out = TocDict()
    total = len(fields) * len(catalogs)
    current = 0
    if progress is not None:
        progress.update(current, total)
    dev = None
    for j, catalog in catalogs.items():
        items = [_alm_item((i, j), field, catalog) for i, field in fields.items() if toc_match((i, j), include, exclude)]
        if not items:
            continue
        if dev is None:
            dev = _device_of(device)
        results = _alms_of_catalog(items, catalog, dev, device is not None)
        for key in list(results):
            out[key] = results.pop(key)
            current += 1
            if progress is not None:
                progress.update(current, total)
    return out


# ---- views of one base catalogue in one pass (hx_catmap_*_sel) -------------------------------------------------------------------------

_MAX_SELECTIONS, _MAX_PREDICATES, _MAX_FILTERS = 32, 64, 4  # HX_CAT_MAX_* of include/hxsht.h
_OPS = {ast.Eq: 0, ast.NotEq: 1, ast.Lt: 2, ast.LtE: 3, ast.Gt: 4, ast.GtE: 5}  # HX_CAT_EQ .. HX_CAT_GE
_FILTER_INVALID, _FILTER_FOOTPRINT = 0, 1


def _constant(node):
    """The number of a constant node (``3``, ``-0.5``), else None."""
    sign = 1
    if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
        sign = -1 if isinstance(node.op, ast.USub) else 1
        node = node.operand
    if isinstance(node, ast.Constant) and type(node.value) in (int, float):
        return sign * node.value
    return None


def _compile_predicate(expr, dtypes):
    """``[(column, op, value), ...]`` for a row filter made of comparisons ``column OP constant`` joined by ``&``, or None when the
    string is anything else (it is then evaluated per page by the row-filter rule).  Parsed with ``ast``, never evaluated.  ``dtypes``
    maps the base's column names to their dtypes: a comparison compiles only where float64 gives numpy's answer (float64 columns;
    integer columns against a constant of magnitude at most 2^53)."""
    try:
        tree = ast.parse(expr, mode="eval")
    except SyntaxError:
        return None
    terms = []

    def walk(node):
        if isinstance(node, ast.BinOp) and isinstance(node.op, ast.BitAnd):
            return walk(node.left) and walk(node.right)
        if not (isinstance(node, ast.Compare) and len(node.ops) == 1 and type(node.ops[0]) in _OPS and isinstance(node.left, ast.Name)):
            return False
        name, value = node.left.id, _constant(node.comparators[0])
        dt = dtypes.get(name)
        if value is None or dt is None:
            return False
        dt = np.dtype(dt)
        if dt == np.float64 or (dt.kind in "iu" and (not float(value).is_integer() or abs(value) <= 2**53)):
            terms.append((name, _OPS[type(node.ops[0])], float(value)))
            return True
        return False

    return terms if walk(tree.body) and terms else None


def _dtypes(base):
    """{column: dtype} of the base's page columns (its page source: ``ArrayCatalog`` and ``FitsCatalog`` both provide it)."""
    return base._column_dtypes()


def _sel_base(catalog):
    """The base ``ArrayCatalog`` or ``FitsCatalog`` whose one-pass group ``catalog`` joins, or None for the per-catalogue path: a ``heracles_amd`` view, or
    its base itself, whose filters are all of the two known types."""
    from .catalog import CatalogView, FootprintFilter, InvalidValueFilter, _CatalogBase

    base = catalog.base if isinstance(catalog, CatalogView) else catalog
    if not isinstance(base, _CatalogBase) or not isinstance(catalog, (_CatalogBase, CatalogView)):
        return None
    if len(base.filters) > _MAX_FILTERS or any(type(f) not in (InvalidValueFilter, FootprintFilter) for f in base.filters):
        return None
    if any(isinstance(f, InvalidValueFilter) and not f.columns for f in base.filters):
        return None  # (a filter that checks no column: the per-catalogue path applies it as it is)
    return base


def _filter_columns(base):
    """The columns the base's filters read, in order."""
    from .catalog import FootprintFilter

    cols = []
    for flt in base.filters:
        names = flt.lonlat if isinstance(flt, FootprintFilter) else (*flt.columns, *(() if flt.weight is None else (flt.weight,)))
        cols.extend(c for c in names if c not in cols)
    return cols


def _room(cols0, mapped):
    """Whether every field of ``mapped`` fits one context next to the columns ``cols0`` (each context reads cols0 first)."""
    return all(len({*cols0, *it.columns}) <= _MAX_COLUMNS for it in mapped)


def _map_budget(device):
    """Bytes the maps of one pass may take (a hook tests lower to force a split)."""
    import torch

    free, _ = torch.cuda.mem_get_info(device)
    return int(free * 0.8)


class _CatMapSel(_Context):
    """One hx_catmap_sel context: the fields of one pass for S selections of one base, and the maps [S][nfields]."""

    _destroy = "hx_catmap_destroy_sel"

    def __init__(self, page_size, ncols, desc, nsel, preds, pval, filters, footprints, maps):
        mp = self._open(maps)
        self.nsel, self.nfield, self.nfilt = nsel, len(desc), len(filters)
        d = np.ascontiguousarray(desc, dtype=np.intc).ravel()
        p = np.ascontiguousarray(preds, dtype=np.intc).reshape(-1)
        v = np.ascontiguousarray(pval, dtype=np.float64).reshape(-1)
        fl = np.ascontiguousarray(filters, dtype=np.intc).reshape(-1)
        self._keep = (d, p, v, fl, footprints)
        fp = (C.c_void_p * max(1, len(footprints)))(*[None if f is None else f.data_ptr() for f in footprints])
        self._created(self._L.hx_catmap_create_sel(int(page_size), int(ncols), len(desc), d.ctypes.data, int(nsel), len(v),
                                                   p.ctypes.data if len(v) else None, v.ctypes.data if len(v) else None, self.nfilt,
                                                   fl.ctypes.data if self.nfilt else None, fp, mp))

    def page(self, n, cols, mask):
        self._lib.check(self._L.hx_catmap_page_sel(self._h, int(n), self._pointers(cols), self._lib.ptr(mask)))

    def moments(self):
        S, nf = self.nsel, self.nfield
        mom, bad = np.empty((S, nf, 4)), np.empty((S, nf, 6), dtype=np.int64)
        fcount = np.empty((S, self.nfilt + 1), dtype=np.int64)
        self._lib.check(self._L.hx_catmap_moments_sel(self._h, mom.ctypes.data, bad.ctypes.data, fcount.ctypes.data))
        return mom, bad, fcount

    def finish(self, s, f, norm, vis):
        self._lib.check(self._L.hx_catmap_finish_sel(self._h, int(s), int(f), float(norm), self._lib.ptr(vis)))


def _pack(masks, n, like):
    """The membership words of a page: bit s set where every mask term of selection s keeps the row (``masks[s]``: a list of boolean
    page masks, empty for a selection without any).  None when no selection has a mask term."""
    if not any(masks):
        return None
    if hasattr(like, "data_ptr") and like.is_cuda:
        import torch

        word = torch.zeros(n, dtype=torch.int32, device=like.device)
        for s, terms in enumerate(masks):
            keep = torch.ones(n, dtype=torch.bool, device=like.device)
            for m in terms:
                keep &= torch.as_tensor(m, device=like.device)
            word |= keep.to(torch.int32) << s
        return word
    word = np.zeros(n, dtype=np.uint32)
    for s, terms in enumerate(masks):
        keep = np.ones(n, dtype=bool)
        for m in terms:
            keep &= m.cpu().numpy() if hasattr(m, "data_ptr") else np.asarray(m, dtype=bool)
        word |= keep.astype(np.uint32) << np.uint32(s)
    return word


def _sel_terms(catalog, dtypes, fcols, mapped):
    """(predicates [(column, op, value)], mask terms) of a view's selection; the base itself selects every row.  A string compiles to
    predicates only while the view's predicates stay within _MAX_PREDICATES and their columns leave room for every field next to the
    filters' columns; otherwise it is a mask term (evaluated per page by the row-filter rule: the same rows)."""
    from .catalog import _flatten

    preds, masks = [], []
    for term in (() if catalog.base is None else _flatten(catalog.selection)):
        compiled = _compile_predicate(term, dtypes) if isinstance(term, str) else None
        if compiled is not None:
            trial = preds + compiled
            cols0 = list(dict.fromkeys([*fcols, *(c for c, _, _ in trial)]))
            if len(trial) > _MAX_PREDICATES or not _room(cols0, mapped):
                compiled = None
        if compiled is None:
            masks.append(term)
        else:
            preds.extend(compiled)
    return preds, masks


def _filter_error(fcount):
    n = int(fcount[-1])
    if n:
        return ValueError(f"map_catalogs: {n} positions have a latitude outside [-90, 90] or a non-finite coordinate in a footprint filter "
                          "(healpy: THETA is out of range [0,pi])")
    return None


def _map_selections(base, entries, terms, device, device_out):
    """One pass over the pages of ``base`` for the views ``entries`` -- [(key j, catalogue, items)] with the same mapped fields, and
    their ``terms`` (_sel_terms) --: {j: ({key: map}, error or None, [warning texts])}."""
    import torch

    from .catalog import CatalogPage, FootprintFilter, _chunk_mask

    filters = list(base.filters)
    pcols = [c for preds, _ in terms for c, _, _ in preds]
    cols0 = list(dict.fromkeys([*_filter_columns(base), *pcols]))
    done = {j: ({}, None, []) for j, _, _ in entries}
    cap = max(1, int(base.page_size))
    S = len(entries)
    for chunk, cols in _chunks(_mapped(entries[0][2]), cols0):
        index = {c: i for i, c in enumerate(cols)}
        fdesc, footprints = [], []
        for flt in filters:
            if isinstance(flt, FootprintFilter):
                fp = flt.footprint
                fp = (fp if hasattr(fp, "data_ptr") else torch.as_tensor(np.ascontiguousarray(np.asarray(fp), dtype=np.float64)))
                fp = fp.to(device=device, dtype=torch.float64).contiguous()
                fdesc.append([_FILTER_FOOTPRINT, index[flt.lonlat[0]], index[flt.lonlat[1]], flt.nside])
                footprints.append(fp)
            else:
                bits = 0
                for c in flt.columns:
                    bits |= 1 << index[c]
                fdesc.append([_FILTER_INVALID, bits, -1 if flt.weight is None else index[flt.weight], 0])
                footprints.append(None)
        preds, pval = [], []
        for s, (ps, _) in enumerate(terms):
            for c, op, v in ps:
                preds.append([s, index[c], op])
                pval.append(v)
        desc, maps = _context_inputs(chunk, cols, S, device)
        ctx = _CatMapSel(cap, len(cols), desc, S, preds, pval, fdesc, footprints, maps)
        try:
            for start in range(0, base.size, cap):
                stop = min(base.size, start + cap)
                page = base._page_columns(start, stop)
                view = CatalogPage(page)
                arrays = [_column(view[c], device) for c in cols]
                masks = [[_chunk_mask(t, page, start, stop) for t in m] for _, m in terms]
                ctx.page(stop - start, arrays, _pack(masks, stop - start, arrays[0]))
                del arrays, page, view, masks
            mom, bad, fcount = ctx.moments()
            for s, (j, cat, items) in enumerate(entries):
                res, err, warns = done[j]
                if err is None:
                    err = _filter_error(fcount[s])
                if err is None:
                    try:
                        _check_page_errors(chunk, bad[s])
                    except ValueError as e:
                        err = e
                for k, flt in enumerate(filters):
                    if not isinstance(flt, FootprintFilter) and flt.warn and fcount[s, k]:
                        _add_texts(warns, ["WARNING: catalog contains invalid values"])
                done[j] = (res, err, warns)
                if err is not None:
                    continue
                byname = {it.key[0]: it for it in items}
                for f, it0 in enumerate(chunk):
                    it = byname[it0.key[0]]
                    with _collect(warns):
                        finish, extra = _norm_and_visibility(it, mom[s, f], cat, device)
                    ctx.finish(s, f, *finish)
                    res[it.key] = _result(it, maps[s * len(chunk) + f], cat, extra, device_out)
        finally:
            ctx.close()
    return done


def _sel_groups(entries, terms, fcols, device):
    """Split one base's views [(j, catalogue, items)] and their terms into passes, in order: at most _MAX_SELECTIONS views, the maps
    within the budget, at most _MAX_PREDICATES predicates, and predicate columns that leave room for every field next to ``fcols``."""
    if not entries:
        return []
    mapped = _mapped(entries[0][2])
    per_view = sum(8 * (2 if it.kind == _COMPLEX else 1) * 12 * it.mapper.nside**2 for it in mapped)
    most = max(1, min(_MAX_SELECTIONS, _map_budget(device) // max(1, per_view)))
    parts, cur, npred, pcols = [], [], 0, []
    for entry, term in zip(entries, terms):
        mine = [c for c, _, _ in term[0]]
        cols0 = list(dict.fromkeys([*fcols, *pcols, *mine]))
        if cur and (len(cur) == most or npred + len(term[0]) > _MAX_PREDICATES or not _room(cols0, mapped)):
            parts.append(cur)
            cur, npred, pcols = [], 0, []
        cur.append((entry, term))
        npred += len(term[0])
        pcols.extend(c for c in mine if c not in pcols)
    parts.append(cur)
    return parts


def _plan_groups(fields, catalogs, include, exclude):
    """{j: (base, field names)} for the catalogues that go through one-pass groups; a group is used when it holds a view or the base
    has filters (a plain catalogue keeps the per-catalogue path)."""
    from .catalog import CatalogView

    members = {}
    for j, catalog in catalogs.items():
        base = _sel_base(catalog)
        if base is None:
            continue
        names = tuple(i for i in fields if toc_match((i, j), include, exclude))
        if names:
            members.setdefault((id(base), names), []).append(j)
    plan = {}
    for (bid, names), js in members.items():
        base = _sel_base(catalogs[js[0]])
        fcols = set(_filter_columns(base))
        for i in names:  # every field must fit one context next to the filters' columns, else the per-catalogue path
            if len(fcols | set(_read(getattr(fields[i], "columns", None) or ()))) > _MAX_COLUMNS:
                break
        else:
            if base.filters or any(isinstance(catalogs[j], CatalogView) for j in js):
                for j in js:
                    plan[j] = (base, names)
    return plan


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
    plan = _plan_groups(fields, catalogs, include, exclude)
    staged = {}  # j -> ({key: map}, error, warning texts) of the one-pass groups, emitted in the order of the catalogues
    for j, catalog in catalogs.items():
        if j in plan and j not in staged:
            if dev is None:
                dev = _device_of(device)
            _run_group(fields, catalogs, plan, j, include, exclude, dev, device is not None, staged)
        if j in staged:
            results, err, warns = staged.pop(j)
            for text in warns:
                warnings.warn(text)
            if err is not None:
                raise err
        else:
            items = [_item((i, j), field, catalog) for i, field in fields.items() if toc_match((i, j), include, exclude)]
            if not items:
                continue
            if dev is None:
                dev = _device_of(device)
            results = _map_catalog(items, catalog, dev, device is not None)
        for key in list(results):
            out[key] = results.pop(key)
            current += 1
            if progress is not None:
                progress.update(current, total)
    return out


def _run_group(fields, catalogs, plan, first, include, exclude, device, device_out, staged):
    """Maps every catalogue of the group of ``first`` in one pass per split, into ``staged``; the item checks of each catalogue run
    first, and a catalogue that fails them keeps its error (raised in its turn)."""
    base, names = plan[first]
    entries = []
    for j, catalog in catalogs.items():
        if plan.get(j) is None or plan[j][0] is not base or plan[j][1] != names:
            continue
        try:
            items = [_item((i, j), fields[i], catalog) for i in names]
        except (ValueError, TypeError, NotImplementedError) as e:
            staged[j] = ({}, e, [])
            continue
        warns = []
        staged[j] = (_map_visibility(items, catalog, device, device_out, warns), None, warns)
        entries.append((j, catalog, items))
    mapped = _mapped(entries[0][2]) if entries else []
    if not mapped:
        for j, _, items in entries:
            staged[j] = ({it.key: staged[j][0][it.key] for it in items}, None, staged[j][2])
        return
    dtypes, fcols = _dtypes(base), _filter_columns(base)
    terms = [_sel_terms(cat, dtypes, fcols, mapped) for _, cat, _ in entries]
    for part in _sel_groups(entries, terms, fcols, device):
        done = _map_selections(base, [e for e, _ in part], [t for _, t in part], device, device_out)
        for (j, catalog, items), _ in part:
            res, err, new = done[j]
            vis_res, _, warns = staged[j]
            _add_texts(warns, new)
            allres = {**vis_res, **res}
            staged[j] = ({it.key: allres[it.key] for it in items} if err is None else {}, err, warns)
