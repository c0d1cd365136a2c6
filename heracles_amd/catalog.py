"""A minimal in-memory catalogue with the page protocol ``map_catalogs`` reads (that of heracles/catalog/base.py:46-199).

``ArrayCatalog`` wraps a numpy structured array, or a mapping from column name to a 1-D numpy array or a contiguous float64 CUDA
tensor.  Pages are slices of the columns: device columns stay in HBM and reach the kernels without a copy.  Any other object with the
same protocol -- iteration over pages with ``get`` / ``[col]`` / ``size`` / ``delete``, and ``visibility``, ``fsky``, ``metadata``,
``size``, ``page_size`` -- works as well, a ``heracles.FitsCatalog`` among them.  ``heracles_amd.fitscatalog.FitsCatalog`` is this
class with a FITS table as its source of pages.

``where`` / ``[]`` give ``CatalogView``s (heracles/catalog/base.py:204-310) and ``add_filter`` takes ``InvalidValueFilter`` and
``FootprintFilter`` (heracles/catalog/filters.py); ``map_catalogs`` maps the views of one ``ArrayCatalog`` in one pass over its pages
(``_column_dtypes`` / ``_page_columns`` are the page source it reads).
"""

from __future__ import annotations

import math
import warnings
from types import MappingProxyType

import numpy as np

__all__ = ["ArrayCatalog", "CatalogPage", "CatalogView", "FootprintFilter", "InvalidValueFilter"]


def _is_tensor(x):
    return hasattr(x, "data_ptr")


def _fsky_of(vis):
    """heracles/catalog/base.py:36-44: the mean of a visibility map; a_00 / sqrt(4 pi) of visibility alms (a complex array)."""
    if _is_tensor(vis):
        if vis.is_complex():
            return float(vis[0].real) / (4 * np.pi) ** 0.5
        return float(vis.mean())
    if np.iscomplexobj(vis):
        return vis[0].real / (4 * np.pi) ** 0.5
    return vis.mean()


def _nonzero(mask):
    """Row indices where ``mask`` is true: numpy indices, or a device index tensor."""
    if _is_tensor(mask):
        return mask.nonzero().flatten()
    return np.where(mask)[0]


def rowfilter(columns, expr):
    """The reference's row filter (heracles/catalog/fits.py:34-36): ``expr`` evaluated with the columns as names."""
    return eval(expr, None, dict(columns))


def _check_selection(selection, size):
    """A selection is a boolean mask of catalogue length (numpy, or a CUDA bool tensor), a row-filter string, or a tuple of these
    joined with ``&``; anything else -- integer index arrays included, which would reorder rows -- raises ``TypeError``."""
    if isinstance(selection, tuple):
        for s in selection:
            _check_selection(s, size)
        return
    if isinstance(selection, str):
        return
    if _is_tensor(selection):
        import torch

        if selection.dtype != torch.bool or selection.ndim != 1:
            raise TypeError("ArrayCatalog: a selection tensor must be a 1-D boolean mask")
        if len(selection) != size:
            raise ValueError(f"ArrayCatalog: selection mask of length {len(selection)} for a catalogue of {size} rows")
        return
    if isinstance(selection, np.ndarray) and selection.dtype == np.bool_ and selection.ndim == 1:
        if len(selection) != size:
            raise ValueError(f"ArrayCatalog: selection mask of length {len(selection)} for a catalogue of {size} rows")
        return
    raise TypeError(f"ArrayCatalog: cannot select rows with {type(selection).__name__!r}: a selection is a boolean mask of catalogue "
                    "length, a row-filter string, or a tuple of these")


def _flatten(selection):
    if isinstance(selection, (tuple, list)):
        return tuple(t for s in selection for t in _flatten(s))
    return () if selection is None else (selection,)


def _chunk_mask(term, columns, start, stop):
    """The rows [start, stop) that one selection term keeps."""
    if isinstance(term, str):
        m = rowfilter(columns, term)
        if _is_tensor(m):
            return m.to(bool)
        return np.asarray(m, dtype=bool)
    return term[start:stop]


class CatalogPage:
    """One batch of rows: ``page[col]`` without checks, ``page.get(*cols)`` with the reference's NaN check, ``delete(where)``."""

    def __init__(self, data):
        self._data = dict(data)
        sizes = {len(v) for v in self._data.values()}
        if len(sizes) > 1:
            raise ValueError("inconsistent row length")
        self._size = sizes.pop() if sizes else 0

    def _column(self, name):
        if name[:1] == "-":
            return -self._data[name[1:]]
        return self._data[name]

    def __getitem__(self, col):
        if isinstance(col, (list, tuple)):
            return tuple(self._column(c) for c in col)
        return self._column(col)

    def __iter__(self):
        yield from self._data

    def __len__(self):
        return len(self._data)

    @property
    def names(self):
        return list(self._data)

    @property
    def size(self):
        return self._size

    def get(self, *cols):
        out = []
        for c in cols:
            v = self._column(c)
            nan = bool(v.isnan().any()) if _is_tensor(v) else bool(np.any(np.isnan(v)))
            if nan:
                raise ValueError(f'invalid values in column "{c}"')
            out.append(v)
        return out[0] if len(out) == 1 else out

    def delete(self, where):
        for name, v in self._data.items():
            if _is_tensor(v):
                import torch

                keep = torch.ones(len(v), dtype=torch.bool, device=v.device)
                keep[torch.as_tensor(where, device=v.device)] = False
                self._data[name] = v[keep]
            else:
                self._data[name] = np.delete(v, where)
        self._size = len(next(iter(self._data.values()))) if self._data else 0


class _CatalogBase:
    """What ``ArrayCatalog`` and ``FitsCatalog`` share: ``page_size``, ``visibility`` and ``fsky``, the metadata, the filters, and ``[]`` /
    iteration in terms of the ``where`` and ``select`` each of them defines.  ``map_catalogs`` maps the views of either in one pass, through
    ``_column_dtypes()`` and ``_page_columns(start, stop)``."""

    def _setup(self, page_size, visibility, metadata):
        self.page_size = int(page_size)
        self.visibility = visibility
        self._metadata = {"catalog": None, **dict(metadata or {})}
        self._filters = []

    @property
    def page_size(self):
        return self._page_size

    @page_size.setter
    def page_size(self, value):
        if value < 1:
            raise ValueError("page_size must be positive")
        self._page_size = int(value)

    @property
    def metadata(self):
        return MappingProxyType(self._metadata)

    @property
    def label(self):
        return self._metadata.get("catalog")

    @property
    def fsky(self):
        vis = self.visibility
        return None if vis is None else _fsky_of(vis)

    @property
    def base(self):
        """``None``: this is not a view."""
        return None

    @property
    def selection(self):
        """``None``: this is not a view."""
        return None

    @property
    def filters(self):
        """Filters applied, in order, to every page the catalogue and its views yield (heracles/catalog/base.py:454-466)."""
        return self._filters

    @filters.setter
    def filters(self, filters):
        self._filters = filters

    def add_filter(self, filt):
        self._filters.append(filt)

    def __getitem__(self, where):
        return self.where(where)

    def __iter__(self):
        yield from self.select(None)


class ArrayCatalog(_CatalogBase):
    """Catalogue of in-memory columns, read in pages of ``page_size`` rows.  ``fsky`` is the mean of the visibility, if one is set
    (heracles/catalog/base.py:36-44), else ``None``."""

    default_page_size = 1_000_000

    def __init__(self, data, *, page_size=default_page_size, visibility=None, metadata=None):
        if isinstance(data, np.ndarray):
            if data.dtype.names is None:
                raise TypeError("ArrayCatalog: a numpy array must be structured (one field per column)")
            cols = {name: data[name] for name in data.dtype.names}
        else:
            cols = dict(data)
        for name, v in cols.items():
            if _is_tensor(v):
                import torch

                if v.ndim != 1 or v.dtype != torch.float64 or not v.is_contiguous():
                    raise ValueError(f"column {name!r}: device columns must be 1-D contiguous float64 tensors")
            elif np.ndim(v) != 1:
                raise ValueError(f"column {name!r} is not 1-D")
        sizes = {len(v) for v in cols.values()}
        if len(sizes) > 1:
            raise ValueError("inconsistent row length")
        self._cols = cols
        self._size = sizes.pop() if sizes else 0
        self._setup(page_size, visibility, metadata)

    @property
    def names(self):
        return list(self._cols)

    @property
    def size(self):
        return self._size

    def _join(self, *where):
        """Selections join lazily: a flat tuple of terms, ANDed row by row."""
        joined = _flatten(where)
        _check_selection(joined, self._size)
        return joined

    def where(self, selection, visibility=None):
        """A view of the rows ``selection`` keeps (heracles/catalog/base.py:438-442)."""
        if isinstance(selection, (tuple, list)):
            selection = self._join(*selection)
        else:
            _check_selection(selection, self._size)
        return CatalogView(self, selection, visibility)

    # the page source ``map_catalogs`` reads when it maps the views of one base in one pass
    def _column_dtypes(self):
        """{column: dtype} of the columns as the pages hold them (device columns are float64)."""
        return {name: (np.float64 if _is_tensor(v) else np.asarray(v).dtype) for name, v in self._cols.items()}

    def _page_columns(self, start, stop):
        """{column: rows [start, stop)} before any selection or filter."""
        return {name: v[start:stop] for name, v in self._cols.items()}

    def _mask(self, selection, start, stop):
        """The rows [start, stop) of the catalogue that ``selection`` keeps, or ``None`` for all."""
        mask = None
        cols = None
        for term in _flatten(selection):
            if isinstance(term, str) and cols is None:
                cols = {name: v[start:stop] for name, v in self._cols.items()}
            m = _chunk_mask(term, cols, start, stop)
            if mask is None:
                mask = m
            elif _is_tensor(mask) or _is_tensor(m):
                import torch

                dev = mask.device if _is_tensor(mask) else m.device
                mask = torch.as_tensor(mask, device=dev) & torch.as_tensor(m, device=dev)
            else:
                mask = mask & m
        return mask

    def _selected(self, selection):
        """The columns of the selected rows, in catalogue order."""
        if not _flatten(selection):
            return self._cols
        parts = {name: [] for name in self._cols}
        for i in range(0, self._size, self._page_size):
            j = min(self._size, i + self._page_size)
            mask = self._mask(selection, i, j)
            for name, v in self._cols.items():
                chunk = v[i:j]
                if _is_tensor(chunk) and not _is_tensor(mask):
                    import torch

                    mask = torch.as_tensor(mask, device=chunk.device)
                elif _is_tensor(mask) and not _is_tensor(chunk):
                    mask = mask.cpu().numpy()
                parts[name].append(chunk[mask])
        out = {}
        for name, ps in parts.items():
            if ps and _is_tensor(ps[0]):
                import torch

                out[name] = torch.cat(ps)
            else:
                out[name] = np.concatenate(ps) if ps else self._cols[name][:0]
        return out

    def _size_of(self, selection):
        if not _flatten(selection):
            return self._size
        n = 0
        for i in range(0, self._size, self._page_size):
            m = self._mask(selection, i, min(self._size, i + self._page_size))
            n += int(m.sum())
        return n

    def select(self, selection):
        """Pages of the rows ``selection`` keeps, cut every ``page_size`` selected rows, with the filters applied to each page."""
        cols = self._selected(selection)
        size = len(next(iter(cols.values()))) if cols else 0
        for i in range(0, size, self._page_size):
            page = CatalogPage({name: v[i : i + self._page_size] for name, v in cols.items()})
            for filt in self._filters:
                filt(page)
            yield page


class CatalogView:
    """The rows of a base catalogue that a selection keeps (heracles/catalog/base.py:204-310), with a visibility of its own if one is
    set.  ``map_catalogs`` maps the views of one ``ArrayCatalog`` in one pass over the base's pages."""

    def __init__(self, catalog, selection, visibility=None, fsky=None):
        self._catalog = catalog
        self._selection = selection
        self._visibility = visibility
        self._fsky = fsky
        if fsky is None and visibility is not None:
            self._fsky = _fsky_of(visibility)

    def __repr__(self):
        return f"{self._catalog!r}[{self._selection!r}]"

    def __str__(self):
        return f"{self._catalog!s}[{self._selection!s}]"

    def __getitem__(self, where):
        return self.where(where)

    @property
    def base(self):
        return self._catalog

    @property
    def metadata(self):
        return self._catalog.metadata

    @property
    def label(self):
        return self._catalog.label

    @property
    def selection(self):
        return self._selection

    @property
    def names(self):
        return self._catalog.names

    @property
    def size(self):
        """Rows the selection keeps (before the base's filters)."""
        return self._catalog._size_of(self._selection)

    @property
    def visibility(self):
        if self._visibility is None:
            return self._catalog.visibility
        return self._visibility

    @visibility.setter
    def visibility(self, visibility):
        self._visibility = visibility
        self._fsky = None if visibility is None else _fsky_of(visibility)

    @property
    def fsky(self):
        if self._fsky is None:
            return self._catalog.fsky
        return self._fsky

    @fsky.setter
    def fsky(self, fsky):
        self._fsky = fsky

    def _joined(self, selection):
        if isinstance(selection, (tuple, list)):
            return (self._selection, *selection)
        return (self._selection, selection)

    def where(self, selection, visibility=None):
        if visibility is None:
            visibility = self._visibility
        return self._catalog.where(self._joined(selection), visibility)

    @property
    def page_size(self):
        return self._catalog.page_size

    def __iter__(self):
        yield from self._catalog.select(self._selection)

    def select(self, selection):
        yield from self._catalog.select(self._joined(selection))


class InvalidValueFilter:
    """Removes the rows with a NaN in one of ``columns`` (and, if ``weight`` is given, a non-zero weight) from every page
    (heracles/catalog/filters.py:25-59)."""

    def __init__(self, *columns, weight=None, warn=True):
        self.columns = columns
        self.weight = weight
        self.warn = warn

    def __repr__(self):
        name = self.__class__.__name__
        args = list(map(repr, self.columns))
        args += [f"weight={self.weight!r}", f"warn={self.warn!r}"]
        return f"{name}({', '.join(args)})"

    def __call__(self, page):
        invalid = None
        for col in self.columns:
            v = page[col]
            bad = v.isnan() if _is_tensor(v) else np.isnan(v)
            invalid = bad if invalid is None else invalid | bad
        if invalid is None:
            return
        if self.weight is not None:
            invalid = invalid & (page[self.weight] != 0)
        rows = _nonzero(invalid)
        if len(rows) > 0:
            if self.warn:
                warnings.warn("WARNING: catalog contains invalid values")
            page.delete(rows)


class FootprintFilter:
    """Removes the rows outside a footprint map, ``footprint[ang2pix(nside, lon, lat)] == 0``, from every page
    (heracles/catalog/filters.py:62-99).  The footprint is a RING map, numpy or a device tensor; its nside follows from its size."""

    def __init__(self, footprint, lon, lat):
        npix = len(footprint)
        nside = math.isqrt(npix // 12)
        if npix < 12 or 12 * nside * nside != npix:
            raise ValueError(f"FootprintFilter: a footprint of {npix} pixels is not a HEALPix map (12 nside^2 pixels)")
        self._footprint = footprint
        self._nside = nside
        self._lonlat = (lon, lat)

    @property
    def footprint(self):
        return self._footprint

    @property
    def lonlat(self):
        return self._lonlat

    @property
    def nside(self):
        return self._nside

    def __repr__(self):
        lon, lat = self.lonlat
        return f"{self.__class__.__name__}(..., {lon!r}, {lat!r})"

    def __call__(self, page):
        from .mapper import ang2pix_ring

        lon, lat = self._lonlat
        ipix = ang2pix_ring(self._nside, page[lon], page[lat])
        fp = self._footprint
        if _is_tensor(ipix):
            import torch

            fp = torch.as_tensor(fp, device=ipix.device)
        elif _is_tensor(fp):
            fp = fp.cpu().numpy()
        page.delete(_nonzero(fp[ipix] == 0))
