"""A minimal in-memory catalogue with the page protocol ``map_catalogs`` reads (that of heracles/catalog/base.py:46-199).

``ArrayCatalog`` wraps a numpy structured array, or a mapping from column name to a 1-D numpy array or a contiguous float64 CUDA
tensor.  Pages are slices of the columns: device columns stay in HBM and reach the kernels without a copy.  Any other object with the
same protocol -- iteration over pages with ``get`` / ``[col]`` / ``size`` / ``delete``, and ``visibility``, ``fsky``, ``metadata``,
``size``, ``page_size`` -- works as well, a ``heracles.FitsCatalog`` among them.
"""

from __future__ import annotations

from types import MappingProxyType

import numpy as np

__all__ = ["ArrayCatalog", "CatalogPage"]


def _is_tensor(x):
    return hasattr(x, "data_ptr")


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


class ArrayCatalog:
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
        self.page_size = int(page_size)
        self.visibility = visibility
        self._metadata = {"catalog": None, **dict(metadata or {})}

    @property
    def page_size(self):
        return self._page_size

    @page_size.setter
    def page_size(self, value):
        if value < 1:
            raise ValueError("page_size must be positive")
        self._page_size = int(value)

    @property
    def names(self):
        return list(self._cols)

    @property
    def size(self):
        return self._size

    @property
    def metadata(self):
        return MappingProxyType(self._metadata)

    @property
    def label(self):
        return self._metadata.get("catalog")

    @property
    def fsky(self):
        vis = self.visibility
        if vis is None:
            return None
        if _is_tensor(vis):
            return float(vis.mean())
        return vis.mean()

    def __iter__(self):
        for i in range(0, self._size, self._page_size):
            yield CatalogPage({name: v[i : i + self._page_size] for name, v in self._cols.items()})
