"""``FitsCatalog``: a catalogue read from a FITS binary table, page by page, into HBM (heracles/catalog/fits.py:39-170).

The reference reads its catalogues through ``fitsio``; neither ``fitsio`` nor ``astropy`` is a requirement of this package, so the
table is read here from the FITS standard, with the header parser of ``heracles_amd.fits``.  A page is ``page_size`` records of the
file: the raw big-endian bytes are read with one ``readinto`` into page-locked memory, uploaded once, and decoded on the GPU
(``hx_fits_unpack_columns``) into one contiguous float64 CUDA tensor per column -- what ``ArrayCatalog`` asks of device columns, so
``map_catalogs`` and the filters take the pages as they are.  While page k is uploaded and decoded, one reader thread reads page k+1
into the second staging buffer.

Read: scalar columns of TFORM ``L`` (``'T'`` is 1.0, anything else 0.0), ``B``, ``I``, ``J``, ``K``, ``E`` and ``D``, with ``TSCAL``
/ ``TZERO`` applied as numpy would (``stored * TSCAL + TZERO``, two roundings); ``K`` values beyond +-2^53 round as a C cast does.
Not read: strings, bit arrays, complex and vector columns, variable-length arrays (requesting one raises ``TypeError``; they are left
out of ``names`` otherwise), compressed files (``ValueError``).  ``TNULL`` is not interpreted, as ``fitsio`` does not by default.
Parity with fitsio-written files is pinned on the FITS standard only, as for maps and alms (``heracles_amd.fits``).
"""

from __future__ import annotations

import ctypes as C
import os
import re
import threading
from collections import OrderedDict

import numpy as np

from . import _lib
from .catalog import ArrayCatalog, CatalogPage, CatalogView, _CatalogBase, _check_selection, _chunk_mask, _flatten, _is_tensor
from .fits import _scan

__all__ = ["FitsCatalog"]

_MAX_COLUMNS = 64  # HX_FITS_MAX_COLUMNS of include/hxsht.h: columns of one hx_fits_unpack_columns call
# bytes of one element of every TFORM letter of the standard (X: bits; P / Q: array descriptors)
_ELEMENT = {"L": 1, "X": 0, "B": 1, "I": 2, "J": 4, "K": 8, "A": 1, "E": 4, "D": 8, "C": 8, "M": 16, "P": 8, "Q": 16}
_SCALARS = "LBIJKED"


def _fields(h):
    """[(name, TFORM, letter, repeat, byte offset, TSCAL, TZERO)] of every field of a binary-table header, in file order."""
    out, off = [], 0
    for i in range(1, h["TFIELDS"] + 1):
        tform = str(h[f"TFORM{i}"]).strip()
        m = re.match(r"(\d*)([LXBIJKAEDCMPQ])", tform)
        if not m:
            raise ValueError(f"column {i} has an invalid TFORM {tform!r}")
        repeat, letter = int(m.group(1) or 1), m.group(2)
        name = str(h.get(f"TTYPE{i}", f"COL{i}")).strip()
        out.append((name, tform, letter, repeat, off, float(h.get(f"TSCAL{i}", 1)), float(h.get(f"TZERO{i}", 0))))
        off += (repeat + 7) // 8 if letter == "X" else repeat * _ELEMENT[letter]
    if off != h["NAXIS1"]:
        raise ValueError(f"the columns take {off} bytes of a record, NAXIS1 is {h['NAXIS1']}")
    return out


def _readable(field):
    return field[2] in _SCALARS and field[3] == 1


class _Read:
    """One page of raw records on its way into a staging buffer; ``thread`` is None when it was read by the caller."""

    def __init__(self, key, buf):
        self.key, self.buf, self.thread, self.error = key, buf, None, None

    def wait(self):
        if self.thread is not None:
            self.thread.join()
            self.thread = None
        if self.error is not None:
            raise self.error


class FitsCatalog(_CatalogBase):
    """Catalogue of the rows of a FITS binary table; what is not about the file -- ``page_size``, ``visibility``, ``fsky``, ``metadata``,
    ``label``, ``filters`` / ``add_filter``, ``[]`` -- is shared with ``ArrayCatalog``, and ``where`` gives the same ``CatalogView``s.

    ``columns``: the columns to read (default: every readable scalar column, in file order).  ``ext``: HDU index or ``EXTNAME``
    (default: the first binary table that has rows; ``TypeError("no table data in FITS")`` if there is none).  Construction neither
    opens nor reads the file.

    Pages are cut every ``page_size`` rows *of the file* and then selected and filtered, as the reference's ``_pages`` does; a page of
    a view can therefore hold fewer rows than ``page_size``, where ``ArrayCatalog.select`` cuts every ``page_size`` *selected* rows.
    The last ``READ_CACHE`` decoded pages are kept, so views iterated one after the other share what was read; ``bytes_read`` counts
    the bytes of table data read from the file.  The kept pages hold HBM -- ``READ_CACHE`` x ``page_size`` x 8 bytes for every column
    read, so name the ``columns`` that are needed -- until ``release()`` or the end of the catalogue object.  One catalogue object is iterated from one thread at a time.
    """

    READ_CACHE = 3

    def __init__(self, path, *, columns=None, ext=None, page_size=ArrayCatalog.default_page_size, visibility=None, metadata=None):
        self._path = path
        self._columns = None if columns is None else list(columns)
        self._ext = ext
        self._setup(page_size, visibility, metadata)
        self._reset()

    def _reset(self):
        self._table = None  # (payload offset, NAXIS1, NAXIS2, [(name, letter, offset, TSCAL, TZERO)] of the columns read)
        self._cache = OrderedDict()  # (start, stop) -> {name: tensor}
        self._stage = [None, None]
        self._turn = 0
        self._pending = None
        self.bytes_read = 0

    def release(self):
        """Drops the cached pages and the staging buffers (they come back with the next read)."""
        if self._pending is not None and self._pending.thread is not None:
            self._pending.thread.join()
        self._cache.clear()
        self._stage, self._pending = [None, None], None

    def __copy__(self):
        """A shallow copy: its own list of filters and its own page cache (heracles/catalog/base.py:327-336)."""
        other = self.__class__.__new__(self.__class__)
        other._path, other._columns, other._ext = self._path, self._columns, self._ext
        other._page_size, other.visibility = self._page_size, self.visibility
        other._metadata = dict(self._metadata)
        other._filters = self._filters.copy()
        other._reset()
        return other

    def __repr__(self):
        s = str(self._path)
        if self._ext is not None:
            s += f"[{self._ext!r}]"
        return s

    @property
    def path(self):
        return self._path

    # ---- the table ------------------------------------------------------------------------------------------------------------------
    def _hdu(self):
        """(header, payload offset) of the catalogue's HDU."""
        path = os.fspath(self._path)
        with open(path, "rb") as f:
            magic = f.read(6)
        if magic[:2] == b"\x1f\x8b":
            raise ValueError(f"{path}: the file is gzip-compressed; compressed FITS files are not read")
        if magic != b"SIMPLE":
            raise ValueError(f"{path}: not a FITS file")
        hdus = _scan(path)
        table = lambda h: str(h.get("XTENSION", "")).strip() == "BINTABLE"
        if self._ext is None:
            found = next(((h, off) for h, off in hdus if table(h) and h.get("NAXIS2", 0) > 0), None)
            if found is None:
                raise TypeError("no table data in FITS")
        elif isinstance(self._ext, (int, np.integer)):
            if not 0 <= self._ext < len(hdus):
                raise IndexError(f"{path}: no HDU {self._ext} (the file has {len(hdus)})")
            found = hdus[self._ext]
        else:
            want = str(self._ext).strip().upper()
            found = next(((h, off) for h, off in hdus if str(h.get("EXTNAME", "")).strip().upper() == want), None)
            if found is None:
                raise KeyError(f"{path}: no extension named {self._ext!r}")
        h = found[0]
        if h.get("ZIMAGE") is True or h.get("ZTABLE") is True:
            raise ValueError(f"{self!r}: the HDU is tile-compressed ({'ZIMAGE' if h.get('ZIMAGE') is True else 'ZTABLE'}); compressed "
                             "FITS data are not read")
        if not table(h):
            raise TypeError(f"{self!r}: the HDU is not a binary table")
        return found

    def _layout(self):
        if self._table is None:
            h, off = self._hdu()
            fields = _fields(h)
            if self._columns is None:
                chosen = [f for f in fields if _readable(f)]
            else:
                byname = {f[0]: f for f in reversed(fields)}
                upper = {f[0].upper(): f for f in reversed(fields)}  # (column names are case-insensitive in FITS)
                chosen = []
                for name in self._columns:
                    f = byname.get(name) or upper.get(str(name).upper())
                    if f is None:
                        raise ValueError(f"{self!r}: no column {name!r} in the table")
                    if not _readable(f):
                        raise TypeError(f"{self!r}: column {name!r} has TFORM {f[1]!r}: only scalar columns of type L, B, I, J, K, E "
                                        "and D can be read")
                    chosen.append((name, *f[1:]))
            self._table = (off, int(h["NAXIS1"]), int(h["NAXIS2"]), [(f[0], f[2], f[4], f[5], f[6]) for f in chosen])
        return self._table

    @property
    def names(self):
        if self._columns is not None:
            return list(self._columns)
        return [c[0] for c in self._layout()[3]]

    @property
    def size(self):
        return self._layout()[2]


    # ---- selections ---------------------------------------------------------------------------------------------------------------------
    def _size_for(self, selection):
        """The table's length if ``selection`` holds a mask to check against it; row-filter strings leave the file unopened."""
        return self.size if any(not isinstance(t, str) for t in _flatten(selection)) else 0

    def _join(self, *where):
        joined = _flatten(where)
        _check_selection(joined, self._size_for(joined))
        return joined

    def where(self, selection, visibility=None):
        if isinstance(selection, (tuple, list)):
            selection = self._join(*selection)
        else:
            _check_selection(selection, self._size_for(selection))
        return CatalogView(self, selection, visibility)

    def _mask_of(self, selection, cols, start, stop):
        """The rows of the page [start, stop) with columns ``cols`` that ``selection`` keeps, as a device mask, or None for all."""
        import torch

        mask = None
        for term in _flatten(selection):
            m = _chunk_mask(term, cols, start, stop)
            if not _is_tensor(m) or not m.is_cuda:
                m = torch.as_tensor(m, device=next(iter(cols.values())).device)
            mask = m if mask is None else mask & m
        return mask

    def _size_of(self, selection):
        if not _flatten(selection):
            return self.size
        return sum(int(self._mask_of(selection, cols, start, stop).sum()) for start, stop, cols in self._pages())

    def select(self, selection):
        """Pages of ``page_size`` rows of the file, each reduced to the rows ``selection`` keeps, with the filters applied."""
        for start, stop, cols in self._pages():
            mask = self._mask_of(selection, cols, start, stop)
            if mask is not None:
                cols = {name: v[mask] for name, v in cols.items()}
            page = CatalogPage(cols)
            for filt in self._filters:
                filt(page)
            yield page

    # ---- the page source of map_catalogs' one-pass path ----------------------------------------------------------------------------------
    def _column_dtypes(self):
        return dict.fromkeys(self.names, np.float64)

    def _page_columns(self, start, stop):
        ahead = min(self.size, stop + (stop - start))
        return self._decoded(start, stop, (stop, ahead) if ahead > stop else None)

    # ---- reading -------------------------------------------------------------------------------------------------------------------------
    def _pages(self):
        """(start, stop, columns) of every ``page_size`` rows of the file."""
        size, step = self.size, self._page_size
        for start in range(0, size, step):
            stop = min(size, start + step)
            yield start, stop, self._page_columns(start, stop)

    def _fill(self, read):
        """Reads the records of ``read.key`` into its staging buffer."""
        try:
            off, width, _, _ = self._layout()
            start, stop = read.key
            want = memoryview(read.buf)[: (stop - start) * width]
            with open(os.fspath(self._path), "rb", buffering=0) as f:
                f.seek(off + start * width)
                got = 0
                while got < len(want):  # (one readinto; the kernel caps a single read at 2 GiB)
                    n = f.readinto(want[got:])
                    if not n:
                        raise ValueError(f"{self!r}: the file ends inside the table")
                    got += n
                    self.bytes_read += n
        except Exception as e:  # noqa: BLE001 -- raised again by the thread that asked for the page (_Read.wait)
            read.error = e

    def _start(self, key, thread):
        """Starts reading the rows ``key`` into the staging buffer whose turn it is: on the reader thread, or here."""
        i, self._turn = self._turn, 1 - self._turn
        nbytes = (key[1] - key[0]) * self._layout()[1]
        if self._stage[i] is None or self._stage[i].nbytes < nbytes:
            self._stage[i] = _lib.pinned_empty(nbytes, np.uint8)
        read = _Read(key, self._stage[i])
        if thread:
            read.thread = threading.Thread(target=self._fill, args=(read,), name="FitsCatalog-reader")
            read.thread.start()
        else:
            self._fill(read)
        return read

    def _decoded(self, start, stop, ahead=None):
        """{name: float64 CUDA tensor} of the rows [start, stop); ``ahead``: the rows the reader thread fetches meanwhile."""
        key = (start, stop)
        cols = self._cache.get(key)
        if cols is not None:
            self._cache.move_to_end(key)
            return cols
        read, self._pending = self._pending, None
        if read is not None and read.key != key:  # (a page nobody came for: its buffer is free once the thread is done)
            read.wait()
            read = None
        if read is None:
            read = self._start(key, False)
        read.wait()
        if ahead is not None and ahead not in self._cache:
            self._pending = self._start(ahead, True)
        cols = self._decode(read.buf, stop - start)
        self._cache[key] = cols
        while len(self._cache) > self.READ_CACHE:
            self._cache.popitem(last=False)
        return cols

    def _decode(self, buf, nrows):
        """The page-locked records go to the library as they are: one asynchronous upload, the kernel behind it on the same stream, one
        synchronisation (a table of more than _MAX_COLUMNS columns is uploaded once per group of them).  The columns live on the
        library's device."""
        import torch

        _, width, _, columns = self._layout()
        device = torch.device("cuda", _lib.device())
        raw = buf[: nrows * width]
        out = {name: torch.empty(nrows, dtype=torch.float64, device=device) for name, *_ in columns}
        L = _lib.load()
        for k in range(0, len(columns), _MAX_COLUMNS):
            part = columns[k : k + _MAX_COLUMNS]
            offsets = np.array([c[2] for c in part], dtype=np.int64)
            tscal = np.array([c[3] for c in part], dtype=np.float64)
            tzero = np.array([c[4] for c in part], dtype=np.float64)
            ptrs = (C.c_void_p * len(part))(*[_lib.ptr(out[c[0]]).value for c in part])
            _lib.check(L.hx_fits_unpack_columns(nrows, width, len(part), offsets.ctypes.data, "".join(c[1] for c in part).encode(),
                                                tscal.ctypes.data, tzero.ctypes.data, _lib.ptr(raw), ptrs, 0))
        return out
