"""HEALPix pixel window functions for ``HipHealpixMapper`` (``hp.pixwin(nside, lmax=lmax, pol=True)``, heracles/healpy.py:104-115
with ``deconvolve=True``, the reference's default), computed on the GPU for any spin weight, and healpy's window files.

The quantity.  For pixel p of area Omega = 4 pi / (12 nside^2) and spin weight s, A_lm(p) = (1 / Omega) int_p sY_lm dOmega is the
pixel average in the local (theta, phi) basis -- what ``map_values`` forms from catalogue values.  The window is

    W_l^(s)^2 = 4 pi / ((2l+1) 12 nside^2)  sum_p sum_{m=-l..l} |A_lm(p)|^2   for l >= s,      W_l = 1 for l < s.

For s = 0 this is the definition of the HEALPix primer (W_0 = 1).  For s != 0 it is the total-power window of the pixel-averaged
field: one array, applied to E and B alike as the mapper does with healpy's polarisation column; the E/B mixing that pixel averaging
causes is not modelled.  ``compute_pixel_window`` evaluates it exactly from the pixel shapes (``hx_pixel_window``,
csrc/hx_pixwin.hip: the phi integral in closed form, a 12-node Gauss-Legendre rule per half pixel in the remaining coordinate), pinned
against an all-pixel two-dimensional quadrature that uses neither the symmetries nor the closed form (tests/test_gpu_pixwin.py).

Parity with healpy is "unpinned", as for the pixel weights (weights.py): the files (``pixel_window_nNNNN.fits``, columns
``TEMPERATURE`` and ``POLARIZATION``) are healpy data, neither in the reference tree nor in this repository.  Two limits are known:

* healpy's polarised column has no stated definition that could be restated here; the spin-2 window computed here is the
  total-power window above, which need not be what that column holds.
* healpy's tables above nside 128 are extrapolations from smaller resolutions and differ slightly from the exact values.

What is implemented for the files -- and tested on synthetic ones -- is the wire format: ``write_pixel_window`` keeps a computed
production-size window on disk, ``read_pixel_window`` / ``find_window_file`` honour a user's healpy data directory.
"""

from __future__ import annotations

import os

import numpy as np

from . import _lib
from . import fits as _fits

NSIDE_MAX = 8192


def window_filename(nside: int) -> str:
    return "pixel_window_n%04d.fits" % int(nside)


def find_window_file(datapath, nside):
    """The window file of ``nside`` under ``datapath`` (healpy keeps it in the data directory itself); a path to the file is
    accepted as well.  None if there is none."""
    if datapath is None:
        return None
    datapath = os.fspath(datapath)
    if os.path.isfile(datapath):
        return datapath if os.path.basename(datapath) == window_filename(nside) else None
    cand = os.path.join(datapath, window_filename(nside))
    return cand if os.path.isfile(cand) else None


def read_pixel_window(path):
    """(pw_T, pw_P) of the first table extension of the file (float64): the columns ``TEMPERATURE`` and ``POLARIZATION``, or the
    first two columns if they carry other names."""
    for h, off in _fits._scan(path):
        if str(h.get("XTENSION", "")).strip() != "BINTABLE":
            continue
        cols = _fits._columns(h)
        if len(cols) < 2:
            raise ValueError(f"{path}: a pixel-window table has two columns, this one has {len(cols)}")
        width = _fits._column_width(h)
        per_row = sum(r for _, r in cols)
        raw = np.fromfile(path, dtype=">f8" if width == 8 else ">f4", count=h["NAXIS2"] * per_row, offset=off)
        raw = raw.astype(np.float64).reshape(h["NAXIS2"], per_row)
        names = [n.upper() for n, _ in cols]
        it = names.index("TEMPERATURE") if "TEMPERATURE" in names else 0
        ip = names.index("POLARIZATION") if "POLARIZATION" in names else 1
        start = np.concatenate([[0], np.cumsum([r for _, r in cols])])
        take = lambda i: np.ascontiguousarray(raw[:, start[i] : start[i + 1]]).ravel()
        return take(it), take(ip)
    raise ValueError(f"{path}: no binary table extension")


def write_pixel_window(path, nside, pw_T, pw_P):
    """A file in the layout of healpy's ``pixel_window_nNNNN.fits``: one binary table of the columns ``TEMPERATURE`` and
    ``POLARIZATION`` (doubles), one row per l."""
    pw_T = np.ascontiguousarray(pw_T, dtype=np.float64)
    pw_P = np.ascontiguousarray(pw_P, dtype=np.float64)
    if pw_T.ndim != 1 or pw_T.shape != pw_P.shape or pw_T.size < 1:
        raise ValueError(f"pw_T and pw_P must be one-dimensional arrays of one length, got {pw_T.shape} and {pw_P.shape}")
    if int(nside) < 1:
        raise ValueError(f"nside = {nside}")
    _fits._new_file(path, True)
    extra = [_fits._card("NSIDE", int(nside), "Resolution parameter of HEALPIX"), _fits._card("MAX-LPOL", int(pw_T.size - 1), "Maximum multipole l")]
    payload = np.stack([pw_T, pw_P], axis=1).astype(">f8").tobytes()
    _fits._append_table(path, "PIXEL WINDOW", ["TEMPERATURE", "POLARIZATION"], 1, pw_T.size, payload, extra, {})


_files: dict = {}
_computed: dict = {}  # compute_pixel_window: (nside, lmax, spin, device, rings) -> array


def load_pixel_window(datapath, nside, lmax):
    """(pw_T, pw_P) up to ``lmax`` from the window file of ``nside`` under ``datapath``, cached per file; None if there is no file."""
    path = find_window_file(datapath, nside)
    if path is None:
        return None
    key = os.path.abspath(path)
    if key not in _files:
        _files[key] = read_pixel_window(path)
    pw0, pw2 = _files[key]
    if pw0.size < lmax + 1:
        raise ValueError(f"{path}: the table ends at l = {pw0.size - 1}, lmax = {lmax} is wanted")
    return pw0[: lmax + 1], pw2[: lmax + 1]


def _key(nside, lmax, spin):
    """Validated (nside, lmax, spins, one spin given)."""
    if int(nside) != nside:
        raise ValueError(f"nside = {nside!r}")
    nside = int(nside)
    if nside < 1 or nside > NSIDE_MAX:
        raise ValueError(f"nside = {nside}: the pixel window is computed for nside 1..{NSIDE_MAX}")
    lmax = 3 * nside - 1 if lmax is None else int(lmax)
    if lmax < 0:
        raise ValueError(f"lmax = {lmax}")
    if lmax > 4 * nside:
        raise ValueError(f"lmax = {lmax}: the pixel window of NSIDE={nside} is computed up to lmax = 4 nside = {4 * nside} (the "
                         f"quadrature rule is validated up to there, and healpy's table ends there)")
    single = not isinstance(spin, (tuple, list))
    spins = (spin,) if single else tuple(spin)
    for s in spins:
        if isinstance(s, bool) or int(s) != s:
            raise ValueError(f"spin = {s!r}")
        if s < 0 or s > lmax:
            raise ValueError(f"spin = {s}: a spin weight in 0..lmax = {lmax}")
    return nside, lmax, tuple(int(s) for s in spins), single


def compute_pixel_window(nside, lmax=None, spin=0, *, device=None, rings=False):
    """The pixel window W_l^(spin), l = 0..lmax, of HEALPix resolution ``nside`` (any integer in 1..8192, not only powers of two),
    computed on the GPU from the pixel shapes (module docstring; ``hx_pixel_window``).  ``lmax`` defaults to ``3 * nside - 1`` and may
    not exceed ``4 * nside``; ``spin`` is a spin weight >= 0, or a tuple of them, which gives a tuple of arrays.

    Returns numpy, or a CUDA tensor if ``device`` is given.  ``rings=True``: the table (2 nside, lmax + 1) of the northern rings' own
    sums ``4 pi / (2l+1) sum_{p in ring} sum_m |A_lm(p)|^2`` instead (``hx_pixel_window_rings``); the window is
    ``sqrt(sum_r c_r row_r / (12 nside^2))`` with c_r = 2, and 1 for the last ring (the equator), added in ring order.

    Results are cached per (nside, lmax, spin, device) until ``release_caches()``."""
    nside, lmax, spins, single = _key(nside, lmax, spin)
    dev = None if device is None else str(device)
    out = []
    for s in spins:
        key = (nside, lmax, s, dev, bool(rings))
        if key not in _computed:
            _lib.ensure_init()
            shape = (2 * nside, lmax + 1) if rings else (lmax + 1,)
            if device is None:
                res = np.empty(shape)
            else:
                import torch

                res = torch.empty(shape, dtype=torch.float64, device=device)
            L = _lib.load()
            if rings:
                _lib.check(L.hx_pixel_window_rings(nside, s, lmax, 1, 2 * nside, _lib.ptr(res)))
            else:
                _lib.check(L.hx_pixel_window(nside, s, lmax, _lib.ptr(res)))
            if device is None:
                res.setflags(write=False)
            _computed[key] = res
        res = _computed[key]
        out.append(res.copy() if isinstance(res, np.ndarray) else res)
    return out[0] if single else tuple(out)


def release_computed():
    """Drop the windows ``compute_pixel_window`` keeps and the tables read from files (``release_caches()`` calls this)."""
    _computed.clear()
    _files.clear()
