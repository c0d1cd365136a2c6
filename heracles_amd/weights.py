"""healpy's pixel-weight files for ``HipHealpixMapper`` (``hp.map2alm(..., use_pixel_weights=True, datapath=DATAPATH)``,
heracles/healpy.py:183-189; ``datapath`` from the configuration, heracles/cli.py:536-538).

The files (``healpix_full_weights_nside_NNNN.fits``, one per resolution) are healpy data: they are not part of the reference
tree nor of this repository, so parity with healpy's own values is "unpinned".  What is implemented -- and tested against a
numpy restatement on synthetic files -- is the wire format (one FITS table column of (nside + 1)(3 nside + 1) / 4 doubles)
and the expansion of that compressed half-quadrant to the full-sky array of multiplicative weights, which runs on the GPU
(``hx_pixel_weights_expand``) and stays in HBM for every later transform.

The values need no file: ``compute_pixel_weights`` solves for them on the GPU (``hx_pixel_weights_solve``: the minimum-norm
weights that integrate every harmonic up to twice the transform's band limit exactly).  That is pinned from first principles --
with them ``map2alm(alm2map(a), niter=0) == a`` to rounding for ``lmax <= 3 * nside // 2`` -- and against a dense least-squares
solve on the CPU oracle (tests/test_gpu_compute_weights.py).
"""

from __future__ import annotations

import os

import numpy as np

from . import _lib
from . import fits as _fits


def weights_filename(nside: int) -> str:
    return "healpix_full_weights_nside_%04d.fits" % int(nside)


def find_weights_file(datapath, nside):
    """The file for ``nside`` under ``datapath``: healpy keeps it in ``<datapath>/full_weights/``; the directory itself and a
    path to the file are accepted as well.  None if there is none."""
    if datapath is None:
        return None
    datapath = os.fspath(datapath)
    if os.path.isfile(datapath):
        return datapath
    for cand in (os.path.join(datapath, "full_weights", weights_filename(nside)), os.path.join(datapath, weights_filename(nside))):
        if os.path.isfile(cand):
            return cand
    return None


def compressed_size(nside: int) -> int:
    return ((nside + 1) * (3 * nside + 1)) // 4


def read_compressed_weights(path):
    """All values of the first table extension of the file, in file order (float64)."""
    for h, off in _fits._scan(path):
        if str(h.get("XTENSION", "")).strip() != "BINTABLE":
            continue
        cols = _fits._columns(h)
        width = _fits._column_width(h)
        count = h["NAXIS2"] * sum(r for _, r in cols)
        if len(cols) != 1:
            raise NotImplementedError("pixel-weight file with more than one column")
        return np.fromfile(path, dtype=">f8" if width == 8 else ">f4", count=count, offset=off).astype(np.float64)
    raise ValueError(f"{path}: no binary table extension")


def write_compressed_weights(path, nside, compressed):
    """A file in the layout healpy ships (one column of doubles) -- used by the tests, to keep what
    ``compute_pixel_weights(..., compressed=True)`` returns, and to convert weights computed elsewhere."""
    compressed = np.ascontiguousarray(compressed, dtype=np.float64)
    if compressed.shape != (compressed_size(nside),):
        raise ValueError(f"NSIDE={nside} needs {compressed_size(nside)} compressed weights, got {compressed.shape}")
    _fits._new_file(path, True)
    extra = [_fits._card("NSIDE", int(nside), "Resolution parameter of HEALPIX")]
    _fits._append_table(path, "FULL WEIGHTS", ["COMPRESSED PIXEL WEIGHTS"], 1, compressed.size, compressed.astype(">f8").tobytes(), extra, {})


def expand_pixel_weights(nside, compressed, device=None):
    """Full-sky multiplicative weights ``1 + w`` (12 nside^2) from the compressed values; numpy out, or a CUDA tensor if
    ``device`` is given."""
    _lib.ensure_init()
    compressed = np.ascontiguousarray(compressed, dtype=np.float64)
    npix = 12 * int(nside) ** 2
    if device is None:
        out = np.empty(npix)
    else:
        import torch

        out = torch.empty(npix, dtype=torch.float64, device=device)
    _lib.check(_lib.load().hx_pixel_weights_expand(int(nside), compressed.size, _lib.ptr(compressed), _lib.ptr(out)))
    return out


_cache: dict = {}
_computed: dict = {}  # compute_pixel_weights: (nside, lmax, epsilon, itmax, device) -> (compressed, full-sky, info)


#: Iterations ``compute_pixel_weights`` allows by default.  A relative gradient of 1e-6 takes about 200 iterations and 1e-9 about
#: 2100 at every nside from 256 to 4096, but 1e-12 takes 406 at nside 64, 3152 at 128, 9856 at 256 and more than 30000 at 1024
#:: 4000 reaches the default ``epsilon`` up to nside 128 and leaves a constraint residual at the level of the
#: transform's own rounding beyond (3e-14 after 2209 iterations at nside 4096, 108 ms each).
DEFAULT_ITMAX = 4000


def _solve_key(nside, lmax, epsilon, itmax, device):
    """Validated arguments of ``compute_pixel_weights`` as its cache key."""
    nside = int(nside)
    if nside < 1:
        raise ValueError(f"nside = {nside}")
    lmax = 3 * nside // 2 if lmax is None else int(lmax)
    if lmax < 0:
        raise ValueError(f"lmax = {lmax}")
    if lmax > 3 * nside // 2:
        raise ValueError(f"lmax = {lmax}: pixel weights of NSIDE={nside} exist for a band limit up to 3 nside / 2 = {3 * nside // 2} only. "
                         f"They must integrate every harmonic up to 2 lmax exactly; beyond 3 nside the pixelisation cannot, and the "
                         f"least-squares weights make the quadrature worse than unit weights do.")
    epsilon = float(epsilon)
    if not epsilon >= 0.0:
        raise ValueError(f"epsilon = {epsilon}")
    itmax = DEFAULT_ITMAX if itmax is None else int(itmax)
    if itmax < 0:
        raise ValueError(f"itmax = {itmax}")
    return (nside, lmax, epsilon, itmax, None if device is None else str(device))


def compute_pixel_weights(nside, lmax=None, *, epsilon=1e-12, itmax=None, device=None, compressed=False, info=False):
    """The pixel quadrature weights of ``nside`` for transforms of band limit ``lmax`` (default and largest: ``3 * nside // 2``),
    computed on the GPU (``hx_pixel_weights_solve``): the minimum-norm weights with the symmetries of the pixelisation that
    integrate every harmonic up to ``2 * lmax`` exactly, i.e. with which ``map2alm(alm2map(a), niter=0) == a`` to rounding -- what
    healpy ships as ``healpix_full_weights_nside_NNNN.fits``.

    Returns the full-sky multiplicative weights (numpy, or a CUDA tensor if ``device`` is given), ready for
    ``Plan.map2alm(pix_weights=...)``; ``compressed=True``: the compressed values instead (numpy), ready for
    ``write_compressed_weights``.  ``info=True``: also a dict of ``iterations``, ``rel_gradient`` and ``max_residual`` (the largest
    violation of a constraint by the weights returned).  The conjugate-gradient iteration stops at a relative gradient ``epsilon``
    or after ``itmax`` iterations (default ``DEFAULT_ITMAX``), whichever comes first; stopping at ``itmax`` is not an error but
    warns, with the residual reached.  From nside 256 on the default ``epsilon`` is out of reach of the default ``itmax``;
    ``epsilon=1e-9`` (about 2100 iterations at any nside) leaves a residual of 6e-12 at nside 256 and 3e-14 at 4096.  Results are
    cached per (nside, lmax, epsilon, itmax, device) until ``release_caches()``."""
    key = _solve_key(nside, lmax, epsilon, itmax, device)
    if key not in _computed:
        import ctypes

        from .sht import Plan

        nside, lmax, epsilon, itmax, _ = key
        _lib.ensure_init()
        x = np.empty(compressed_size(nside))
        it, rel, res = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        plan = Plan(nside, 2 * lmax)  # (used once: its tables and scratch go back when the solve is done)
        try:
            _lib.check(_lib.load().hx_pixel_weights_solve(plan._h, lmax, epsilon, itmax, _lib.ptr(x), ctypes.byref(it), ctypes.byref(rel),
                                                         ctypes.byref(res)))
        finally:
            plan.close()
        stats = {"iterations": it.value, "rel_gradient": rel.value, "max_residual": res.value}
        x.setflags(write=False)
        _computed[key] = (x, expand_pixel_weights(nside, x, device=device), stats)
    x, full, stats = _computed[key]
    if stats["rel_gradient"] > key[2]:
        import warnings

        warnings.warn(f"compute_pixel_weights(nside={key[0]}, lmax={key[1]}): epsilon = {key[2]:g} was not reached in {stats['iterations']} "
                      f"iterations (relative gradient {stats['rel_gradient']:.3g}, largest constraint residual {stats['max_residual']:.3g})",
                      RuntimeWarning, stacklevel=2)
    out = x.copy() if compressed else (full.copy() if isinstance(full, np.ndarray) else full)
    return (out, dict(stats)) if info else out


def release_computed():
    """Drop the weights ``compute_pixel_weights`` keeps (``release_caches()`` calls this)."""
    _computed.clear()


def load_pixel_weights(datapath, nside, device="cuda"):
    """Full-sky weights of ``nside`` from ``datapath`` as a device tensor, cached per (file, device); None if there is no file."""
    path = find_weights_file(datapath, nside)
    if path is None:
        return None
    key = (os.path.abspath(path), int(nside), str(device))
    if key not in _cache:
        _cache[key] = expand_pixel_weights(nside, read_compressed_weights(path), device=device)
    return _cache[key]
