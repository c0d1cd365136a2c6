"""Jackknife regions made in HBM: the ``jk_map`` every jackknife entry point takes, from a visibility (or any weight) map.

The reference has no counterpart: its tutorial gets the region map from a third-party host package
(``skysegmentor.segmentmapN(vis_map, Njk)``).  ``jackknife_regions`` cuts the footprint -- the pixels of positive weight -- into
``njk`` compact regions of equal summed weight by recursive weighted bisection along the principal axis (``hx_jk_regions``, DESIGN.md
4.17): deterministic, bit-identical from run to run, a function of the map and ``njk`` alone."""

from __future__ import annotations

import numpy as np

from . import _lib
from .core import DeviceArray

__all__ = ["jackknife_regions"]

#: the largest number of regions (NJK_MAX of csrc/hx_jkregions.h), restated for tests and tools
NJK_MAX = 4096


def _is_tensor(a):
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


def jackknife_regions(vis_map, njk, *, return_info=False, device="cuda"):
    """Region labels of the HEALPix map ``vis_map`` (RING, any integer nside up to 8192, taken from its length): an ``int32`` map
    that is 0 where ``vis_map <= 0`` and 1 .. ``njk`` inside the footprint, the regions having equal summed weight to within a few
    pixel weights per level of the bisection.

    The rule: the footprint is one segment with the labels 1 .. njk.  A segment with n >= 2 labels is split in two along the
    principal axis of its weighted pixel-centre covariance -- the pixels ordered by their projection on the axis, ties by pixel
    index -- where the running weight crosses the fraction (n // 2) / n, and its labels go n // 2 to the left part, the rest to the
    right; no part is left with fewer pixels than labels.  Weights are quantised to 2^-32 of the largest, so every weight sum is an
    exact integer.  All segments of a level are split together: ceil(log2 njk) levels.

    Where the two largest eigenvalues of a segment's covariance are (nearly) equal -- the full sky, a round cap -- the axis is
    whatever the eigen-solver returns: the result is still a valid equal-weight partition and still repeatable, but it is not
    pinned against any other implementation of the rule.

    A numpy map gives a numpy map; a CUDA tensor or ``DeviceArray`` is used in place and gives a CUDA ``int32`` tensor on its
    device (``device`` is accepted for symmetry with ``region_alms``: a numpy map is worked on by the library's device and comes back
    as numpy).  ``return_info=True`` returns ``(labels, {"weights": (njk,) summed weight
    per region, "axes": (njk - 1, 3)})``; ``axes[b - 2]`` is the axis of the split whose right part starts at label ``b``.
    ``ValueError``: a map whose length is not 12 nside^2, ``njk`` outside 1 .. 4096.  ``HxError``: a NaN, negative or infinite
    weight (the message names the first such pixel), fewer footprint pixels than ``njk``."""
    njk = int(njk)
    if not 1 <= njk <= NJK_MAX:
        raise ValueError(f"njk = {njk}, 1 .. {NJK_MAX} are supported")
    src = vis_map.tensor if isinstance(vis_map, DeviceArray) else vis_map
    tensor = _is_tensor(src)
    if tensor:
        import torch

        src = src.to(torch.float64).contiguous()
    else:
        src = np.ascontiguousarray(src, dtype=np.float64)
    if src.ndim != 1:
        raise ValueError(f"vis_map has shape {tuple(src.shape)}, a 1-D map is needed")
    npix = int(src.shape[0])
    nside = int(round((npix / 12) ** 0.5))
    if nside < 1 or 12 * nside * nside != npix:
        raise ValueError(f"vis_map has {npix} pixels, which is not a HEALPix map (12 nside^2)")
    if nside > 8192:
        raise ValueError(f"nside = {nside}, 1 .. 8192 are supported")
    if tensor:
        labels = torch.empty(npix, dtype=torch.int32, device=src.device)
        weights = torch.empty(njk, dtype=torch.float64, device=src.device) if return_info else None
    else:
        labels = np.empty(npix, dtype=np.int32)
        weights = np.empty(njk, dtype=np.float64) if return_info else None
    axes = np.zeros((njk - 1, 3), dtype=np.float64) if return_info else None
    _jk_regions(nside, src, njk, labels, weights, axes)
    if return_info:
        return labels, {"weights": weights, "axes": axes}
    return labels


def _jk_regions(nside, weight, njk, labels, weights, axes):
    """``hx_jk_regions`` on arrays of either kind."""
    _lib.ensure_init()
    _lib.check(_lib.load().hx_jk_regions(nside, _lib.ptr(weight), njk, _lib.ptr(labels), _lib.ptr(weights), _lib.ptr(axes)))
