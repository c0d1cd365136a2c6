"""Mask tools in HBM: what is done to a mask before it reaches ``mixing_matrices``, ``mask_product_cls`` or ``mock_catalogs``.

``mask_discs`` cuts holes around catalogue positions (bright-star and bad-region masks; on the host a Python loop over
``healpy.query_disc``), ``mask_polygons`` cuts convex spherical polygons -- diffraction spikes, trails, chip gaps -- or builds a
footprint as the union of its tiles (``healpy.query_polygon`` in a loop), ``mask_distance`` is the angle to the
nearest masked pixel, ``apodize_mask`` multiplies the mask by a taper in that angle (NaMaster's ``mask_apodization``, kinds "C1" and "C2").  The rule (``hx_mask_discs``, ``hx_mask_distance``,
``hx_mask_taper``): maps are RING, float64, any integer nside up to 8192; between unit vectors
``h(u, v) = ((u_x - v_x)^2 + (u_y - v_y)^2 + (u_z - v_z)^2) / 2 = 1 - cos(angle)``, for an angle ``h(a) = 2 sin^2(a / 2)``; a pixel is
masked when ``mask <= 0``.  Every result is bit-identical from run to run."""

from __future__ import annotations

import numpy as np

from . import _lib
from .core import DeviceArray

__all__ = ["mask_discs", "mask_polygons", "rectangle_polygons", "mask_distance", "apodize_mask"]

#: the taper kinds and their numbers in ``hx_mask_taper`` (KIND_C1, KIND_C2 of csrc/hx_masktools.h)
KINDS = {"C1": 1, "C2": 2}


def _is_tensor(a):
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


def _nside_of(npix):
    nside = int(round((npix / 12) ** 0.5))
    if nside < 1 or 12 * nside * nside != npix:
        raise ValueError(f"the mask has {npix} pixels, which is not a HEALPix map (12 nside^2)")
    if nside > 8192:
        raise ValueError(f"nside = {nside}, 1 .. 8192 are supported")
    return nside


def _read_map(mask):
    """(float64 contiguous 1-D array or tensor, is-tensor, nside) of a mask that is only read."""
    src = mask.tensor if isinstance(mask, DeviceArray) else mask
    tensor = _is_tensor(src)
    if tensor:
        import torch

        src = src.to(torch.float64).contiguous()
    else:
        src = np.ascontiguousarray(src, dtype=np.float64)
    if src.ndim != 1:
        raise ValueError(f"the mask has shape {tuple(src.shape)}, a 1-D map is needed")
    return src, tensor, _nside_of(int(src.shape[0]))


def _angle(deg, what):
    deg = float(deg)
    if not 0.0 < deg <= 180.0:
        raise ValueError(f"{what} = {deg} degrees, (0, 180] is supported")
    return deg


def _coords(a, name):
    if _is_tensor(a):
        import torch

        a = a.to(torch.float64).contiguous()
    else:
        a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{name} has shape {tuple(a.shape)}, a 1-D array is needed")
    return a


def _work_map(mask, device, fill):
    """(the map the library writes, what the caller gets back, nside) of a mask that is changed: a copy of a numpy mask, a tensor or
    ``DeviceArray`` itself, or for an int nside a new map of ``fill`` (numpy, or a tensor on ``device`` when that is given)."""
    out = mask
    if isinstance(mask, (int, np.integer)):
        nside = int(mask)
        if not 1 <= nside <= 8192:
            raise ValueError(f"nside = {nside}, 1 .. 8192 are supported")
        if device is None:
            work = out = np.full(12 * nside * nside, fill)
        else:
            import torch

            work = out = torch.full((12 * nside * nside,), fill, dtype=torch.float64, device=device)
    else:
        work = mask.tensor if isinstance(mask, DeviceArray) else mask
        if _is_tensor(work):
            import torch

            if work.dtype != torch.float64 or not work.is_contiguous():
                raise ValueError("a tensor mask is changed in place: it must be float64 and contiguous")
        else:
            work = out = np.array(work, dtype=np.float64, order="C")
        if work.ndim != 1:
            raise ValueError(f"the mask has shape {tuple(work.shape)}, a 1-D map is needed")
        nside = _nside_of(int(work.shape[0]))
    return work, out, nside


def mask_discs(mask, lon, lat, radius, *, device=None):
    """Set the pixels of ``mask`` whose centres lie within ``radius`` of a position ``(lon, lat)`` to 0.0 (all angles in degrees):
    pixel p goes iff ``h(v_p, c_k) <= h(radius_k)`` for some disc k -- ``healpy.query_disc(inclusive=False)`` for every disc at once.
    ``radius`` is one number for all discs or an array of one per disc, 0 .. 180.

    A numpy mask gives a new numpy mask; a CUDA tensor (float64, contiguous) or a ``DeviceArray`` is changed in place and returned.
    ``mask`` may be an int nside: the result starts from ones (numpy, or a tensor on ``device`` when that is given).  Coordinates may
    be numpy arrays or CUDA tensors.  The result does not depend on the order of the discs.  ``ValueError``: a mask that is not a
    HEALPix map, coordinate arrays of different lengths, a tensor that cannot be used in place.  ``HxError``, nothing written: a NaN
    or infinite coordinate, ``|lat| > 90``, a radius outside [0, 180] (the message names the first such disc), a NaN or infinite
    mask value (the first such pixel)."""
    work, out, nside = _work_map(mask, device, 1.0)
    lon, lat = _coords(lon, "lon"), _coords(lat, "lat")
    ndisc = int(lon.shape[0])
    if int(lat.shape[0]) != ndisc:
        raise ValueError(f"lon has {ndisc} entries, lat {int(lat.shape[0])}")
    if np.ndim(radius) == 0 and not _is_tensor(radius):
        radii, radius_all = None, float(radius)
    else:
        radii, radius_all = _coords(radius, "radius"), 0.0
        if int(radii.shape[0]) != ndisc:
            raise ValueError(f"lon has {ndisc} entries, radius {int(radii.shape[0])}")
    _mask_discs(nside, work, ndisc, lon, lat, radii, radius_all)
    return out


def mask_polygons(mask, lon, lat, offsets=None, *, value=0.0, device=None):
    """Set the pixels of ``mask`` whose centres lie inside at least one convex spherical polygon to ``value``:
    ``healpy.query_polygon(inclusive=False)`` for every polygon at once.  A polygon is a cyclic list of 3 .. 64
    vertices ``(lon, lat)`` in degrees, in either winding, joined by the minor great-circle arcs between consecutive vertices; it
    must be convex.  ``lon`` and ``lat`` are 2-D ``(npoly, nvert)`` for polygons of equal vertex counts (as ``rectangle_polygons``
    returns them), or 1-D with ``offsets`` (``npoly + 1`` integers, polygon k owning the vertices ``offsets[k] : offsets[k + 1]``);
    numpy arrays or CUDA tensors.  ``value = 0.0`` cuts holes; a map of zeros with ``value = 1.0`` builds a footprint as the union of
    its tiles.

    ``mask`` as for ``mask_discs``: a numpy mask gives a new numpy mask; a CUDA tensor (float64, contiguous) or a ``DeviceArray`` is
    changed in place and returned; an int nside starts from ones when ``value == 0`` and from zeros otherwise (numpy, or a tensor on
    ``device``).  The result does not depend on the order of the polygons and is bit-identical from run to run.  ``ValueError``: a
    mask that is not a HEALPix map, ``lon`` and ``lat`` of different shapes, 1-D vertices without ``offsets`` or ``offsets`` that do
    not end at their length.  ``HxError``, nothing written: a NaN or infinite coordinate, ``|lat| > 90``, a vertex count outside
    3 .. 64, offsets that do not start at 0 or decrease, a polygon that is not convex (the message names the first such polygon), a
    NaN or infinite ``value`` or mask value."""
    value = float(value)
    work, out, nside = _work_map(mask, device, 1.0 if value == 0.0 else 0.0)
    lon, lat = _vertices(lon, "lon"), _vertices(lat, "lat")
    if tuple(lon.shape) != tuple(lat.shape):
        raise ValueError(f"lon has shape {tuple(lon.shape)}, lat {tuple(lat.shape)}")
    if lon.ndim == 2:
        if offsets is not None:
            raise ValueError("offsets go with 1-D vertex arrays; 2-D arrays hold one polygon per row")
        npoly, nvert = int(lon.shape[0]), int(lon.shape[1])
        offsets = np.arange(npoly + 1, dtype=np.int64) * nvert
        lon, lat = lon.reshape(-1), lat.reshape(-1)
    elif offsets is None:
        raise ValueError("1-D vertex arrays need offsets")
    else:
        if _is_tensor(offsets):
            import torch

            offsets = offsets.to(torch.int64).contiguous()
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or int(offsets.shape[0]) < 1:
            raise ValueError(f"offsets has shape {tuple(offsets.shape)}, npoly + 1 entries are needed")
        npoly = int(offsets.shape[0]) - 1
        if int(offsets[-1]) != int(lon.shape[0]):
            raise ValueError(f"offsets end at {int(offsets[-1])}, lon has {int(lon.shape[0])} entries")
    _mask_polygons(nside, work, npoly, offsets, lon, lat, value)
    return out


def _vertices(a, name):
    if _is_tensor(a):
        import torch

        a = a.to(torch.float64).contiguous()
    else:
        a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim not in (1, 2):
        raise ValueError(f"{name} has shape {tuple(a.shape)}, a 1-D or 2-D array is needed")
    return a


def rectangle_polygons(lon, lat, length, width, angle):
    """The gnomonic rectangles of ``length`` by ``width`` around the centres ``(lon, lat)``, turned by ``angle`` (all in degrees; each
    a number or an array of n): ``(lon, lat)`` of shape ``(n, 4)`` for ``mask_polygons``.  With c the centre,
    ``e = (-sin lon, cos lon, 0)`` (east), ``n = (-sin lat cos lon, -sin lat sin lon, cos lat)`` (north),
    ``a = cos(angle) n + sin(angle) e`` and ``b = -sin(angle) n + cos(angle) e``, the corners are
    ``normalise(c +- tan(length / 2) a +- tan(width / 2) b)`` in the order (+, +), (+, -), (-, -), (-, +): the long axis points north
    at angle 0 and turns towards east.  The edges are great circles; through the centre the rectangle is exactly ``length`` by
    ``width``, and it is convex for both in (0, 180).  Computed in float64 with numpy, or with torch on the device of the first
    tensor among the arguments; longitudes come back in [0, 360).  ``ValueError``: a length or width outside (0, 180)."""
    args = (lon, lat, length, width, angle)
    tensors = [a for a in args if _is_tensor(a)]
    if tensors:
        import torch as xp

        args = xp.broadcast_tensors(*[xp.atleast_1d(a.to(xp.float64) if _is_tensor(a) else xp.as_tensor(np.asarray(a, dtype=np.float64))).to(tensors[0].device)
                                      for a in args])
    else:
        xp = np
        args = np.broadcast_arrays(*[np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in args])
    lon, lat, length, width, angle = args
    if lon.ndim != 1:
        raise ValueError(f"the centres have shape {tuple(lon.shape)}, numbers or 1-D arrays are needed")
    for name, a in (("length", length), ("width", width)):
        if not bool(((a > 0.0) & (a < 180.0)).all()):
            raise ValueError(f"{name} outside (0, 180) degrees")
    rad, deg = np.pi / 180.0, 180.0 / np.pi
    lo, la, an = lon * rad, lat * rad, angle * rad
    tl, tw = xp.tan(0.5 * (length * rad)), xp.tan(0.5 * (width * rad))
    sl, cl, sb, cb, sa, ca = xp.sin(lo), xp.cos(lo), xp.sin(la), xp.cos(la), xp.sin(an), xp.cos(an)
    c = (cb * cl, cb * sl, sb)
    e = (-sl, cl, 0.0 * sl)
    n = (-sb * cl, -sb * sl, cb)
    a = [ca * n[i] + sa * e[i] for i in range(3)]
    b = [ca * e[i] - sa * n[i] for i in range(3)]
    atan2 = xp.atan2 if tensors else np.arctan2
    lons, lats = [], []  # (the angles of c +- .. a +- .. b are those of its normalisation)
    for sgn_a, sgn_b in ((1.0, 1.0), (1.0, -1.0), (-1.0, -1.0), (-1.0, 1.0)):
        x, y, z = [(c[i] + sgn_a * (tl * a[i])) + sgn_b * (tw * b[i]) for i in range(3)]
        phi = atan2(y, x) * deg
        phi = xp.where(phi < 0.0, phi + 360.0, phi)
        lons.append(xp.where(phi >= 360.0, phi - 360.0, phi))
        lats.append(atan2(z, xp.sqrt(x * x + y * y)) * deg)
    return xp.stack(lons, -1), xp.stack(lats, -1)


def mask_distance(mask, max_distance):
    """The angle in degrees from every pixel centre to the nearest masked pixel centre (``mask <= 0``), capped at ``max_distance``
    (degrees, in (0, 180]); 0 on masked pixels, the cap everywhere when nothing is masked.  The same kind of array as ``mask``
    (numpy, or a CUDA tensor on its device)."""
    deg = _angle(max_distance, "max_distance")
    src, tensor, nside = _read_map(mask)
    if tensor:
        import torch

        H = torch.empty_like(src)
        _mask_distance(nside, src, deg, H)
        return torch.rad2deg(2.0 * torch.asin(torch.sqrt(H * 0.5).clamp_(max=1.0)))
    H = np.empty_like(src)
    _mask_distance(nside, src, deg, H)
    return np.degrees(2.0 * np.arcsin(np.minimum(np.sqrt(H * 0.5), 1.0)))


def apodize_mask(mask, aposize, kind="C1"):
    """``mask`` times a taper in the distance to the nearest masked pixel: with H the chord measure of that distance capped at
    ``h(aposize)`` and ``x = sqrt(H / h(aposize))``, "C1" is ``x - sin(2 pi x) / (2 pi)`` and "C2" ``(1 - cos(pi x)) / 2`` --
    NaMaster's ``mask_apodization`` of those names.  Masked pixels come back as 0.0; a non-binary mask keeps its values away from the
    edges.  ``aposize`` in degrees, in (0, 180].  A new array of the kind of ``mask`` (numpy, or a CUDA tensor on its device).
    ``ValueError``: any other ``kind`` (NaMaster's "Smooth" needs a transform and is not offered), ``aposize`` out of range."""
    if kind not in KINDS:
        raise ValueError(f"kind = {kind!r}, 'C1' and 'C2' are supported")
    deg = _angle(aposize, "aposize")
    src, tensor, nside = _read_map(mask)
    if tensor:
        import torch

        out = torch.empty_like(src)
    else:
        out = np.empty_like(src)
    _mask_taper(nside, src, deg, KINDS[kind], out)
    return out


def _mask_discs(nside, mask, ndisc, lon, lat, radius, radius_all):
    """``hx_mask_discs`` on arrays of either kind."""
    _lib.ensure_init()
    _lib.check(_lib.load().hx_mask_discs(nside, _lib.ptr(mask), ndisc, _lib.ptr(lon), _lib.ptr(lat), _lib.ptr(radius), radius_all))


def _mask_polygons(nside, mask, npoly, offsets, lon, lat, value):
    """``hx_mask_polygons`` on arrays of either kind."""
    _lib.ensure_init()
    _lib.check(_lib.load().hx_mask_polygons(nside, _lib.ptr(mask), npoly, _lib.ptr(offsets), _lib.ptr(lon), _lib.ptr(lat), value))


def _mask_distance(nside, mask, max_distance, H):
    """``hx_mask_distance`` on arrays of either kind."""
    _lib.ensure_init()
    _lib.check(_lib.load().hx_mask_distance(nside, _lib.ptr(mask), max_distance, _lib.ptr(H)))


def _mask_taper(nside, mask, aposize, kind, out):
    """``hx_mask_taper`` on arrays of either kind."""
    _lib.ensure_init()
    _lib.check(_lib.load().hx_mask_taper(nside, _lib.ptr(mask), aposize, kind, _lib.ptr(out)))
