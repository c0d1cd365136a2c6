"""Mapper that holds alms directly: the ``heracles.ducc.DiscreteMapper`` surface
(heracles/ducc.py:40-162) in front of the same two-point backend.

``create`` / ``transform`` / ``resample`` / ``area`` are reproduced;
``resample`` re-packs on the GPU through ``hx_alm_resample``.  ``map_values`` -- ducc0's
non-uniform adjoint synthesis (heracles/ducc.py:92-133) -- runs through
``hx_pointsht_adjoint``: a type-1 non-uniform FFT on the (theta, phi) torus and the Legendre
analysis kernel of the HEALPix path on equidistant rings (csrc/hx_nufft.hip).  ``sample`` is the
way back, alms to values at points (ducc0's ``synthesis_general``), through
``hx_pointsht_synthesis``; ``PointSHT.field`` keeps a field resident for page after page.
"""

from __future__ import annotations

import numpy as np

from . import _lib
from .core import update_metadata


def alm_resample(data, lmax_out, dtype=np.complex128):
    """Change the band limit of m-major alms (..., nlm_in) -> (..., nlm_out): truncate or zero-pad."""
    _lib.ensure_init()
    n = data.shape[-1]
    lmax_in = (int((8 * n + 1) ** 0.5 + 0.01) - 3) // 2
    if (lmax_in + 1) * (lmax_in + 2) // 2 != n:
        raise ValueError(f"{n} is not a triangular alm size")
    n_out = (lmax_out + 1) * (lmax_out + 2) // 2
    ncomp = 1
    for d in data.shape[:-1]:
        ncomp *= d
    if hasattr(data, "data_ptr"):
        import torch

        src = data.to(torch.complex128).contiguous()
        out = torch.empty((*data.shape[:-1], n_out), dtype=torch.complex128, device=data.device)
    else:
        src = np.ascontiguousarray(data, dtype=np.complex128)
        out = np.empty((*data.shape[:-1], n_out), dtype=np.complex128)
    _lib.check(_lib.load().hx_alm_resample(lmax_in, int(lmax_out), ncomp, _lib.ptr(src), _lib.ptr(out)))
    if not hasattr(out, "data_ptr") and np.dtype(dtype) != np.complex128:
        out = out.astype(dtype)
    return out


class PointSHT:
    """``alm = sum_p values_p conj(sY_lm(theta_p, phi_p))`` for points anywhere on the sphere: the object behind
    ``hx_pointsht_*`` (one per band limit and accuracy; it owns the oversampled grid and the ring plan)."""

    def __init__(self, lmax, epsilon=1e-12):
        _lib.ensure_init()
        self.lmax, self.epsilon = int(lmax), float(epsilon)
        self._h = _lib.load().hx_pointsht_create(self.lmax, self.epsilon)
        if not self._h:
            raise _lib.HxError(-1, _lib.load().hx_last_error().decode(errors="replace"))
        import ctypes

        info = (ctypes.c_int * 4)()
        _lib.check(_lib.load().hx_pointsht_info(self._h, info))
        _, self.nrings_circle, self.ngrid, self.kernel_width = list(info)
        self.nlm = (self.lmax + 1) * (self.lmax + 2) // 2

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().hx_pointsht_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def adjoint_synthesis(self, loc, values, spin=0, out=None):
        """values (ncomp, npoints) float64 at loc (npoints, 2) = (colatitude, longitude) [rad] -> alm (ncomp, nlm)
        complex128; numpy in -> numpy out, torch device tensors in -> device tensor out.  ``spin`` is any weight s >= 0:
        0 transforms every row on its own, s >= 1 reads the rows in pairs (Q, U) and returns (E, B) per pair (zero for l < s);
        a negative ``spin`` or an odd number of rows with s >= 1 is a ``ValueError``."""
        dev = hasattr(values, "data_ptr")
        if dev:
            import torch

            values = values.to(torch.float64).contiguous()
            loc = loc.to(torch.float64).contiguous()
            if out is None:
                out = torch.empty((values.shape[0], self.nlm), dtype=torch.complex128, device=values.device)
        else:
            values = np.ascontiguousarray(values, dtype=np.float64)
            loc = np.ascontiguousarray(loc, dtype=np.float64)
            if out is None:
                out = np.empty((values.shape[0], self.nlm), dtype=np.complex128)
        if values.ndim != 2 or tuple(loc.shape) != (values.shape[1], 2):
            raise ValueError("values must be (ncomp, npoints) and loc (npoints, 2)")
        try:
            _lib.check(_lib.load().hx_pointsht_adjoint(self._h, int(spin), int(values.shape[0]), int(values.shape[1]),
                                                       _lib.ptr(loc), _lib.ptr(values), _lib.ptr(out)))
        except _lib.HxError as e:
            if e.code == _lib.HX_ERR_ARG:
                raise ValueError(str(e)) from None
            raise
        return out

    def _alm_arg(self, alm, spin):
        """alm as a contiguous (ncomp, nlm) complex128 array or device tensor; ValueError for what the library would refuse."""
        dev = hasattr(alm, "data_ptr")
        if dev:
            import torch

            alm = alm.to(torch.complex128).contiguous()
        else:
            alm = np.ascontiguousarray(alm, dtype=np.complex128)
        if alm.ndim != 2 or alm.shape[1] != self.nlm:
            raise ValueError(f"alm must be (ncomp, {self.nlm}) for lmax {self.lmax}")
        if int(spin) < 0 or alm.shape[0] < 1 or (int(spin) > 0 and alm.shape[0] % 2):
            raise ValueError(f"{alm.shape[0]} components of spin {spin}")
        return alm, dev

    @staticmethod
    def _loc_arg(loc, dev, like):
        if dev:
            import torch

            loc = torch.as_tensor(loc, device=like.device).to(torch.float64).contiguous()
        else:
            loc = np.ascontiguousarray(loc, dtype=np.float64)
        if loc.ndim != 2 or loc.shape[1] != 2:
            raise ValueError("loc must be (npoints, 2)")
        return loc

    @staticmethod
    def _values_out(shape, dev, like, out):
        if out is not None:
            return _lib.result_array(shape, out)
        if dev:
            import torch

            return torch.empty(shape, dtype=torch.float64, device=like.device)
        return np.empty(shape, dtype=np.float64)

    def synthesis(self, loc, alm, spin=0, out=None):
        """The forward direction (ducc0's ``synthesis_general``): alm (ncomp, nlm) complex128 -> the field's values (ncomp, npoints)
        float64 at loc (npoints, 2) = (colatitude, longitude) [rad]; numpy in -> numpy out, torch device tensors in -> device tensor
        out, ``out=`` is written in place and returned.  ``spin`` as for :meth:`adjoint_synthesis`: s >= 1 reads the rows in pairs
        (E, B) and returns (Q, U) per pair (zero for s > lmax); a negative ``spin``, an odd number of rows with s >= 1 or a point
        outside the sphere is a ``ValueError``.  Bit-identical from call to call."""
        alm, dev = self._alm_arg(alm, spin)
        loc = self._loc_arg(loc, dev, alm)
        out = self._values_out((alm.shape[0], loc.shape[0]), dev, alm, out)
        try:
            _lib.check(_lib.load().hx_pointsht_synthesis(self._h, int(spin), int(alm.shape[0]), int(loc.shape[0]),
                                                         _lib.ptr(loc), _lib.ptr(alm), _lib.ptr(out)))
        except _lib.HxError as e:
            if e.code == _lib.HX_ERR_ARG:
                raise ValueError(str(e)) from None
            raise
        return out

    def field(self, alm, spin=0):
        """The field with coefficients alm, resident on the device, to be read at any number of point sets: the part of
        :meth:`synthesis` that does not depend on the points is done once here (``ncomp`` grids of ``ngrid``^2 float64)."""
        return PointField(self, alm, spin)


class PointField:
    """What ``PointSHT.field`` returns (``hx_pointgrid``): ``at(loc)`` equals ``PointSHT.synthesis(loc, alm, spin)`` bit for bit, page
    after page, at the cost of the gather alone.  It keeps its ``PointSHT`` alive."""

    def __init__(self, sht, alm, spin=0):
        self._h = None
        alm, _ = sht._alm_arg(alm, spin)
        self._sht, self.spin, self.ncomp = sht, int(spin), int(alm.shape[0])
        self._h = _lib.load().hx_pointsht_grids(sht._h, self.spin, self.ncomp, _lib.ptr(alm))
        if not self._h:
            raise _lib.HxError(-1, _lib.load().hx_last_error().decode(errors="replace"))

    def at(self, loc, out=None):
        """Values (ncomp, npoints) float64 at loc (npoints, 2); a numpy array unless loc or ``out`` is a device tensor."""
        if not self._h:
            raise ValueError("the field has been closed")
        dev = hasattr(loc, "data_ptr") and getattr(loc, "is_cuda", False) or (out is not None and getattr(out, "is_cuda", False))
        like = loc if hasattr(loc, "data_ptr") and getattr(loc, "is_cuda", False) else out
        loc = PointSHT._loc_arg(loc, dev, like)
        out = PointSHT._values_out((self.ncomp, loc.shape[0]), dev, like, out)
        try:
            _lib.check(_lib.load().hx_pointgrid_gather(self._h, int(loc.shape[0]), _lib.ptr(loc), _lib.ptr(out)))
        except _lib.HxError as e:
            if e.code == _lib.HX_ERR_ARG:
                raise ValueError(str(e)) from None
            raise
        return out

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().hx_pointgrid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_point_plans = {}


def get_point_sht(lmax, epsilon=1e-12):
    key = (int(lmax), float(epsilon))
    if key not in _point_plans:
        _point_plans[key] = PointSHT(*key)
    return _point_plans[key]


class HipDiscreteMapper:
    """Mapper that creates alms directly (heracles/ducc.py:40-162)."""

    def __init__(self, lmax, *, dtype=np.complex128, nthreads=0):
        self.__lmax = lmax
        self.__dtype = np.dtype(dtype)
        self.__nthreads = nthreads  # accepted for signature compatibility; unused

    @property
    def lmax(self):
        return self.__lmax

    @property
    def area(self):
        """The effective area for this mapper (heracles/ducc.py:66-71)."""
        return 1.0

    def create(self, *dims, spin=0):
        lmax = self.__lmax
        m = np.zeros((*dims, (lmax + 1) * (lmax + 2) // 2), dtype=self.__dtype)
        update_metadata(m, geometry="discrete", kernel="none", lmax=lmax, spin=spin)
        return m

    def map_values(self, lon, lat, data, values, spin=0):
        """Add values to alms (heracles/ducc.py:92-133): ``data += sum_p values_p conj(sY_lm(lon_p, lat_p))``.
        float32 values are transformed to 1e-5, everything else in float64 to 1e-12, as the reference asks of ducc0.
        ``spin`` is any weight s >= 0, as for ducc0: rows in pairs (Q, U) -> (E, B) for s >= 1."""
        values = np.asarray(values)
        flatten = values.ndim == 1
        if flatten:
            values = values.reshape(1, -1)
        epsilon = 1e-5 if values.dtype == np.float32 else 1e-12
        lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
        loc = np.empty((lon.size, 2), dtype=np.float64)
        loc[:, 0] = np.radians(90.0 - lat)
        loc[:, 1] = np.radians(lon % 360.0)
        alms = get_point_sht(self.__lmax, epsilon).adjoint_synthesis(loc, values, spin=spin)
        if flatten:
            alms = alms[0]
        data += alms

    def sample(self, lon, lat, data, spin=0):
        """The inverse direction of :meth:`map_values`: the values at (lon, lat) [degrees] of the field whose alms are ``data``
        ((ncomp, nlm), or (nlm,) for one row of values), through ``PointSHT.synthesis``.  complex64 alms are evaluated to 1e-5,
        everything else in float64 to 1e-12; alms of another band limit than the mapper's are a ``ValueError``."""
        data = np.asarray(data)
        flatten = data.ndim == 1
        if flatten:
            data = data.reshape(1, -1)
        lmax = self.__lmax
        if data.ndim != 2 or data.shape[1] != (lmax + 1) * (lmax + 2) // 2:
            raise ValueError(f"alms of shape {data.shape} do not have the mapper's band limit {lmax}")
        epsilon = 1e-5 if data.dtype == np.complex64 else 1e-12
        lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
        loc = np.empty((lon.size, 2), dtype=np.float64)
        loc[:, 0] = np.radians(90.0 - lat)
        loc[:, 1] = np.radians(lon % 360.0)
        values = get_point_sht(lmax, epsilon).synthesis(loc, data, spin=spin)
        return values[0] if flatten else values

    def transform(self, data, spin=0):
        """Does nothing, since inputs are alms already (heracles/ducc.py:135-143)."""
        return data

    def resample(self, data):
        """Change LMAX of alm (heracles/ducc.py:145-162)."""
        return alm_resample(data, self.__lmax, dtype=self.__dtype)
