"""Rotation of alms by any Euler angles in HBM (``hx_rotate_alm``): brings alms that come in another coordinate
system -- galactic lensing potentials, ecliptic masks -- into the frame of the catalogues without leaving the GPU.

Convention: ``R = Rz(phi) Ry(theta) Rz(psi)`` on column vectors, counter-clockwise about the fixed axes (psi about z first, then theta
about y, then phi about z); the rotated field is ``f'(n) = f(R^-1 n)`` and

    a'_lm = sum_m' exp(-i m phi) d^l_mm'(theta) exp(-i m' psi) a_lm',    d^l(theta) = exp(-i theta J_y)  (Condon-Shortley).

E and B of a field of any spin weight rotate like scalars, so every component gets the same matrices and there is no spin argument."""

from __future__ import annotations

import numpy as np

from . import _lib
from .core import DeviceArray, TocDict, update_metadata

__all__ = ["rotate_alm", "rotate_alms", "euler_from_matrix", "matrix_from_euler", "coord_matrix"]

#: the tiling of the rotation kernel (ROT_CB, ROT_MO, ROT_MB, ROT_LB of csrc/hx_rotate.hip), restated for tests and tools: components
#: per block of a work-group, output columns m per work-group (its waves), pairs of input orders (+m', -m') per block (the lanes of
#: a wave), multipoles per LDS tile
TILE_COMP, TILE_COLS, TILE_M, TILE_L = 4, 4, 64, 16

#: equatorial (J2000) -> galactic, x_G = A x_C: the Hipparcos matrix (ESA SP-1200, vol. 1, eq. 1.5.11), orthogonal to ~1e-10 as printed
_A_GALACTIC = (
    (-0.0548755604, -0.8734370902, -0.4838350155),
    (+0.4941094279, -0.4448296300, +0.7469822445),
    (-0.8676661490, -0.1980763734, +0.4559837762),
)
#: obliquity of the ecliptic at J2000 (IAU 1976), arc seconds
_OBLIQUITY_ARCSEC = 84381.448

_from_equatorial = {}


def _is_tensor(a):
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


def matrix_from_euler(psi, theta, phi):
    """``Rz(phi) @ Ry(theta) @ Rz(psi)``, a 3 x 3 array."""
    def rz(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])

    c, s = np.cos(theta), np.sin(theta)
    ry = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    return rz(phi) @ ry @ rz(psi)


def _check_rotation(R):
    R = np.asarray(R, dtype=np.float64)
    if R.shape != (3, 3) or not np.isfinite(R).all():
        raise ValueError("a rotation matrix is a finite 3 x 3 array")
    if np.abs(R.T @ R - np.eye(3)).max() > 1e-10:
        raise ValueError("the matrix is not orthogonal (|R^T R - 1| > 1e-10)")
    if np.linalg.det(R) < 0:
        raise ValueError("the matrix is a reflection (det < 0), not a rotation")
    return R


def euler_from_matrix(R):
    """``(psi, theta, phi)`` with ``matrix_from_euler(psi, theta, phi) == R``: theta in [0, pi], psi and phi in (-pi, pi]; in the
    degenerate cases theta = 0 and theta = pi, where only psi + phi or psi - phi is defined, phi = 0.  ``ValueError`` for a matrix that
    is not orthogonal to 1e-10 or has determinant < 0."""
    R = _check_rotation(R)
    sin_theta = float(np.hypot(R[0, 2], R[1, 2]))
    theta = float(np.arctan2(sin_theta, R[2, 2]))
    if sin_theta < 1e-15:  # theta within rounding of 0 or pi (sin of the double next to pi is 1.2e-16)
        # Rz(psi) or Ry(pi) Rz(psi) = [[-c, s, 0], [s, c, 0], [0, 0, -1]]
        psi = float(np.arctan2(R[1, 0], R[0, 0])) if R[2, 2] > 0 else float(np.arctan2(R[1, 0], R[1, 1]))
        return psi, (0.0 if R[2, 2] > 0 else float(np.pi)), 0.0
    return float(np.arctan2(R[2, 1], -R[2, 0])), theta, float(np.arctan2(R[1, 2], R[0, 2]))


def _equatorial_to(system):
    """x_system = M x_C."""
    if system not in _from_equatorial:
        if system == "C":
            M = np.eye(3)
        elif system == "G":
            u, _, vt = np.linalg.svd(np.array(_A_GALACTIC))  # the nearest orthogonal matrix
            M = u @ vt
        elif system == "E":
            eps = np.deg2rad(_OBLIQUITY_ARCSEC / 3600.0)
            c, s = np.cos(eps), np.sin(eps)
            M = np.array([[1.0, 0.0, 0.0], [0.0, c, s], [0.0, -s, c]])
        else:
            raise ValueError(f"unknown coordinate system {system!r}: 'C' (equatorial J2000), 'G' (galactic) or 'E' (ecliptic)")
        _from_equatorial[system] = M
    return _from_equatorial[system]


def coord_matrix(src, dst):
    """The 3 x 3 matrix that takes the components of a vector in system ``src`` to its components in ``dst``: ``"C"`` equatorial
    (J2000), ``"G"`` galactic (the Hipparcos matrix, re-orthonormalised), ``"E"`` ecliptic (obliquity 84381.448 arc seconds).
    ``rotate_alm(alm, matrix=coord_matrix(src, dst))`` turns the alms of a field given in ``src`` into its alms in ``dst``."""
    return _equatorial_to(dst) @ _equatorial_to(src).T


def _angles(psi, theta, phi, matrix, coord):
    given = (psi, theta, phi) != (0.0, 0.0, 0.0)
    if sum((given, matrix is not None, coord is not None)) > 1:
        raise ValueError("give the rotation once: angles, matrix= or coord=")
    if coord is not None:
        src, dst = coord
        matrix = coord_matrix(src, dst)
    if matrix is not None:
        return euler_from_matrix(matrix)
    psi, theta, phi = float(psi), float(theta), float(phi)
    if not (np.isfinite(psi) and np.isfinite(theta) and np.isfinite(phi)):
        raise ValueError(f"the angles ({psi}, {theta}, {phi}) are not finite")
    return psi, theta, phi


def _rotate(src, lmax, angles, out):
    """``hx_rotate_alm`` on a C-contiguous complex128 (ncomp, nlm) array or tensor; ``out`` of the same shape."""
    _lib.ensure_init()
    _lib.check(_lib.load().hx_rotate_alm(int(lmax), int(src.shape[0]), _lib.ptr(src), _lib.ptr(out), *angles))
    return out


def rotate_alm(alm, psi=0.0, theta=0.0, phi=0.0, *, matrix=None, coord=None, lmax=None, out=None, device=None):
    """The alms of the field rotated by ``R = Rz(phi) Ry(theta) Rz(psi)`` (see the module text), any angles.

    alm: ``(..., nlm)`` complex, the project's m-major layout with mmax = lmax: a numpy array, a CUDA tensor or a ``DeviceArray``.
    Every row is one component and is rotated with the same matrices; the imaginary part of ``a_l0`` is not read.  A numpy array
    gives a numpy array, a tensor a tensor, a ``DeviceArray`` a ``DeviceArray``; device inputs are read where they are and the result
    stays in HBM.  dtype metadata is copied to the result.

    matrix: a 3 x 3 proper rotation instead of the angles (``euler_from_matrix``); coord: ``(src, dst)`` for ``coord_matrix``.  Giving
    the rotation more than once is a ``ValueError``.  lmax: inferred from the size when not given.  out: receives the result (numpy
    array or tensor of the shape of ``alm``, complex128, contiguous); it must not overlap ``alm`` (``HxError``): there is no in-place
    rotation.  device: a numpy input is rotated into a ``DeviceArray`` on that device."""
    angles = _angles(psi, theta, phi, matrix, coord)
    md = dict(getattr(getattr(alm, "dtype", None), "metadata", None) or {})
    dressed = isinstance(alm, DeviceArray)
    data = alm.tensor if dressed else alm
    tensor = _is_tensor(data)
    if tensor:
        import torch

        src = data.to(torch.complex128).contiguous()
    else:
        src = np.ascontiguousarray(data, dtype=np.complex128)
    shape = tuple(src.shape)
    if len(shape) < 1 or shape[-1] < 1:
        raise ValueError(f"alm has shape {shape}, expected (..., nlm)")
    if lmax is None:
        lmax = (int((8 * shape[-1] + 1) ** 0.5 + 0.01) - 3) // 2
    lmax = int(lmax)
    if (lmax + 1) * (lmax + 2) // 2 != shape[-1]:
        raise ValueError(f"alm has {shape[-1]} coefficients per component, lmax = {lmax} has {(lmax + 1) * (lmax + 2) // 2}")
    if 0 in shape:
        raise ValueError(f"alm has shape {shape}: no components")
    if device is not None and not tensor:
        import torch

        src = torch.from_numpy(src).to(device)
        tensor = dressed = True
    if out is None:
        if tensor:
            import torch

            out = torch.empty(shape, dtype=torch.complex128, device=src.device)
        else:
            out = np.empty(shape, dtype=np.complex128)
    else:
        if tuple(out.shape) != shape:
            raise ValueError(f"out has shape {tuple(out.shape)}, the result has {shape}")
        if isinstance(out, np.ndarray):
            if out.dtype != np.complex128 or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError("out must be a writeable C-contiguous complex128 array")
        elif _is_tensor(out):
            import torch

            if out.dtype != torch.complex128 or not out.is_contiguous():
                raise ValueError("out must be a contiguous complex128 tensor")
        else:
            raise TypeError(f"out: cannot write into {type(out)!r}")
    _rotate(src.reshape(-1, shape[-1]), lmax, angles, out.reshape(-1, shape[-1]))
    if isinstance(out, np.ndarray):
        if md:
            update_metadata(out, **md)
        return out
    return DeviceArray(out, md) if dressed else out


def rotate_alms(alms, psi=0.0, theta=0.0, phi=0.0, *, matrix=None, coord=None, device=None):
    """``rotate_alm`` for a dict ``{key: alm}``: all entries of equal lmax are rotated in one call of the library, so the Wigner
    matrices are computed once for them.  Keys, their order and the metadata of every entry are kept; each entry comes back as the
    kind it came in (or as a ``DeviceArray`` with ``device=``)."""
    angles = _angles(psi, theta, phi, matrix, coord)
    groups = {}
    for key, alm in alms.items():
        groups.setdefault((int(alm.shape[-1]), _is_tensor(getattr(alm, "tensor", alm))), []).append(key)
    done = {}
    for (nlm, tensor), keys in groups.items():
        rows = [getattr(alms[k], "tensor", alms[k]).reshape(-1, nlm) for k in keys]
        if tensor:
            import torch

            stack = torch.cat([r.to(torch.complex128) for r in rows])
        else:
            stack = np.concatenate([np.asarray(r, dtype=np.complex128) for r in rows])
        res = rotate_alm(stack, *angles, device=device)
        res = getattr(res, "tensor", res)
        first = 0
        for k, r in zip(keys, rows):
            src = alms[k]
            part = res[first : first + r.shape[0]].reshape(tuple(src.shape))
            first += r.shape[0]
            md = dict(getattr(getattr(src, "dtype", None), "metadata", None) or {})
            if _is_tensor(part):
                done[k] = DeviceArray(part, md) if isinstance(src, DeviceArray) or device is not None else part
            else:
                if md:
                    update_metadata(part, **md)
                done[k] = part
    out = TocDict()
    for key in alms:
        out[key] = done[key]
    return out
