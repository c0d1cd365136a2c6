"""Shifted lognormal mocks: the step from target spectra to the spectra of the underlying Gaussian fields and back,
the repair of matrices of spectra that come out of it slightly indefinite, and the exponentiation of the maps, all in HBM.

A *component* is numbered as ``synalm`` numbers it (one row per spin-0 field, E then B per field of spin >= 1, in the order of the
auto-spectra).  A spin-0 component is *lognormal* with shift lambda > 0, X = lambda (exp(g - sigma^2 / 2) - 1) >= -lambda with g a
Gaussian field of pixel variance sigma^2 = sum_l (2l + 1) / (4 pi) G_l, or *Gaussian*.  With xi the Legendre correlation function:

    both lognormal        xi_G = log1p(xi_C / (lambda_i lambda_j)),  xi_C = lambda_i lambda_j expm1(xi_G)
    lognormal x Gaussian  G_l = C_l / lambda_i      (harmonic space, no transform)
    both Gaussian         G = C

``lognormal_gaussian_cls`` / ``lognormal_realised_cls`` are the two directions (``hx_lognormal_xi`` between one ``cl2corr_columns`` and
one ``corr2cl_columns``), ``nearest_psd_cls`` the repair (``hx_cl_nearest_psd``), ``lognormal_maps`` the driver that ends in
``hx_lognormal_maps``."""

from __future__ import annotations

import dataclasses
import re

import numpy as np

from . import _lib
from .core import DeviceArray, TocDict, update_metadata
from .mocks import _fields_of, _is_tensor, _packed_spectra, gaussian_maps

__all__ = ["lognormal_xi", "lognormal_gaussian_cls", "lognormal_realised_cls", "nearest_psd_cls", "lognormal_transform_maps", "lognormal_maps",
           "default_psd_floor"]

#: the largest number of components of ``nearest_psd_cls`` and the sweep cap of its Jacobi iteration (PSD_MAXN, PSD_SWEEPS of
#: csrc/hx_lognormal.hip), restated for tests and tools
PSD_MAX_COMPONENTS, PSD_SWEEPS = 64, 40


def default_psd_floor(ncomp):
    """The eigenvalue floor ``nearest_psd_cls`` uses by default: 64 ncomp^2 2^-52, relative to a unit diagonal."""
    return 64.0 * int(ncomp) ** 2 * 2.0**-52


# ---- the three library calls -------------------------------------------------------------------------------------------------------------

def lognormal_xi(xi, factors, *, inverse=False, out=None):
    """``hx_lognormal_xi`` on columns ``xi`` (ncol, nnodes), numpy or a contiguous CUDA tensor: ``log1p(xi * factors[c])``, or with
    ``inverse`` ``factors[c] * expm1(xi)``; ``out`` may be ``xi``.  An argument of log1p that is <= -1 raises ``HxError`` naming the
    smallest (column, node) and writes nothing."""
    from .transforms import _columns_in, _columns_out

    in_place = out is xi
    xi = _columns_in(xi, "lognormal_xi")
    ncol, nnodes = (int(x) for x in xi.shape)
    fac = np.ascontiguousarray(factors, dtype=np.float64)
    if fac.shape != (ncol,):
        raise ValueError(f"lognormal_xi: {fac.size} factors for {ncol} columns")
    if ncol < 1 or nnodes < 1:
        raise ValueError(f"lognormal_xi: xi has shape {(ncol, nnodes)}")
    if in_place and not _is_tensor(xi) and not (isinstance(out, np.ndarray) and out is xi):
        raise ValueError("lognormal_xi: in place needs a C-contiguous float64 array")
    out = xi if in_place else _columns_out(xi, (ncol, nnodes), out)
    _lib.ensure_init()
    _lib.check(_lib.load().hx_lognormal_xi(1 if inverse else 0, ncol, nnodes, _lib.ptr(fac), _lib.ptr(xi), _lib.ptr(out)))
    return out


def lognormal_transform_maps(g, sigma2, shifts, *, out=None):
    """``hx_lognormal_maps``: ``out[r] = shifts[r] * expm1(g[r] - sigma2[r] / 2)`` for maps ``g`` (nrow, npix) or (npix,), numpy or a
    contiguous CUDA tensor; ``out`` defaults to ``g`` itself (in place)."""
    shape = tuple(int(x) for x in g.shape)
    if len(shape) not in (1, 2) or 0 in shape:
        raise ValueError(f"lognormal_transform_maps: maps of shape {shape}")
    nrow, npix = (1, shape[0]) if len(shape) == 1 else shape
    s2 = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma2, dtype=np.float64), (nrow,)))
    lam = np.ascontiguousarray(np.broadcast_to(np.asarray(shifts, dtype=np.float64), (nrow,)))
    if out is None:
        out = g
    if tuple(out.shape) != shape:
        raise ValueError(f"lognormal_transform_maps: out has shape {tuple(out.shape)}, the maps have {shape}")
    for a, name in ((g, "g"), (out, "out")):
        if _is_tensor(a):
            import torch

            if a.dtype != torch.float64 or not a.is_contiguous():
                raise ValueError(f"lognormal_transform_maps: {name} must be a contiguous float64 tensor")
        elif not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous:
            raise ValueError(f"lognormal_transform_maps: {name} must be a C-contiguous float64 array")
    _lib.ensure_init()
    _lib.check(_lib.load().hx_lognormal_maps(nrow, npix, _lib.ptr(s2), _lib.ptr(lam), _lib.ptr(g), _lib.ptr(out)))
    return out


def _ncomp_of_rows(npair):
    n = int(round((np.sqrt(8.0 * npair + 1.0) - 1.0) / 2.0))
    if n < 1 or n * (n + 1) // 2 != npair:
        raise ValueError(f"{npair} rows are not the packed upper triangle of a square matrix")
    return n


def _nearest_psd_packed(packed, floor, return_change):
    tensor = _is_tensor(packed)
    if tensor:
        import torch

        src = packed.to(torch.float64).contiguous()
    else:
        src = np.ascontiguousarray(packed, dtype=np.float64)
    if src.ndim != 2 or src.shape[1] < 1:
        raise ValueError(f"nearest_psd_cls: packed spectra of shape {tuple(src.shape)}, expected (ncomp (ncomp + 1) / 2, lmax + 1)")
    ncomp = _ncomp_of_rows(int(src.shape[0]))
    if ncomp > PSD_MAX_COMPONENTS:
        raise ValueError(f"nearest_psd_cls: {ncomp} components, at most {PSD_MAX_COMPONENTS} are supported")
    if floor is not None and not 0.0 <= float(floor) < 1.0:
        raise ValueError(f"nearest_psd_cls: floor = {floor!r}, expected 0 <= floor < 1 (relative to a unit diagonal)")
    nl = int(src.shape[1])
    if tensor:
        out = torch.empty_like(src)
        change = torch.empty(nl, dtype=torch.float64, device=src.device)
    else:
        out, change = np.empty_like(src), np.empty(nl)
    _lib.ensure_init()
    _lib.check(_lib.load().hx_cl_nearest_psd(ncomp, nl - 1, _lib.ptr(src), -1.0 if floor is None else float(floor), _lib.ptr(out), _lib.ptr(change)))
    return (out, change) if return_change else out


# ---- dicts of spectra <-> the packed matrix ----------------------------------------------------------------------------------------------

def _like(block, array):
    """``array`` dressed as ``block``: a Result keeps its fields (per-multipole arrays cut to the new length), an array its metadata."""
    if dataclasses.is_dataclass(block) and hasattr(block, "array"):
        old, new = np.shape(block.array)[-1], array.shape[-1]
        cut = {}
        for f in dataclasses.fields(block):
            v = getattr(block, f.name)
            if f.name != "array" and isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[-1] == old and new != old:
                cut[f.name] = v[..., :new]
        md = getattr(np.asarray(block.array).dtype, "metadata", None)
        if md:
            update_metadata(array, **md)
        return dataclasses.replace(block, array=array, **cut)
    md = getattr(getattr(block, "dtype", None), "metadata", None)
    if md:
        update_metadata(array, **md)
    return array


def _unpack_spectra(cls, fields, ncomp, packed):
    """The inverse of ``_packed_spectra``: a TocDict of the keys of ``cls`` with blocks of their shapes, read off the packed matrix."""
    nl = packed.shape[1]
    full = np.zeros((ncomp, ncomp, nl))
    iu = np.triu_indices(ncomp)
    full[iu] = packed
    full[(iu[1], iu[0])] = packed
    out = TocDict()
    for key, block in cls.items():
        k1, k2, i1, i2 = key
        a, b = fields[k1, i1], fields[k2, i2]
        shape = np.shape(getattr(block, "array", block))
        new = np.ascontiguousarray(full[a[0] : a[0] + a[1], b[0] : b[0] + b[1]]).reshape(shape[:-1] + (nl,))
        out[key] = _like(block, new)
    return out


def _component_shifts(fields, ncomp, shifts):
    """lambda per component (0: Gaussian) from ``{k or (k, i): lambda}``; the argument errors of the drivers."""
    lam = np.zeros(ncomp)
    for key, value in (shifts or {}).items():
        targets = [f for f in fields if f == key or f[0] == key]
        if not targets:
            raise ValueError(f"shifts: {key!r} names no field of cls")
        value = float(value)
        if not value > 0.0 or not np.isfinite(value):
            raise ValueError(f"shifts: the shift of {key!r} is {value!r}, a lognormal field needs a finite shift > 0")
        for f in targets:
            first, rows, spin = fields[f]
            if spin != 0 or rows != 1:
                raise ValueError(f"shifts: field {f!r} has spin {spin}; only spin-0 fields can be lognormal")
            lam[first] = value
    return lam


def _component_names(fields):
    names = {}
    for (k, i), (first, rows, spin) in fields.items():
        for r in range(rows):
            names[first + r] = (k, i) if rows == 1 else (k, i, "EB"[r])
    return names


def _convert(cls, shifts, lmax, nodes, inverse):
    from .transforms import cl2corr_columns, corr2cl_columns

    who = "lognormal_realised_cls" if inverse else "lognormal_gaussian_cls"
    fields, ncomp = _fields_of(cls)
    if not fields:
        raise ValueError("cls holds no auto-spectrum (k, k, i, i)")
    lam = _component_shifts(fields, ncomp, shifts)
    packed, lmax = _packed_spectra(cls, fields, ncomp, lmax)
    nodes = 2 * lmax + 2 if nodes is None else int(nodes)
    if nodes < lmax + 1:
        raise ValueError(f"{who}: nodes = {nodes}, at least lmax + 1 = {lmax + 1} are needed")
    ia, ib = np.triu_indices(ncomp)  # the component pair of each packed row
    both = (lam[ia] > 0) & (lam[ib] > 0)
    one = (lam[ia] > 0) ^ (lam[ib] > 0)
    out = packed.copy()
    if one.any():
        scale = np.where(lam[ia] > 0, lam[ia], lam[ib])[one][:, None]
        out[one] = packed[one] * scale if inverse else packed[one] / scale
    if both.any():
        import torch

        rows = np.flatnonzero(both)
        prod = lam[ia[rows]] * lam[ib[rows]]
        fam = np.zeros(rows.size, dtype=np.int32)
        dev = torch.device("cuda", _lib.device())
        a = torch.from_numpy(np.ascontiguousarray(packed[rows])).to(dev)
        xi = cl2corr_columns(a, fam, nodes - 1)
        try:
            lognormal_xi(xi, prod if inverse else 1.0 / prod, inverse=inverse, out=xi)
        except _lib.HxError as err:
            m = re.search(r"column (\d+), node (\d+)", str(err))
            if m is None:
                raise
            names = _component_names(fields)
            r = rows[int(m.group(1))]
            raise ValueError(f"{who}: the target correlation of {names[int(ia[r])]} x {names[int(ib[r])]} is <= -lambda_i lambda_j at "
                             f"Gauss-Legendre node {int(m.group(2))} of {nodes}: no Gaussian correlation gives it") from err
        out[rows] = corr2cl_columns(xi, fam, nodes - 1, nl=lmax + 1).cpu().numpy()
    return _unpack_spectra(cls, fields, ncomp, out)


def lognormal_gaussian_cls(cls, shifts, *, lmax=None, nodes=None):
    """The spectra of the Gaussian fields behind lognormal fields with target spectra ``cls``: a dict of the same keys, shapes and
    metadata.  ``cls`` is keyed and shaped as for ``synalm``; ``shifts`` is ``{k or (k, i): lambda}`` (a name alone shifts every bin
    of that field); fields without a shift stay Gaussian.  All lognormal x lognormal pairs go through one ``cl2corr_columns``, one
    ``hx_lognormal_xi`` and one ``corr2cl_columns`` at ``nodes`` Gauss-Legendre nodes (default 2 lmax + 2; the logarithm is not
    band-limited, so more than lmax + 1 are wanted) and are cut at ``lmax`` on the way back; lognormal x Gaussian pairs are divided by
    the shift, the rest passes through.  ``ValueError``: a shift on a field of spin != 0, a shift <= 0, a key that names no field, and
    a target correlation <= -lambda_i lambda_j (the message names the pair and the first node)."""
    return _convert(cls, shifts, lmax, nodes, False)


def lognormal_realised_cls(gaussian_cls, shifts, *, lmax=None, nodes=None):
    """The forward direction: the exact expected spectra, up to ``lmax``, of the lognormal fields made from Gaussian fields of spectra
    ``gaussian_cls`` -- what a mock is compared with, and what a repair by ``nearest_psd_cls`` is checked with."""
    return _convert(gaussian_cls, shifts, lmax, nodes, True)


def nearest_psd_cls(cls_or_packed, *, floor=None, return_change=False):
    """Spectra whose matrices C_l are all positive semi-definite, nearest to the given ones in the sense of clipped eigenvalues
    (``hx_cl_nearest_psd``): per l, with the diagonal scaled to one, eigenvalues below ``floor`` (default ``default_psd_floor(ncomp)``)
    are raised to it; a matrix that has none is returned bit for bit.  The result passes ``synalm``.

    The argument is a dict keyed and shaped as for ``synalm`` (a dict of the same keys comes back; spectra are cut to the shortest) or
    the packed array ``(ncomp (ncomp + 1) / 2, lmax + 1)`` of ``synalm_components``, numpy or a CUDA tensor (the same kind comes back).
    ``return_change``: also ``change[l] = max_ij |C' - C| / sqrt(C_ii C_jj)``, 0 where nothing was changed."""
    if not isinstance(cls_or_packed, dict):
        return _nearest_psd_packed(cls_or_packed, floor, return_change)
    fields, ncomp = _fields_of(cls_or_packed)
    if not fields:
        raise ValueError("cls holds no auto-spectrum (k, k, i, i)")
    packed, _ = _packed_spectra(cls_or_packed, fields, ncomp, None)
    fixed, change = _nearest_psd_packed(packed, floor, True)
    out = _unpack_spectra(cls_or_packed, fields, ncomp, fixed)
    return (out, change) if return_change else out


# ---- the driver --------------------------------------------------------------------------------------------------------------------------

def shear_factor(lmax):
    """f_l = sqrt((l + 2)(l - 1) / (l (l + 1))) for l >= 2, 0 below: E_lm = f_l kappa_lm."""
    l = np.arange(int(lmax) + 1, dtype=np.float64)
    f = np.zeros(int(lmax) + 1)
    f[2:] = np.sqrt((l[2:] + 2.0) * (l[2:] - 1.0) / (l[2:] * (l[2:] + 1.0)))
    return f


def _mapper_of(field):
    return field.mapper_or_error if hasattr(field, "mapper_or_error") else field.mapper


def lognormal_maps(fields, cls, shifts, *, seed, realisation=0, device=None, nodes=None, regularize=None, convergence=None):
    """Lognormal HEALPix maps ``{(k, i): map}`` with the target spectra ``cls`` for ``fields`` (name -> field with a
    ``HipHealpixMapper``), in the form ``gaussian_maps`` returns them: ready for ``mock_catalogs`` and ``transform``.

    ``lognormal_gaussian_cls(cls, shifts, nodes=nodes)`` at the largest ``lmax`` of the mappers; ``regularize="clip"`` then repairs
    the Gaussian spectra with ``nearest_psd_cls`` (with the default ``None`` a set that is not positive semi-definite fails as
    ``synalm`` fails, and the error says so); ``gaussian_maps`` with the same ``(seed, realisation)`` contract -- the order of the
    auto-spectra numbers the components --; then every lognormal field is exponentiated in place, X = lambda expm1(g - sigma^2 / 2)
    with sigma^2 = sum_l (2l + 1) / (4 pi) G_l of the spectra that were factored, up to the field's own lmax.  X >= -lambda exactly.

    ``convergence={shear: kappa}``: the maps of the spin-2 field ``shear`` are not drawn but derived, bin by bin, from the finished
    lognormal maps of the spin-0 field ``kappa`` (a lognormal field on a mapper of the same nside and lmax): ``kappa``'s mapper
    transforms the map (its weights, iterations and pixel-window setting), E_lm = + f_l kappa_lm with f_l = sqrt((l + 2)(l - 1) /
    (l (l + 1))) and B = 0 (``hx_alm_apply_cl``), and ``Plan.alm2map`` of spin 2 gives (Q, U).  The sign is that of HEALPix's spin-2
    convention, Q + iU = -sum (E + iB) 2Y_lm, in which the maps of a ``Shears`` field are kept: around a positive kappa the shear is
    tangential, Q cos 2 phi + U sin 2 phi < 0 with phi the position angle of the pixel seen from the peak, from south through east.
    A derived field must not appear in ``cls``.

    ``ValueError``: an unknown field name, a shift on a field of spin != 0, a shift <= 0, a ``shifts`` key that names no field of
    ``cls``, an unknown ``regularize``, and ``convergence`` entries that are not (spin-2 field, lognormal spin-0 field of the same
    nside and lmax) or whose shear field appears in ``cls``."""
    from .deprojection import alm_apply_cl
    from .sht import get_plan

    if regularize not in (None, "clip"):
        raise ValueError(f"regularize = {regularize!r}: None or \"clip\"")
    convergence = dict(convergence or {})
    cls_fields, ncomp = _fields_of(cls)
    if not cls_fields:
        raise ValueError("cls holds no auto-spectrum (k, k, i, i)")
    names = {key[0] for key in cls} | {key[1] for key in cls}
    for name in names | set(convergence) | set(convergence.values()):
        if name not in fields:
            raise ValueError(f"unknown field name: {name}")
    lam = _component_shifts(cls_fields, ncomp, shifts)
    for shear, kappa in convergence.items():
        if shear in names:
            raise ValueError(f"convergence: the maps of {shear!r} are derived from {kappa!r}; it must not appear in cls")
        if fields[shear].spin != 2:
            raise ValueError(f"convergence: {shear!r} has spin {fields[shear].spin}, a spin-2 field is needed")
        bins = [f for f in cls_fields if f[0] == kappa]
        if not bins or any(lam[cls_fields[f][0]] <= 0 for f in bins):
            raise ValueError(f"convergence: {kappa!r} must be a lognormal spin-0 field of cls (with a shift)")
        ms, mk = _mapper_of(fields[shear]), _mapper_of(fields[kappa])
        if (ms.nside, ms.lmax) != (mk.nside, mk.lmax):
            raise ValueError(f"convergence: the mappers of {shear!r} and {kappa!r} differ in nside or lmax")
    lmax = max(_mapper_of(fields[name]).lmax for name in names)
    gcls = lognormal_gaussian_cls(cls, shifts, lmax=lmax, nodes=nodes)
    if regularize == "clip":
        gcls = nearest_psd_cls(gcls)
    try:
        out = gaussian_maps(fields, gcls, seed=seed, realisation=realisation, device=device)
    except _lib.HxError as err:
        if regularize is None and "not positive semi-definite" in str(err):
            raise _lib.HxError(err.code, str(err).split(": ", 1)[-1] + " -- the Gaussianised spectra of a lognormal set can be slightly indefinite; "
                               "regularize=\"clip\" repairs them (nearest_psd_cls)") from err
        raise
    for key, (first, rows, spin) in cls_fields.items():
        if lam[first] <= 0:
            continue
        mapper = _mapper_of(fields[key[0]])
        g_l = np.asarray(getattr(gcls[key[0], key[0], key[1], key[1]], "array", gcls[key[0], key[0], key[1], key[1]]), dtype=np.float64)[: mapper.lmax + 1]
        sigma2 = float(np.sum((2.0 * np.arange(g_l.size) + 1.0) / (4.0 * np.pi) * g_l))
        m = out[key]
        lognormal_transform_maps(m.tensor if isinstance(m, DeviceArray) else m, sigma2, lam[first])
    for shear, kappa in convergence.items():
        mapper = _mapper_of(fields[kappa])
        plan = get_plan(mapper.nside, mapper.lmax)
        f = np.zeros((2, 1, mapper.lmax + 1))
        f[0, 0] = shear_factor(mapper.lmax)
        for name, i in [k for k in out if k[0] == kappa]:
            m = out[name, i]
            alm = mapper.transform(m, 0)
            a = alm.tensor if isinstance(alm, DeviceArray) else alm
            eb = alm_apply_cl(f, a.reshape(1, -1))
            qu = plan.alm2map(eb, 2)
            md = dict(geometry="healpix", kernel="healpix", nside=mapper.nside, lmax=mapper.lmax, deconv=_mapper_of(fields[shear]).deconvolve, spin=2)
            if isinstance(m, DeviceArray):
                out[shear, i] = DeviceArray(qu, md)
            else:
                update_metadata(qu, **md)
                out[shear, i] = qu
    return out
