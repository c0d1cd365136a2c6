"""Correlated Gaussian mocks of a set of spectra, generated in HBM: the inverse of ``angular_power_spectra``.

``synalm_components`` is the library call (``hx_synalm``): the packed matrix of spectra in, one alm row per component out.
``synalm`` takes spectra keyed and shaped as ``angular_power_spectra`` returns them and gives alms keyed as ``transform`` returns
them; ``gaussian_maps`` carries those on to HEALPix maps of the fields' mappers.  The definition of a realisation -- Philox4x32-10
with counter (l, m, component, realisation), Box-Muller, an unpivoted Cholesky factor per l -- is in DESIGN.md 4.15; a realisation is
a function of (seed, realisation, the order of the fields) alone and does not depend on lmax."""

from __future__ import annotations

import numpy as np

from . import _lib
from .core import DeviceArray, TocDict, update_metadata

__all__ = ["synalm_components", "synalm", "gaussian_maps"]

#: the tiling of the generator kernel (SYN_LT, SYN_MC, SYN_RB, SYN_RB_SMALL, SYN_MAXN of csrc/hx_synalm.hip), restated for tests and
#: tools: multipoles per work-group, orders per work item, output components per register block (and the smaller block of calls with
#: at most that many components), and the largest number of components
TILE_L, TILE_M, TILE_COMP, TILE_COMP_SMALL, MAX_COMPONENTS = 256, 2, 16, 8, 64


def _is_tensor(a):
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


def synalm_components(cl, ncomp, *, seed, realisation=0, out=None):
    """Gaussian alms ``(ncomp, nlm)`` complex128 with ``<a^i_lm conj(a^j_lm)> = C^{ij}_l``.

    cl: ``(ncomp (ncomp + 1) / 2, lmax + 1)``, rows in the order of ``itertools.combinations_with_replacement(range(ncomp), 2)`` --
    the array ``alm2cl_pairs(comps, that_pair_list, lmax)`` returns.  A numpy array gives a numpy array, a CUDA tensor a CUDA tensor;
    ``out`` (either kind, of the result's shape) receives the result instead.  ``seed`` < 2^64 and ``realisation`` < 2^32 select the
    mock; spectra that are not positive semi-definite at some l raise ``HxError`` and write nothing."""
    ncomp, seed, realisation = int(ncomp), int(seed), int(realisation)
    if not 0 <= seed < 2**64:
        raise ValueError("seed must be in [0, 2^64)")
    if not 0 <= realisation < 2**32:
        raise ValueError("realisation must be in [0, 2^32)")
    tensor = _is_tensor(cl)
    if tensor:
        import torch

        src = cl.to(torch.float64).contiguous()
    else:
        src = np.ascontiguousarray(cl, dtype=np.float64)
    if src.ndim != 2 or src.shape[0] != ncomp * (ncomp + 1) // 2 or src.shape[1] < 1:
        raise ValueError(f"cl has shape {tuple(src.shape)}, expected ({ncomp * (ncomp + 1) // 2}, lmax + 1) for {ncomp} components")
    lmax = int(src.shape[1]) - 1
    shape = (ncomp, (lmax + 1) * (lmax + 2) // 2)
    if out is None:
        if tensor:
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
    _lib.ensure_init()
    _lib.check(_lib.load().hx_synalm(ncomp, lmax, _lib.ptr(src), seed, realisation, _lib.ptr(out)))
    return out


def cl_cholesky(cl, ncomp):
    """The factor ``hx_synalm`` applies (``hx_cl_cholesky``): ``cl`` packed as for ``synalm_components``; L_ij (i >= j) comes back
    at the row of pair (j, i)."""
    src = np.ascontiguousarray(cl, dtype=np.float64)
    out = np.empty_like(src)
    _lib.ensure_init()
    _lib.check(_lib.load().hx_cl_cholesky(int(ncomp), int(src.shape[1]) - 1, _lib.ptr(src), _lib.ptr(out)))
    return out


def _block_spins(block):
    """(spin_1, spin_2) of a spectrum block: its dtype metadata, else the ``spin`` of a Result, else (None, None)."""
    array = getattr(block, "array", block)
    md = getattr(getattr(array, "dtype", None), "metadata", None) or {}
    if "spin_1" in md or "spin_2" in md:
        return md.get("spin_1"), md.get("spin_2")
    spin = getattr(block, "spin", None)
    if isinstance(spin, (tuple, list)) and len(spin) == 2:
        return spin[0], spin[1]
    return None, None


def _fields_of(cls):
    """The fields of a set of spectra: {(k, i): (first row, rows, spin)} from the auto-spectra (k, k, i, i), in the order of ``cls``."""
    fields, nrows = {}, 0
    for key, block in cls.items():
        k1, k2, i1, i2 = key
        if (k1, i1) != (k2, i2):
            continue
        shape = np.shape(getattr(block, "array", block))
        if len(shape) == 1:
            rows = 1
        elif len(shape) == 3 and shape[0] == shape[1]:
            rows = int(shape[0])
        else:
            raise ValueError(f"auto-spectrum {key} has shape {shape}, expected (nl,) or (rows, rows, nl)")
        spin = _block_spins(block)[0]
        if spin is None:
            if rows != 1:
                raise ValueError(f"auto-spectrum {key} has {rows} components and no spin: give spin_1 metadata or a Result with spin")
            spin = 0
        if (rows == 1) != (spin == 0):
            raise ValueError(f"auto-spectrum {key} of spin {spin} has {rows} component(s)")
        fields[k1, i1] = (nrows, rows, int(spin))
        nrows += rows
    return fields, nrows


def _packed_spectra(cls, fields, ncomp, lmax):
    """The matrix of spectra of all components, packed as ``synalm_components`` takes it; and the lmax used."""
    if lmax is None:
        lmax = min(np.shape(getattr(b, "array", b))[-1] for b in cls.values()) - 1
    lmax = int(lmax)
    full = np.zeros((ncomp, ncomp, lmax + 1))
    for key, block in cls.items():
        k1, k2, i1, i2 = key
        a, b = fields.get((k1, i1)), fields.get((k2, i2))
        if a is None or b is None:
            missing = (k1, i1) if a is None else (k2, i2)
            raise ValueError(f"spectrum {key}: no auto-spectrum {(missing[0], missing[0], missing[1], missing[1])} in cls")
        array = np.asarray(getattr(block, "array", block), dtype=np.float64)
        if array.shape[-1] < lmax + 1:
            raise ValueError(f"spectrum {key} has {array.shape[-1]} multipoles, lmax = {lmax} needs {lmax + 1}")
        if array.size != a[1] * b[1] * array.shape[-1]:
            raise ValueError(f"spectrum {key} has shape {array.shape}, its fields have {a[1]} and {b[1]} component(s)")
        array = array.reshape(a[1], b[1], -1)[..., : lmax + 1]
        for ra in range(a[1]):
            for rb in range(b[1]):
                if (k1, i1) == (k2, i2) and rb < ra:
                    continue  # (the upper triangle of an auto block is the matrix)
                full[a[0] + ra, b[0] + rb] = array[ra, rb]
                full[b[0] + rb, a[0] + ra] = array[ra, rb]
    iu = np.triu_indices(ncomp)  # row-major upper triangle = combinations_with_replacement order
    return np.ascontiguousarray(full[iu]), lmax


def synalm(cls, *, seed, realisation=0, lmax=None, device=None):
    """Gaussian alms ``{(k, i): alm}`` of the spectra ``cls``, keyed ``(k1, k2, i1, i2)`` with blocks shaped as
    ``angular_power_spectra`` returns them -- ``(nl,)``, ``(2, nl)``, ``(2, 2, nl)`` -- so that
    ``angular_power_spectra(synalm(cls, seed=...), debias=False)`` has the keys and shapes of ``cls`` and ``cls`` as expectation.

    The fields are the ``(k, i)`` of the auto-spectra ``(k, k, i, i)`` **in the order of the dict**; that order numbers the
    components (a spin-0 field is one, a field of spin s >= 1 is two, E then B) and is therefore part of the definition of the
    realisation: the same spectra in another order give another, equally valid, mock.  The rows of a field come from its auto block,
    its spin from the block's ``spin_1`` metadata or the Result's ``spin`` (a bare ``(nl,)`` array is spin 0).  A missing
    cross-spectrum is zero; a cross key may come in either order, ``(k2, k1, i2, i1)`` being the transpose; a cross key whose field
    has no auto-spectrum is a ``ValueError``.  ``lmax`` defaults to the shortest spectrum; shorter spectra are a ``ValueError``,
    longer ones are cut.  Each alm carries ``spin`` metadata; with ``device="cuda"`` they are ``DeviceArray`` views of one
    ``(N, nlm)`` tensor that never leaves HBM."""
    fields, ncomp = _fields_of(cls)
    if not fields:
        raise ValueError("cls holds no auto-spectrum (k, k, i, i)")
    packed, lmax = _packed_spectra(cls, fields, ncomp, lmax)
    if device is not None:
        import torch

        packed = torch.from_numpy(packed).to(device)
    alms = synalm_components(packed, ncomp, seed=seed, realisation=realisation)
    out = TocDict()
    for key, (first, rows, spin) in fields.items():
        part = alms[first] if rows == 1 else alms[first : first + rows]
        if device is not None:
            out[key] = DeviceArray(part, {"spin": spin})
        else:
            update_metadata(part, spin=spin)
            out[key] = part
    return out


def gaussian_maps(fields, cls, *, seed, realisation=0, device=None):
    """Gaussian HEALPix maps ``{(k, i): map}`` of the spectra ``cls`` for ``fields`` (name -> field with a ``HipHealpixMapper``):
    one ``synalm`` at the largest ``lmax`` of the mappers, each field's alm cut to its own mapper's ``lmax`` (``alm_resample``) and
    synthesised with ``get_plan(nside, lmax).alm2map(alm, spin)``.  The maps carry the ``spin``, ``nside`` and ``kernel`` metadata
    ``transform`` expects, so ``transform(fields, maps)`` runs on them; ``device="cuda"`` gives ``DeviceArray`` maps.

    No pixel window is applied: the maps are the band-limited field sampled at the pixel centres, not its average over the pixels.
    A mapper with ``deconvolve=True`` will nevertheless divide the alms it transforms by the window."""
    from .discrete import alm_resample
    from .sht import get_plan

    names = {key[0] for key in cls} | {key[1] for key in cls}
    for name in names:
        if name not in fields:
            raise ValueError(f"unknown field name: {name}")
    mappers = {name: fields[name].mapper_or_error if hasattr(fields[name], "mapper_or_error") else fields[name].mapper for name in names}
    lmax = max(m.lmax for m in mappers.values())
    alms = synalm(cls, seed=seed, realisation=realisation, lmax=lmax, device=device)
    out = TocDict()
    for (name, i), alm in alms.items():
        mapper, spin = mappers[name], fields[name].spin
        have = alm.dtype.metadata["spin"]
        if have != spin:
            raise ValueError(f"spin mismatch for field {name!r}: spectra have spin {have}, field has spin {spin}")
        data = alm.tensor if isinstance(alm, DeviceArray) else alm
        if mapper.lmax != lmax:
            data = alm_resample(data, mapper.lmax)
        m = get_plan(mapper.nside, mapper.lmax).alm2map(data, spin)
        md = dict(geometry="healpix", kernel="healpix", nside=mapper.nside, lmax=mapper.lmax, deconv=mapper.deconvolve, spin=spin)
        if isinstance(alm, DeviceArray):
            out[name, i] = DeviceArray(m, md)
        else:
            update_metadata(m, **md)
            out[name, i] = m
    return out
