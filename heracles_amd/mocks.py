"""Correlated Gaussian mocks of a set of spectra, generated in HBM: the inverse of ``angular_power_spectra``.

``synalm_components`` is the library call (``hx_synalm``): the packed matrix of spectra in, one alm row per component out.
``synalm`` takes spectra keyed and shaped as ``angular_power_spectra`` returns them and gives alms keyed as ``transform`` returns
them; ``gaussian_maps`` carries those on to HEALPix maps of the fields' mappers.  The definition of a realisation -- Philox4x32-10
with counter (l, m, component, realisation), Box-Muller, an unpivoted Cholesky factor per l -- is in DESIGN.md 4.15; a realisation is
a function of (seed, realisation, the order of the fields) alone and does not depend on lmax.

``poisson_catalog`` and ``mock_catalogs`` carry maps on to catalogues: Poisson counts of an expected-count map, points uniform on the
sphere within their pixels, and values read off maps at the points' pixels, all made in HBM (``hx_mockcat_counts`` /
``hx_mockcat_points``).  A catalogue is a function of (seed, realisation, nside, pixel, index) alone."""

from __future__ import annotations

import numpy as np

from . import _lib
from .core import DeviceArray, TocDict, update_metadata

__all__ = ["synalm_components", "synalm", "gaussian_maps", "poisson_catalog", "mock_catalogs"]

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


# ---- Poisson-sampled catalogues ----------------------------------------------------------------------------------------

#: points per work-group of the point kernel (MC_BLOCK of csrc/hx_mockcat.hip) and the switch between the two count samplers, restated
#: for tests and tools
POINTS_PER_GROUP, LAMBDA_SWITCH, LAMBDA_MAX = 256, 32.0, 2.0**30


def _data_of(a):
    """The tensor of a DeviceArray, else the array itself."""
    return a.tensor if isinstance(a, DeviceArray) else a


def _as_f64(a):
    a = _data_of(a)
    if _is_tensor(a):
        import torch

        return a.to(torch.float64).contiguous()
    return np.ascontiguousarray(a, dtype=np.float64)


def _mockcat_counts(nside, pix_begin, pix_end, lam, seed, realisation):
    """``hx_mockcat_counts``: (counts int64 of the kind of ``lam``, their total)."""
    import ctypes as C

    n = pix_end - pix_begin
    if _is_tensor(lam):
        import torch

        counts = torch.empty(n, dtype=torch.int64, device=lam.device)
    else:
        counts = np.empty(n, dtype=np.int64)
    total = C.c_int64(0)
    _lib.ensure_init()
    _lib.check(_lib.load().hx_mockcat_counts(nside, pix_begin, pix_end, _lib.ptr(lam), seed, realisation, _lib.ptr(counts), C.byref(total)))
    return counts, int(total.value)


def _mockcat_points(nside, pix_begin, pix_end, counts, total, seed, realisation, maps, sigma, like, pix=False):
    """``hx_mockcat_points``: (lon, lat, values [nval][total]) of the kind of ``like``; with ``pix`` the source pixels as a fourth."""
    nval = 0 if maps is None else int(maps.shape[0])
    if _is_tensor(like):
        import torch

        def empty(shape, dtype=torch.float64):
            return torch.empty(shape, dtype=dtype, device=like.device)

        ipix = empty(total, torch.int64) if pix else None
    else:
        empty = np.empty
        ipix = np.empty(total, dtype=np.int64) if pix else None
    lon, lat, values = empty(total), empty(total), empty((nval, total))
    sig = None if nval == 0 else np.ascontiguousarray(sigma, dtype=np.float64)
    _lib.ensure_init()
    _lib.check(_lib.load().hx_mockcat_points(nside, pix_begin, pix_end, _lib.ptr(counts), seed, realisation, nval, _lib.ptr(maps) if nval else None,
                                             _lib.ptr(sig) if nval else None, _lib.ptr(lon), _lib.ptr(lat), _lib.ptr(values) if nval else None,
                                             _lib.ptr(ipix)))
    return (lon, lat, values, ipix) if pix else (lon, lat, values)


def poisson_catalog(expected, values=None, *, nside=None, noise=None, seed, realisation=0, pixel_range=None, names=("ra", "dec"),
                    value_names=None, weight=None, page_size=None, visibility=None):
    """A Poisson-sampled catalogue of the expected-count map ``expected`` (RING): pixel p holds n_p ~ Poisson(expected[p]) points,
    uniform on the sphere within the pixel, in columns ``names`` (longitude, latitude in degrees); returns an ``ArrayCatalog``.

    values: ``(nval, npix)`` maps (or one ``(npix,)`` map); a point of pixel p gets ``values[j][p]`` (piecewise constant, no
    interpolation) plus ``noise[j]`` times a standard normal, in column ``value_names[j]`` (default ``value0`` ..).  ``weight="w"``
    adds a column of ones.  ``pixel_range=(begin, end)``: ``expected`` and ``values`` cover those pixels only and ``nside`` must be
    given; otherwise ``nside`` follows from the size of the map.  Pieces made range by range are the pieces of the whole catalogue.

    A CUDA tensor or ``DeviceArray`` gives CUDA float64 columns that never leave HBM, numpy gives numpy columns.  The rows are
    sorted by pixel, then by index within the pixel: **the order of the catalogue correlates with position** (pages are patches of
    the sky).  ``seed`` < 2^64 and ``realisation`` < 2^32 select the mock; the metadata records ``seed``, ``realisation``, ``nside``,
    ``total`` and ``pixel_range``.  An expected count that is NaN, negative or above 2^30, or 2^31 points and more in one call, raise
    ``HxError`` (use pixel ranges)."""
    from .catalog import ArrayCatalog

    seed, realisation = int(seed), int(realisation)
    if not 0 <= seed < 2**64:
        raise ValueError("seed must be in [0, 2^64)")
    if not 0 <= realisation < 2**32:
        raise ValueError("realisation must be in [0, 2^32)")
    lam = _as_f64(expected)
    if lam.ndim != 1:
        raise ValueError(f"expected has shape {tuple(lam.shape)}, a 1-D map is needed")
    n = int(lam.shape[0])
    if pixel_range is None:
        if nside is None:
            nside = int(round((n / 12) ** 0.5))
        nside = int(nside)
        if n != 12 * nside * nside:
            raise ValueError(f"expected has {n} pixels, which is not a HEALPix map" + (f" of nside {nside}" if nside else ""))
        begin, end = 0, n
    else:
        if nside is None:
            raise ValueError("pixel_range needs nside")
        nside = int(nside)
        begin, end = (int(x) for x in pixel_range)
        if not 0 <= begin <= end <= 12 * nside * nside or end - begin != n:
            raise ValueError(f"pixel_range {(begin, end)} does not match the {n} pixels of expected at nside {nside}")
    if not 1 <= nside <= 8192:
        raise ValueError(f"nside = {nside}, 1 .. 8192 are supported")
    maps = None
    if values is not None:
        maps = _as_f64(values)
        if maps.ndim == 1:
            maps = maps[None]
        if maps.ndim != 2 or maps.shape[1] != n:
            raise ValueError(f"values has shape {tuple(maps.shape)}, expected (nval, {n})")
        if _is_tensor(maps) != _is_tensor(lam):
            raise ValueError("values and expected must both be numpy arrays or both be tensors")
    nval = 0 if maps is None else int(maps.shape[0])
    sigma = np.zeros(nval) if noise is None else np.atleast_1d(np.asarray(noise, dtype=np.float64))
    if sigma.shape != (nval,):
        raise ValueError(f"noise has {sigma.size} entries for {nval} value columns")
    if value_names is None:
        value_names = tuple(f"value{j}" for j in range(nval))
    if len(value_names) != nval or len(names) != 2:
        raise ValueError(f"value_names names {len(value_names)} columns for {nval} value maps" if len(names) == 2 else "names must be (longitude, latitude)")
    counts, total = _mockcat_counts(nside, begin, end, lam, seed, realisation)
    lon, lat, vals = _mockcat_points(nside, begin, end, counts, total, seed, realisation, maps, sigma, lam)
    cols = {names[0]: lon, names[1]: lat}
    for j, name in enumerate(value_names):
        cols[name] = vals[j]
    if weight is not None:
        if _is_tensor(lon):
            import torch

            cols[weight] = torch.ones(total, dtype=torch.float64, device=lon.device)
        else:
            cols[weight] = np.ones(total)
    md = {"seed": seed, "realisation": realisation, "nside": nside, "total": total, "pixel_range": (begin, end)}
    return ArrayCatalog(cols, page_size=ArrayCatalog.default_page_size if page_size is None else page_size, visibility=visibility, metadata=md)


def bin_seed(seed, i):
    """The seed of bin ``i`` (an integer) of ``mock_catalogs``: (seed + 0x9E3779B97F4A7C15 (i + 1)) mod 2^64 -- the 64-bit golden-ratio
    increment, so that the bins of one seed, and bin i of seed s against bin j of seed s + 1, draw from different Philox keys."""
    if int(i) != i:
        raise TypeError(f"bin {i!r} is not an integer")
    return (int(seed) + 0x9E3779B97F4A7C15 * (int(i) + 1)) % 2**64


def _map_nside(m, key):
    md = getattr(getattr(m, "dtype", None), "metadata", None) or {}
    npix = int(m.shape[-1])
    nside = int(md.get("nside", round((npix / 12) ** 0.5)))
    if 12 * nside * nside != npix:
        raise ValueError(f"map {key} has {npix} pixels, which is not a HEALPix map of nside {nside}")
    return nside


def mock_catalogs(fields, maps, nbar, *, visibility=None, noise=None, seed, realisation=0, page_size=None):
    """Poisson-sampled catalogues ``{i: ArrayCatalog}`` of the maps ``maps`` (``{(name, i): map}``, as ``gaussian_maps`` returns
    them), ready for ``map_catalogs(fields, catalogs)``.

    For each bin ``i`` the map delta of the ``Positions`` field gives the expected counts nbar[i] vis max(0, 1 + delta): ``nbar`` (a
    number, or ``{i: number}``) is the expected count of a fully visible pixel, ``visibility`` a map, ``{i: map}`` or None; it becomes
    the catalogue's visibility.  Every other field with columns, a map ``(name, i)``, the longitude / latitude columns of the
    ``Positions`` field and its nside supplies value columns under its own column names: one row for a ``ScalarField``, two (real,
    imaginary) for a ``ComplexField`` / ``Shears``; weight columns are ones.  ``noise`` is ``{field name: sigma, or one per
    component}``.  Bin ``i`` is drawn with the seed ``bin_seed(seed, i)``, so bins are independent; ``realisation`` numbers the mocks.

    ``ValueError``: no ``Positions`` field, a bin without its ``Positions`` map, a map whose nside is not its mapper's, a map whose
    rows do not match its field's components, a bin without ``nbar``."""
    from .fields import ComplexField, Positions, ScalarField

    pos = [(name, f) for name, f in fields.items() if isinstance(f, Positions) and f.columns is not None]
    if not pos:
        raise ValueError("mock_catalogs needs a Positions field with columns")
    pos_name, pos_field = pos[0]
    lon_col, lat_col, pos_weight = pos_field.columns
    nside = int(pos_field.mapper_or_error.nside)
    bins = []
    for name, i in maps:
        if name in fields and i not in bins:
            bins.append(i)
    for i in bins:
        if (pos_name, i) not in maps:
            raise ValueError(f"bin {i!r}: no map of the Positions field {pos_name!r} in maps")
    out = {}
    for i in bins:
        delta = maps[pos_name, i]
        if _map_nside(delta, (pos_name, i)) != nside:
            raise ValueError(f"map {(pos_name, i)} has nside {_map_nside(delta, (pos_name, i))}, the mapper of {pos_name!r} has nside {nside}")
        delta = _as_f64(delta)
        if delta.ndim != 1:
            raise ValueError(f"map {(pos_name, i)} has {delta.shape[0]} rows, the Positions field has one component")
        if isinstance(nbar, dict):
            if i not in nbar:
                raise ValueError(f"nbar has no entry for bin {i!r}")
            nb = float(nbar[i])
        else:
            nb = float(nbar)
        vis = visibility.get(i) if isinstance(visibility, dict) else visibility
        tensor = _is_tensor(delta)
        if tensor:
            import torch

            lam = torch.clamp(1.0 + delta, min=0.0)
        else:
            lam = np.maximum(0.0, 1.0 + delta)
        if vis is not None:
            v = _as_f64(vis)
            if tuple(v.shape) != tuple(delta.shape):
                raise ValueError(f"the visibility of bin {i!r} has shape {tuple(v.shape)}, the maps have {tuple(delta.shape)}")
            if tensor != _is_tensor(v):
                v = torch.as_tensor(v, device=delta.device) if tensor else v.cpu().numpy()
            lam = nb * v * lam
        else:
            lam = nb * lam
        rows, sigmas, value_names, ones = [], [], [], []
        if pos_weight is not None:
            ones.append(pos_weight)
        for name, f in fields.items():
            if f is pos_field or (name, i) not in maps or f.columns is None or not isinstance(f, (ScalarField, ComplexField)):
                continue
            if f.columns[:2] != (lon_col, lat_col) or int(f.mapper_or_error.nside) != nside:
                continue
            m = maps[name, i]
            if _map_nside(m, (name, i)) != nside:
                raise ValueError(f"map {(name, i)} has nside {_map_nside(m, (name, i))}, the mapper of {name!r} has nside {nside}")
            m = _as_f64(m)
            want = 2 if isinstance(f, ComplexField) else 1
            have = 1 if m.ndim == 1 else int(m.shape[0])
            if have != want or m.ndim > 2:
                raise ValueError(f"map {(name, i)} has {have} rows, field {name!r} has {want} component(s)")
            if tensor != _is_tensor(m):
                m = torch.as_tensor(m, device=delta.device) if tensor else m.cpu().numpy()
            sig = np.broadcast_to(np.asarray((noise or {}).get(name, 0.0), dtype=np.float64), (want,))
            for r in range(want):
                if f.columns[2 + r] in value_names:
                    continue  # (two fields that read one column: the first map wins)
                rows.append(m if m.ndim == 1 else m[r])
                sigmas.append(float(sig[r]))
                value_names.append(f.columns[2 + r])
            w = f.columns[2 + want]
            if w is not None and w not in ones:
                ones.append(w)
        ones = [w for w in ones if w not in value_names]
        if len(set(ones)) > 1:
            raise ValueError(f"bin {i!r}: the fields name different weight columns {ones}; a mock has unit weights in one column")
        if rows:
            values = torch.stack(rows) if tensor else np.stack(rows)
        else:
            values = None
        out[i] = poisson_catalog(lam, values, nside=nside, noise=sigmas if rows else None, seed=bin_seed(seed, i), realisation=realisation,
                                 names=(lon_col, lat_col), value_names=tuple(value_names), weight=ones[0] if ones else None,
                                 page_size=page_size, visibility=vis)
    return out
