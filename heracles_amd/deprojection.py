"""Template deprojection of maps in HBM and the bias it leaves in the pseudo-Cl.

For one field and bin: ``d`` its map as ``map_catalogs`` returns it (already weighted by its mask ``v``), ``t_1 .. t_k`` its
systematics templates (unmasked, the shape of ``d``), ``f_i = v t_i``.  Sums over pixels also run over the components of the field
(one for spin 0, else two).  Then ::

    G_ij = sum f_i f_j,   r_i = sum f_i d,   alpha = G^+ r,   d_c = d - sum_i alpha_i f_i   (= P d, P = 1 - F G^+ F^T)

``G`` and ``r`` are one Gram matrix over the pixel axis (``hx_deproject_gram``, FP64 matrix unit), the removal is one streaming pass
(``hx_deproject_apply``).  The pseudo-inverse is taken on the host (``G`` is k x k): ``G`` is scaled to unit diagonal, a template with
a zero diagonal entry is dropped, and the eigenvalues of the scaled matrix at or below ``rcond`` times the largest are dropped.

``deprojection_bias`` is what the projection takes out of the expected pseudo-Cl, from P D P with D_ab = V_a Y_a C^{ab} Y_b^T V_b; it
is NaMaster's deprojection bias written in this library's transforms and subtracts with ``debias_cls``."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .core import DeviceArray, Result, update_metadata

__all__ = ["DeprojectionInfo", "deproject_templates", "deproject_maps", "deprojection_bias", "alm_apply_cl", "scaled_pinv"]


@dataclass
class DeprojectionInfo:
    """What ``deproject_templates`` found: ``gram`` (k, k) the matrix G on the host, ``inverse`` (k, k) its pseudo-inverse G^+,
    ``alpha`` (nmap, k) the fitted amplitudes, ``rank`` the number of eigenvalues kept, ``dropped`` the indices of the templates
    with a zero diagonal entry (all zero under the mask), ``removed`` (nmap,) alpha^T r, the sum of squares taken out of each map."""

    gram: np.ndarray
    inverse: np.ndarray
    alpha: np.ndarray
    rank: int
    dropped: tuple
    removed: np.ndarray


def _is_tensor(a):
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


def scaled_pinv(gram, rcond=1e-12):
    """(G^+, rank, dropped) by the rule of this module: unit-diagonal scaling, templates with a zero diagonal entry dropped,
    symmetric eigen-decomposition of the scaled matrix, eigenvalues <= rcond x (the largest) dropped."""
    G = np.asarray(gram, dtype=np.float64)
    k = G.shape[0]
    inv = np.zeros((k, k))
    d = np.diag(G)
    keep = np.flatnonzero(d > 0)
    dropped = tuple(int(i) for i in np.flatnonzero(~(d > 0)))
    if keep.size == 0:
        return inv, 0, dropped
    s = 1.0 / np.sqrt(d[keep])
    Gs = G[np.ix_(keep, keep)] * s[:, None] * s[None, :]
    w, V = np.linalg.eigh(0.5 * (Gs + Gs.T))
    good = w > rcond * w.max()
    Vg = V[:, good]
    inv[np.ix_(keep, keep)] = ((Vg / w[good]) @ Vg.T) * s[:, None] * s[None, :]
    return inv, int(good.sum()), dropped


def _f64(a, what):
    """``a`` (array, tensor or DeviceArray) as a contiguous float64 array or tensor."""
    if isinstance(a, DeviceArray):
        a = a.tensor
    if _is_tensor(a):
        import torch

        if a.is_complex():
            raise ValueError(f"{what} is complex: real maps are needed")
        return a.to(torch.float64).contiguous()
    return np.ascontiguousarray(a, dtype=np.float64)


def _map_columns(maps):
    """The maps as a list of (ncomp, npix) views of one contiguous float64 array or tensor, and that array."""
    a = _f64(maps, "maps")
    if a.ndim == 1:
        cols = [a[None, :]]
    elif a.ndim == 2:
        cols = [a]
    elif a.ndim == 3:
        cols = [a[m] for m in range(a.shape[0])]
    else:
        raise ValueError(f"maps have shape {tuple(a.shape)}: (npix,), (ncomp, npix) or (nmap, ncomp, npix) is needed")
    return cols, a


def _template_columns(templates):
    """The templates as a list of (ncomp, npix) contiguous float64 views: an array (ntemp, [ncomp,] npix) or a list of ([ncomp,] npix)."""
    if isinstance(templates, (list, tuple)):
        cols = []
        for i, t in enumerate(templates):
            t = _f64(t, f"template {i}")
            if t.ndim not in (1, 2):
                raise ValueError(f"template {i} has shape {tuple(t.shape)}: (npix,) or (ncomp, npix) is needed")
            cols.append(t[None, :] if t.ndim == 1 else t)
        return cols
    a = _f64(templates, "templates")
    if a.ndim == 2:
        return [a[i][None, :] for i in range(a.shape[0])]
    if a.ndim == 3:
        return [a[i] for i in range(a.shape[0])]
    raise ValueError(f"templates have shape {tuple(a.shape)}: (ntemp, npix) or (ntemp, ncomp, npix) is needed")


def _pointers(cols):
    arr = (C.c_void_p * max(len(cols), 1))()
    for i, c in enumerate(cols):
        arr[i] = _lib.ptr(c).value
    return arr


def _check_shapes(mcols, tcols, mask):
    ncomp, npix = (int(x) for x in mcols[0].shape)
    if ncomp not in (1, 2):
        raise ValueError(f"maps have {ncomp} components: 1 (spin 0) or 2 is supported")
    for i, t in enumerate(tcols):
        if tuple(t.shape) != (ncomp, npix):
            raise ValueError(f"template {i} has shape {tuple(t.shape)}, the maps have ({ncomp}, {npix})")
    if mask is not None and tuple(mask.shape) != (npix,):
        raise ValueError(f"the mask has shape {tuple(mask.shape)}, the maps have {npix} pixels")
    return ncomp, npix


def deproject_gram(templates, maps, mask=None):
    """``hx_deproject_gram``: the (n, n) matrix X^T X of the columns X = (v t_1 .. v t_k, d_1 .. d_m) on the host.  ``templates`` and
    ``maps`` are lists of (ncomp, npix) contiguous float64 arrays or CUDA tensors (either may be empty), ``mask`` (npix,) or None."""
    _lib.ensure_init()
    first = (list(maps) + list(templates))[0]
    ncomp, npix = (int(x) for x in first.shape)
    n = len(templates) + len(maps)
    gram = np.empty((n, n))
    _lib.check(_lib.load().hx_deproject_gram(npix, ncomp, len(templates), _pointers(templates), len(maps), _pointers(maps), _lib.ptr(mask),
                                             _lib.ptr(gram)))
    return gram


def deproject_apply(templates, mask, maps, alpha, outs):
    """``hx_deproject_apply``: outs[m] = maps[m] - mask * sum_i alpha[m][i] templates[i] (lists of (ncomp, npix) arrays or tensors)."""
    _lib.ensure_init()
    ncomp, npix = (int(x) for x in maps[0].shape)
    alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(len(maps), len(templates))
    _lib.check(_lib.load().hx_deproject_apply(npix, ncomp, len(templates), _pointers(templates), _lib.ptr(mask), len(maps), _pointers(maps),
                                              _lib.ptr(alpha) if alpha.size else None, _pointers(outs)))


def deproject_templates(maps, templates, mask=None, *, rcond=1e-12, out=None):
    """Remove the templates from the maps: ``(cleaned, info)`` with ``cleaned = d - sum_i alpha_i v t_i``, ``alpha = G^+ r``.

    ``maps``: ``(npix,)``, ``(ncomp, npix)`` or a stack ``(nmap, ncomp, npix)`` that shares the templates and the mask (already
    weighted by the mask, as ``map_catalogs`` returns them); ``templates``: ``(ntemp, [ncomp,] npix)`` or a list of arrays, unmasked;
    ``mask``: ``(npix,)`` or None for all ones.  numpy maps give a numpy result; a CUDA tensor or a ``DeviceArray`` stays on its
    device (a ``DeviceArray`` keeps its metadata).  ``out``: the destination, an array of the kind and shape of ``maps``; the input
    itself (float64, contiguous) works in place.  ``info`` is a :class:`DeprojectionInfo`.  A NaN or an infinite value in a template
    or a map is an ``HxError`` that names it; nothing is written then."""
    mcols, marr = _map_columns(maps)
    tcols = _template_columns(templates)
    vmask = None if mask is None else _f64(mask, "mask")
    ncomp, npix = _check_shapes(mcols, tcols, vmask)
    src = maps.tensor if isinstance(maps, DeviceArray) else maps
    shape = tuple(src.shape) if hasattr(src, "shape") else tuple(np.shape(src))
    if out is None:
        if _is_tensor(marr):
            import torch

            dst = torch.empty_like(marr)
        else:
            dst = np.empty_like(marr)
    else:
        dst = out.tensor if isinstance(out, DeviceArray) else out
        if _is_tensor(dst) != _is_tensor(marr) or tuple(dst.shape) != shape:
            raise ValueError(f"out must be of the kind and shape of maps, {shape}")
        if _is_tensor(dst):
            import torch

            ok = dst.dtype == torch.float64 and dst.is_contiguous()
        else:
            ok = isinstance(dst, np.ndarray) and dst.dtype == np.float64 and dst.flags.c_contiguous and dst.flags.writeable
        if not ok:
            raise ValueError("out must be float64, contiguous and writeable")
    ocols, _ = _map_columns(dst)
    k, nmap = len(tcols), len(mcols)
    gram = deproject_gram(tcols, mcols, vmask)
    G, r = gram[:k, :k], gram[:k, k:]
    inverse, rank, dropped = scaled_pinv(G, rcond)
    alpha = np.ascontiguousarray((inverse @ r).T)  # (nmap, k)
    deproject_apply(tcols, vmask, mcols, alpha, ocols)
    info = DeprojectionInfo(gram=np.array(G), inverse=inverse, alpha=alpha, rank=rank, dropped=dropped, removed=np.einsum("mi,im->m", alpha, r))
    if out is not None:
        return out, info
    cleaned = dst.reshape(shape)
    if isinstance(maps, DeviceArray):
        cleaned = DeviceArray(cleaned, maps.dtype.metadata)
    elif isinstance(maps, np.ndarray) and maps.dtype.metadata:
        update_metadata(cleaned, **maps.dtype.metadata)
    return cleaned, info


def _mask_of(fields, name, i, mask_maps):
    """The mask map of (name, i), found as ``gausscov._mask_key`` finds it."""
    if name not in fields:
        raise ValueError(f"unknown field name: {name}")
    mask = fields[name].mask
    if mask is None:
        raise ValueError(f"field {name!r} has no mask: deprojection needs the mask its maps are weighted by")
    if (mask, i) not in mask_maps:
        raise KeyError(f"mask_maps has no map for {(mask, i)!r}, the mask of {(name, i)!r}")
    return mask_maps[mask, i]


def _templates_of(templates, name, i):
    if (name, i) in templates:
        return templates[name, i]
    return templates.get(name)


def _dof(spin):
    return 1 if spin == 0 else 2


def deproject_maps(fields, maps, templates, mask_maps, *, rcond=1e-12):
    """``deproject_templates`` for every map of ``maps`` (``{(name, bin): map}`` as ``map_catalogs`` returns it) that has templates:
    ``templates`` is ``{name: ...}`` or ``{(name, bin): ...}`` (the latter wins), ``mask_maps`` is ``{(mask name, bin): map}`` with the
    mask name from ``fields[name].mask``.  Maps without templates pass through untouched.  Returns ``(maps, infos)``: new maps with the
    metadata of the old ones, and ``{(name, bin): DeprojectionInfo}`` for the cleaned ones.  An unknown field, a field without a mask
    and a shape that does not fit are a ``ValueError``, a missing mask map is a ``KeyError``; each names the key and is raised before
    anything is computed.  A key of ``templates`` that names no map is a ``KeyError`` too."""
    todo = {}
    for key in templates:
        if not any(key == mk or key == mk[0] for mk in maps):
            raise KeyError(f"templates has the key {key!r}, which names no map")
    for key, m in maps.items():
        name, i = key
        t = _templates_of(templates, name, i)
        if t is None:
            continue
        v = _mask_of(fields, name, i, mask_maps)
        try:
            mcols, _ = _map_columns(m)
            if len(mcols) != 1:
                raise ValueError(f"the map has shape {tuple(m.shape)}: one map per key is needed")
            tcols = _template_columns(t)
            dof = _dof(fields[name].spin)
            if mcols[0].shape[0] != dof:
                raise ValueError(f"the map has {mcols[0].shape[0]} components, a field of spin {fields[name].spin} has {dof}")
            _check_shapes(mcols, tcols, _f64(v, "mask"))
        except ValueError as err:
            raise ValueError(f"{key!r}: {err}") from None
        todo[key] = (t, v)
    out, infos = type(maps)(), {}
    for key, m in maps.items():
        if key not in todo:
            out[key] = m
            continue
        t, v = todo[key]
        out[key], infos[key] = deproject_templates(m, t, v, rcond=rcond)
    return out, infos


def alm_apply_cl(cl, alm_in, out=None):
    """``hx_alm_apply_cl``: ``out[x] = sum_y cl[x][y][l] alm_in[y]`` per (l, m).  ``cl`` (nout, nin, lmax + 1), ``alm_in`` (nin, nlm)
    complex128, numpy or a CUDA tensor; the result is of the kind of ``alm_in``, (nout, nlm)."""
    _lib.ensure_init()
    cl = np.ascontiguousarray(cl, dtype=np.float64) if not _is_tensor(cl) else cl.contiguous()
    if cl.ndim != 3:
        raise ValueError(f"cl has shape {tuple(cl.shape)}: (nout, nin, lmax + 1) is needed")
    nout, nin, nl = (int(x) for x in cl.shape)
    nlm = nl * (nl + 1) // 2
    a = alm_in.contiguous() if _is_tensor(alm_in) else np.ascontiguousarray(alm_in, dtype=np.complex128)
    if tuple(a.shape) != (nin, nlm):
        raise ValueError(f"alm_in has shape {tuple(a.shape)}, cl needs ({nin}, {nlm})")
    if out is None:
        if _is_tensor(a):
            import torch

            out = torch.empty((nout, nlm), dtype=torch.complex128, device=a.device)
        else:
            out = np.empty((nout, nlm), dtype=np.complex128)
    elif tuple(out.shape) != (nout, nlm):
        raise ValueError(f"out has shape {tuple(out.shape)}, the result has ({nout}, {nlm})")
    _lib.check(_lib.load().hx_alm_apply_cl(nl - 1, nin, nout, _lib.ptr(cl), _lib.ptr(a), _lib.ptr(out)))
    return out


class _Unit:
    """One (field, bin) with templates: f = v t on the device (k, dof, npix), the alms of f under the field's own analysis, G^+."""

    def __init__(self, key, field, t, v, info, device):
        import torch

        from .mapper import HipHealpixMapper

        mapper = field.mapper_or_error if hasattr(field, "mapper_or_error") else field.mapper
        if not isinstance(mapper, HipHealpixMapper):
            raise TypeError(f"{key!r}: deprojection_bias serves HipHealpixMapper fields, not {type(mapper).__name__}")
        self.key, self.spin, self.mapper, self.dof = key, int(field.spin), mapper, _dof(field.spin)
        cols = _template_columns(t)
        self.k = len(cols)
        dev = [c if _is_tensor(c) else torch.from_numpy(c).to(device) for c in cols]
        v = _f64(v, "mask")
        self.v = v if _is_tensor(v) else torch.from_numpy(v).to(device)
        npix = 12 * mapper.nside**2
        if tuple(self.v.shape) != (npix,) or any(tuple(c.shape) != (self.dof, npix) for c in dev):
            raise ValueError(f"{key!r}: templates and mask must be ({self.dof}, {npix}) and ({npix},) for nside {mapper.nside} and spin {self.spin}")
        self.M = np.asarray(info.inverse, dtype=np.float64)
        if self.M.shape != (self.k, self.k):
            raise ValueError(f"{key!r}: the info holds a {self.M.shape} inverse for {self.k} templates")
        self.f = torch.stack(dev) * self.v  # (k, dof, npix)
        self.alm_f = self.analyse(self.f)

    def analyse(self, maps):
        """(n, dof, npix) -> (n, dof, nlm): the transform the field's data go through."""
        n = maps.shape[0]
        alm = self.mapper.transform(maps[:, 0].contiguous() if self.spin == 0 else maps.contiguous(), self.spin)
        return alm.reshape(n, self.dof, -1)


def _block(cls, key, dof1, dof2):
    """The fiducial block of ``key`` as (dof1, dof2, nl)."""
    from .covariance import get_cl

    arr = np.asarray(get_cl(key, cls).array, dtype=np.float64)
    return np.ascontiguousarray(arr.reshape(dof1, dof2, arr.shape[-1]))


def deprojection_bias(cls, fields, templates, mask_maps, infos, *, lmax=None, keys=None):
    """The deprojection bias ``E[PCL(d_c^a, d_c^b)] - E[PCL(d^a, d^b)]`` of every key ``(a, b, i, j)`` of ``cls`` (or of ``keys``), as
    ``{key: Result}`` with blocks shaped like those of ``angular_power_spectra``; subtract it with ``debias_cls(cls, bias)``.

    ``cls`` are the fiducial spectra of the fields (read with ``get_cl``), ``templates`` and ``mask_maps`` as in ``deproject_maps``,
    ``infos`` what it returned.  With M = G^+, f_i = v t_i and
    ``g^{ab}_j = v_b alm2map_{s_b}(C^{ba} o map2alm_{s_a}(v_a f_a,j)) / pixel area`` (plain quadrature: no weights, no iterations) ::

        bias = - sum_ij M_a,ij PCL(f_a,i, g^{ab}_j) - sum_ij M_b,ij PCL(g^{ba}_j, f_b,i)
               + sum_ijkl M_a,ij M_b,kl (f_a,j . g^{ba}_k) PCL(f_a,i, f_b,l)

    where PCL is the pseudo-spectrum under each field's own mapper (its weights, iterations and deconvolution).  A field without
    templates drops its terms.  The alms of f_i, and of g_j per partner, are formed once and shared by the keys; everything stays in
    HBM.  ``lmax``: the band limit of the result (default: the smaller ``lmax`` of the two mappers).  ``HipHealpixMapper`` fields only."""
    import torch

    from .sht import get_plan
    from .twopoint import alm2cl_pairs

    _lib.ensure_init()
    device = torch.device("cuda", _lib.device())
    keys = list(cls) if keys is None else list(keys)
    units, galms = {}, {}

    def unit(name, i):
        if (name, i) not in units:
            if name not in fields:
                raise ValueError(f"unknown field name: {name}")
            t = _templates_of(templates, name, i)
            u = None
            if t is not None and len(_template_columns(t)) > 0:
                if (name, i) not in infos:
                    raise KeyError(f"infos has no entry for {(name, i)!r}, which has templates")
                u = _Unit((name, i), fields[name], t, _mask_of(fields, name, i, mask_maps), infos[name, i], device)
            units[name, i] = u
        return units[name, i]

    def g_of(ua, b, j):
        """(g^{ab} maps (k_a, dof_b, npix), their alms under b's analysis): D_ba f_a,j for every template j of a."""
        kb = (b, j)
        if (ua.key, kb) not in galms:
            fb = fields[b]
            mb = fb.mapper_or_error if hasattr(fb, "mapper_or_error") else fb.mapper
            if mb.nside != ua.mapper.nside:
                raise ValueError(f"{ua.key!r} and {kb!r} live at nside {ua.mapper.nside} and {mb.nside}: one resolution is needed")
            sb, dofb = int(fb.spin), _dof(fb.spin)
            cba = _block(cls, (b, ua.key[0], j, ua.key[1]), dofb, ua.dof)
            plan = get_plan(mb.nside, cba.shape[-1] - 1)
            vb = _f64(_mask_of(fields, b, j, mask_maps), "mask")
            vb = vb if _is_tensor(vb) else torch.from_numpy(vb).to(device)
            area = 4.0 * np.pi / plan.npix
            g = torch.empty((ua.k, dofb, plan.npix), dtype=torch.float64, device=device)
            for q in range(ua.k):
                a = plan.map2alm((ua.f[q] * ua.v).contiguous(), ua.spin).reshape(ua.dof, -1)
                plan.alm2map(alm_apply_cl(cba, a), sb, out=g[q])
            g *= vb / area
            ub = unit(b, j)
            if ub is not None:
                alm_g = ub.analyse(g)
            else:
                n = g.shape[0]
                alm_g = mb.transform(g[:, 0].contiguous() if sb == 0 else g, sb).reshape(n, dofb, -1)
            galms[ua.key, kb] = (g, alm_g)
        return galms[ua.key, kb]

    out = {}
    for key in keys:
        a, b, i, j = key
        ua, ub = unit(a, i), unit(b, j)
        fa, fb = fields[a], fields[b]
        dofa, dofb = _dof(fa.spin), _dof(fb.spin)
        ma = fa.mapper_or_error if hasattr(fa, "mapper_or_error") else fa.mapper
        mb = fb.mapper_or_error if hasattr(fb, "mapper_or_error") else fb.mapper
        lout = min(ma.lmax, mb.lmax) if lmax is None else min(int(lmax), ma.lmax, mb.lmax)
        shape = tuple(d for d, f in ((dofa, fa), (dofb, fb)) if f.spin != 0) + (lout + 1,)
        total = np.zeros((dofa, dofb, lout + 1))
        comps, pairs, terms = [], [], []

        def add(x, y, weight):
            """weight[p, q] x PCL(x[p], y[q]) over all (p, q): the rows go to the pair list, the contraction happens on the host."""
            base_x = len(comps)
            comps.extend(x.reshape(-1, x.shape[-1]))
            base_y = len(comps)
            comps.extend(y.reshape(-1, y.shape[-1]))
            start = len(pairs)
            for p in range(x.shape[0]):
                for q in range(y.shape[0]):
                    for cx in range(dofa):
                        for cy in range(dofb):
                            pairs.append((base_x + p * dofa + cx, base_y + q * dofb + cy))
            terms.append((start, x.shape[0], y.shape[0], weight))

        if ua is not None:
            _, alm_g = g_of(ua, b, j)  # g^{ab}: type b
            add(ua.alm_f, alm_g, -ua.M)
        if ub is not None:
            g_ba, alm_gba = g_of(ub, a, i)  # g^{ba}: type a
            add(alm_gba, ub.alm_f, -ub.M.T)
            if ua is not None:
                # S_jk = f_a,j . g^{ba}_k: the off-diagonal block of one Gram matrix
                cols = [ua.f[q] for q in range(ua.k)] + [g_ba[q] for q in range(ub.k)]
                S = deproject_gram([], cols, None)[: ua.k, ua.k :]
                add(ua.alm_f, ub.alm_f, ua.M @ S @ ub.M)
        if pairs:
            block = alm2cl_pairs(comps, pairs, lout)
            for start, nx, ny, weight in terms:
                part = np.asarray(block[start : start + nx * ny * dofa * dofb]).reshape(nx, ny, dofa, dofb, lout + 1)
                total += np.einsum("pq,pqxyl->xyl", weight, part)
        out[key] = Result(total.reshape(shape), spin=(int(fa.spin), int(fb.spin)), axis=-1)
    return out
