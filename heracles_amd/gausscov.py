"""Mask-aware Gaussian covariance of pseudo-Cl under the narrow-kernel approximation (NKA; Garcia-Garcia et al. 2019, the form
NaMaster carries) on the GPU -- DESIGN.md 4.19.

For data-vector components C^{ab} and C^{cd}, where a, b, c, d each stand for a (field, bin, component E / B),

    Cov_{ll'} = Sbar^{ac}_{ll'} Sbar^{bd}_{ll'} Xi_{ll'}[(m_a m_c), (m_b m_d)] + Sbar^{ad}_{ll'} Sbar^{bc}_{ll'} Xi_{ll'}[(m_a m_d), (m_b m_c)]
    Sbar_{ll'} = (S_l + S_l') / 2
    Xi_{ll'}[X, Y] = sum_l'' (2l'' + 1) / (4 pi) W^{X,Y}_l'' (l l' l''; 0 0 0)^2

with S the fiducial spectra (``bias`` metadata added, as ``gaussian_covariance`` does), m_a the mask map of a's field and bin, keyed
``(fields[a].mask, bin)``, and W^{X,Y} the cross-spectrum of two products of mask maps.  Xi is the (0,0) mixing matrix of W with its
column factor (2l' + 1) divided out.  EVERY component uses this scalar coupling: E and B are treated as scalars, the spin-weighted
couplings Xi^{+-+-} are not formed.  The scalar form is exact for spin-0 fields with white spectra and an approximation otherwise
(the narrow-kernel step, and for fields of non-zero spin the scalar kernel in place of the spin-weighted ones).

Three layers:

* ``mask_product_cls``: the spectra W of the mask products the data vector needs (torch products, batched spin-0 ``map2alm``,
  ``alm2cl_pairs``), keyed by the canonical table key of ``table_key``;
* ``covariance_requests``: pure Python -- the layout of the data vector, the spectrum indices and, per coupling table, the list of
  blocks it serves;
* ``gaussian_covariance_coupled``: one ``MixmatContext``, one table build and one ``hx_gauss_cov_accumulate`` call per table; the
  dense N x N matrix stays in HBM, in the form ``shrinkage_factor`` / ``shrink`` take as ``target``.
"""

from __future__ import annotations

import itertools
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib
from .binning import BinPlan
from .core import Result
from .covariance import _check_dense, _cov_result, _expand_spin0, _Layout, _with_bias, get_cl

__all__ = ["mask_product_cls", "covariance_requests", "gaussian_covariance_coupled", "table_key"]


def table_key(key, tables=None):
    """The canonical form of a coupling-table key ``((k1, k2), (k3, k4))`` -- the cross-spectrum of the product maps m_k1 m_k2 and
    m_k3 m_k4 does not change when k1 and k2, k3 and k4, or the two pairs are swapped: both pairs sorted, then the pairs sorted.
    With ``tables`` (a mapping) the entry of ``key`` is returned instead: under the canonical key, or else under any of its
    equivalent forms; ``KeyError`` naming the key if there is none."""
    (a, b), (c, d) = key
    p, q = tuple(sorted((a, b))), tuple(sorted((c, d)))
    canon = (p, q) if p <= q else (q, p)
    if tables is None:
        return canon
    if canon in tables:
        return tables[canon]
    for x, y in ((p, q), (q, p)):
        for xx in (x, x[::-1]):
            for yy in (y, y[::-1]):
                if (xx, yy) in tables:
                    return tables[xx, yy]
    raise KeyError(f"no mask-product spectrum for the table {canon}")


def _mask_key(fields, name, i):
    if name not in fields:
        raise ValueError(f"unknown field name: {name}")
    mask = fields[name].mask
    if mask is None:
        raise ValueError(f"field {name!r} has no mask: the coupled covariance needs the mask of every field")
    return (mask, i)


def _term_tables(k1, k2, fields):
    """The canonical table keys of the two terms of the block (k1, k2): (m_a m_c, m_b m_d) and (m_a m_d, m_b m_c)."""
    a, b, i, j = k1
    c, d, k, m = k2
    ma, mb, mc, md = _mask_key(fields, a, i), _mask_key(fields, b, j), _mask_key(fields, c, k), _mask_key(fields, d, m)
    return table_key(((ma, mc), (mb, md))), table_key(((ma, md), (mb, mc)))


def _dof(spin):
    return 1 if spin == 0 else 2


@dataclass
class CovarianceRequests:
    """What ``covariance_requests`` hands to the driver.

    ``layout``: the ``_Layout`` of the data vector; ``nl``: multipoles per block; ``units``: the blocks of the data vector in order,
    ``(key, x, y)`` with x, y the component (0 = E or scalar, 1 = B) of the key's two fields -- unit u starts at ``u * nl`` (unbinned);
    ``spectra``: spectrum index -> ``((field, bin, comp), (field, bin, comp))``, the sorted pair of components it stands between;
    ``tables``: canonical table key -> list of ``(u1, u2, (s0, s1, s2, s3))`` with u1 <= u2, in sorted key order; s2 = s3 = -1
    where the block's other term reads another table."""

    layout: object
    nl: int
    units: list
    spectra: list
    tables: dict = field(default_factory=dict)

    @property
    def nitems(self):
        return sum(len(v) for v in self.tables.values())


def covariance_requests(cls, fields):
    """The work list of the coupled Gaussian covariance of the spectra ``cls`` (``(a, b, i, j) -> Result``) of ``fields``
    (name -> anything with ``spin`` and ``mask``).  Pure Python, deterministic: blocks in layout order, tables in sorted order."""
    lay = _Layout(cls)
    lengths = {key: (lay.ells[key][-1] if lay.ells[key] else 0) for key in lay.keys}
    for key in lay.keys:
        if len(lay.axis[key]) != 1:
            raise ValueError(f"spectrum {key} has {len(lay.axis[key])} angular axes, one is supported")
    nl = lengths[lay.keys[0]] if lay.keys else 0
    for key, n in lengths.items():
        if n != nl:
            raise ValueError(f"spectrum {key} has {n} multipoles, {lay.keys[0]} has {nl}: the coupled covariance needs one length")
    units, comps = [], []
    for key in lay.keys:
        a, b, i, j = key
        for name in (a, b):
            if name not in fields:
                raise ValueError(f"unknown field name: {name}")
        da, db = _dof(fields[a].spin), _dof(fields[b].spin)
        if lay.size[key] != da * db * nl:
            raise ValueError(f"spectrum {key} has {lay.size[key] // max(nl, 1)} components, its fields' spins give {da * db}")
        for x in range(da):
            for y in range(db):
                units.append((key, x, y))
                comps.append(((a, i, x), (b, j, y)))
    index, spectra = {}, []

    def spec(p, q):
        pair = (p, q) if p <= q else (q, p)
        if pair not in index:
            index[pair] = len(spectra)
            spectra.append(pair)
        return index[pair]

    found = {}
    tkeys = {}
    for u1, u2 in itertools.combinations_with_replacement(range(len(units)), 2):
        k1, k2 = units[u1][0], units[u2][0]
        if (k1, k2) not in tkeys:
            tkeys[k1, k2] = _term_tables(k1, k2, fields)
        t1, t2 = tkeys[k1, k2]
        (ca, cb), (cc, cd) = comps[u1], comps[u2]
        first, second = (spec(ca, cc), spec(cb, cd)), (spec(ca, cd), spec(cb, cc))
        if t1 == t2:
            found.setdefault(t1, []).append((u1, u2, first + second))
        else:
            found.setdefault(t1, []).append((u1, u2, first + (-1, -1)))
            found.setdefault(t2, []).append((u1, u2, second + (-1, -1)))
    return CovarianceRequests(lay, nl, units, spectra, {t: found[t] for t in sorted(found)})


def _spectrum_rows(cls, req):
    """(nspec, nl) array of the spectra ``req.spectra`` names, read with ``get_cl`` / ``_expand_spin0``."""
    rows = np.empty((max(len(req.spectra), 1), req.nl))
    cache = {}
    for s, ((a, i, x), (c, k, y)) in enumerate(req.spectra):
        key = (a, c, i, k)
        if key not in cache:
            cache[key] = np.asarray(_expand_spin0(get_cl(key, cls)).array, dtype=np.float64)
        block = cache[key]
        if block.shape[-1] != req.nl:
            raise ValueError(f"spectrum {key} has {block.shape[-1]} multipoles, the data vector has {req.nl}")
        rows[s] = block[x, y]
    return rows


# ---- mask products ------------------------------------------------------------------------------------------------------------------
def _as_tensor(m, device):
    import torch

    if hasattr(m, "tensor"):  # DeviceArray
        m = m.tensor
    if hasattr(m, "data_ptr") and not isinstance(m, np.ndarray):
        return m.to(device=device, dtype=torch.float64).reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64).reshape(-1)).to(device)


def mask_product_cls(mask_maps, fields, cls_keys=None, *, lmax, niter=0, device="cuda"):
    """The spectra of the mask products behind every coupling table of a data vector.

    ``mask_maps``: ``{(mask_name, bin): HEALPix map}`` (RING; numpy, CUDA tensor or ``DeviceArray``), what ``map_catalogs`` returns for
    ``Visibility`` / ``Weights`` fields; ``fields``: name -> field, whose ``mask`` names the mask of its maps; ``cls_keys``: the keys
    ``(a, b, i, j)`` of the data vector (default: every pair, with replacement, of the (field, bin) for which there is a mask map, in
    the order of ``fields`` and then of ``mask_maps``).  Returns ``{table_key(((k1, k2), (k3, k4))): W}`` with W (lmax + 1) the
    cross-spectrum of the maps m_k1 m_k2 and m_k3 m_k4.  The driver reads W up to twice the band limit of the spectra.

    The product maps are formed with torch, their alms in batched spin-0 ``map2alm`` calls (``niter`` Jacobi iterations each), the
    spectra in one ``alm2cl_pairs`` call;
    two keys bound to the same map object share their products and spectra."""
    import torch

    from .sht import get_plan
    from .twopoint import alm2cl_pairs

    _lib.ensure_init()
    if cls_keys is None:
        have = [(name, i) for name, f in fields.items() for (mask, i) in mask_maps if f.mask is not None and mask == f.mask]
        cls_keys = [(a, b, i, j) for (a, i), (b, j) in itertools.combinations_with_replacement(have, 2)]
    cls_keys = list(cls_keys)
    tables = {}
    for k1, k2 in itertools.combinations_with_replacement(cls_keys, 2):
        for t in _term_tables(k1, k2, fields):
            tables.setdefault(t, None)
    for t in tables:
        for pair in t:
            for k in pair:
                if k not in mask_maps:
                    raise KeyError(f"no mask map for {k}")
    # one tensor per map object, one product per unordered pair of objects, one spectrum per unordered pair of products
    tensors, ident = {}, {}
    for k, m in mask_maps.items():
        obj = m.tensor if hasattr(m, "tensor") else m
        ident[k] = id(obj)
        if id(obj) not in tensors:
            tensors[id(obj)] = _as_tensor(m, device)
    npix = {int(t.numel()) for t in tensors.values()}
    if len(npix) != 1:
        raise ValueError(f"the mask maps have different sizes: {sorted(npix)}")
    npix = npix.pop()
    nside = int(round((npix / 12) ** 0.5))
    if 12 * nside * nside != npix:
        raise ValueError(f"{npix} pixels are no HEALPix map")
    products, spectra = {}, {}

    def product_of(pair):
        pid = tuple(sorted((ident[pair[0]], ident[pair[1]])))
        return products.setdefault(pid, len(products)), pid

    wanted = {}
    for t in sorted(tables):
        (p, _), (q, _) = product_of(t[0]), product_of(t[1])
        sid = (min(p, q), max(p, q))
        wanted[t] = spectra.setdefault(sid, len(spectra))
    order = sorted(products, key=products.get)
    plan = get_plan(nside, int(lmax))
    alms = torch.empty((len(order), plan.nlm), dtype=torch.complex128, device=device)
    batch = 8
    for p0 in range(0, len(order), batch):
        maps = torch.stack([tensors[x] * tensors[y] for x, y in order[p0:p0 + batch]])
        plan.map2alm(maps, 0, niter=niter, out=alms[p0:p0 + maps.shape[0]])
    pairs = sorted(spectra, key=spectra.get)
    cl = alm2cl_pairs([alms[k] for k in range(len(order))], pairs, int(lmax))
    return {t: np.array(cl[wanted[t]]) for t in sorted(tables)}


# ---- the kernel call ----------------------------------------------------------------------------------------------------------------
#: hx_cov_item as a numpy record (``_lib.CovItem`` is the same struct for ctypes callers)
ITEM = np.dtype([("row", np.int64), ("col", np.int64), ("s", np.int32, (4,))])


def pack_items(items, scale=1):
    """A sequence of ``(row, col, (s0, s1, s2, s3))`` as the array of hx_cov_item the library reads; ``row`` and ``col`` times ``scale``
    (the driver's blocks count in units, a unit is one block edge).  An array of ``ITEM`` passes through."""
    if isinstance(items, np.ndarray) and items.dtype == ITEM:
        return np.ascontiguousarray(items)
    arr = np.empty(len(items), dtype=ITEM)
    if len(items):
        arr["row"] = np.fromiter((it[0] for it in items), dtype=np.int64, count=len(items)) * scale
        arr["col"] = np.fromiter((it[1] for it in items), dtype=np.int64, count=len(items)) * scale
        arr["s"] = np.array([it[2] for it in items], dtype=np.int32).reshape(len(items), 4)
    return arr


def _accumulate(g00, spec, items, cov, plan=None):
    """hx_gauss_cov_accumulate: add the blocks ``items`` -- ``(row, col, (s0, s1, s2, s3))``, s2 < 0 for one term -- of the table
    ``g00`` (L + 1, L + 1) and the spectra ``spec`` (nspec, L + 1) into the CUDA tensor ``cov`` (rows, ldc); ``plan``: the ``BinPlan`` of
    both axes, None for unbinned blocks."""
    nl = int(g00.shape[-1])
    arr = pack_items(items)
    if plan is None:
        nbins, which, w, norm = 0, None, None, None
    else:
        nbins = int(plan.nbins)
        which = np.ascontiguousarray(plan.which, dtype=np.int32)
        w = np.ascontiguousarray(plan.w, dtype=np.float64)
        norm = np.ascontiguousarray(plan.norm, dtype=np.float64)
    _lib.check(_lib.load().hx_gauss_cov_accumulate(nl - 1, _lib.ptr(g00), int(spec.shape[0]), _lib.ptr(spec), nbins, _lib.ptr(which),
                                                   _lib.ptr(w), _lib.ptr(norm), len(arr), _lib.ptr(arr) if len(arr) else None, _lib.ptr(cov),
                                                   int(cov.shape[-1])))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def gaussian_covariance_coupled(cls, mask_cls, fields, *, bins=None, weights=None, as_dict=False, out=None):
    """The mask-aware Gaussian covariance (NKA, scalar coupling for every component: module docstring) of the spectra ``cls``.

    ``cls``: ``(a, b, i, j) -> Result`` of one length L + 1, the fiducial spectra and at the same time the layout of the data vector;
    ``mask_cls``: the spectra of ``mask_product_cls`` (read up to 2L, shorter ones are zero beyond their end); ``fields``: name ->
    field with ``spin`` and ``mask``.  ``bins`` / ``weights``: one ``BinPlan`` over 0 .. L for both axes of every block,
    Cov_{bb'} = sum_{l in b, l' in b'} w_l w_l' Cov_{ll'} / (norm_b norm_b').

    Returns the dense N x N CUDA float64 tensor in data-vector order (``out``, if given, receives it) -- the ``target`` that
    ``shrinkage_factor`` takes as it is; with ``as_dict=True`` the dict of blocks in the format of ``jackknife_covariance`` /
    ``gaussian_covariance``, with the binned ``ell`` / ``lower`` / ``upper`` of the plan.

    ``ValueError`` for a field without a mask and for spectra of unequal length, ``KeyError`` naming the table for a missing mask
    spectrum -- all before anything is allocated."""
    import torch

    from .twopoint import MixmatContext

    req = covariance_requests(cls, fields)
    for t in req.tables:
        table_key(t, mask_cls)
    spec_rows = _spectrum_rows(_with_bias(cls), req)
    nl = req.nl
    if nl < 1:
        raise ValueError("the spectra are empty")
    L = nl - 1
    plan = None
    if bins is not None:
        plan = BinPlan(np.arange(nl), np.asarray(bins), weights)
        if plan.nbins < 1:
            raise ValueError("no bins")
    nbe = nl if plan is None else plan.nbins
    N = len(req.units) * nbe
    _check_dense(N, 3 if out is None else 2, "gaussian_covariance_coupled")
    _lib.ensure_init()
    device = torch.device("cuda", torch.cuda.current_device())
    if out is None:
        cov = torch.zeros((N, N), dtype=torch.float64, device=device)
    else:
        if not (hasattr(out, "is_cuda") and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (N, N)):
            raise ValueError(f"out must be a contiguous CUDA float64 tensor of shape {(N, N)}")
        cov = out.zero_()
    spec = torch.from_numpy(spec_rows).to(device)
    g00 = torch.empty((nl, nl), dtype=torch.float64, device=device)
    with MixmatContext(L, L, 2 * L) as ctx:
        for t, blocks in req.tables.items():
            wcl = np.asarray(table_key(t, mask_cls), dtype=np.float64)[: 2 * L + 1]
            ctx(wcl, (0, 0), out=g00)
            _accumulate(g00, spec, pack_items(blocks, nbe), cov, plan)
    # the blocks u1 <= u2 were formed: the strict lower triangle is the mirror of the upper one
    upper = torch.triu(cov, 1)
    cov.copy_(torch.triu(cov) + upper.T)
    del upper
    if not as_dict:
        return cov
    host = cov.cpu().numpy()
    first = {}
    for key in req.layout.keys:
        shape = req.layout.dofs[key] + (nbe,)
        src = cls[key]
        if plan is None:
            first[key] = Result(np.zeros(shape), spin=src.spin, axis=(len(shape) - 1,), ell=getattr(src, "ell", None))
        else:
            first[key] = Result(np.zeros(shape), spin=src.spin, axis=(len(shape) - 1,), ell=plan.ell, lower=plan.lower, upper=plan.upper)
    lay = _Layout(first)
    result = {}
    for k1, k2 in itertools.combinations_with_replacement(lay.keys, 2):
        key, res = _cov_result(first, k1, k2, lay.block(host, k1, k2))
        if plan is not None:
            res = replace(res, lower=(plan.lower, plan.lower), upper=(plan.upper, plan.upper))
        result[key] = res
    return result
