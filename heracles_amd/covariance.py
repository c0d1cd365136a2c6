"""Covariance estimators of DICES on the GPU: jackknife covariance, delete-2 debiasing and linear shrinkage.

The reference (heracles/dices/jackknife.py:449-593, heracles/dices/shrinkage.py:46-181, heracles/utils.py) takes the delete-1 /
delete-2 spectra of ``jackknife_cls`` to a covariance with a Welford loop per key pair and, for the shrinkage factor, an
(Njk, N, N) array of W matrices walked by a Python double loop.  Here every sample dict is flattened into one row of a data-vector
matrix X (n x N, the first sample's keys in order, each block dof-major then l), and the arithmetic runs in three private entry
points on hand-written FP64 matrix kernels (csrc/hx_covariance.hip):

* ``_gram``: alpha Dx^T Dy of the centred columns (jackknife_covariance, sample_covariance);
* ``_delete2_q``: the delete-2 ensemble, centred, and its per-l Gram matrices (delete2_correction keeps only l1 = l2);
* ``_shrink_sums``: numerator and denominator of the optimal shrinkage factor, contracted over the samples tile by tile.

The dict formats (keys, ``spin``, ``axis``, ``ell`` tuples, array layout) are the reference's.  Host helpers (``flatten``,
``impose_correlation``, ``get_cl``, ``gaussian_covariance``, ``shrink``) are plain numpy.

One deliberate deviation: the reference's ``shrinkage_factor`` flattens the target in the order of ``list(set(keys))``
(heracles/utils.py:188-190) while the samples are flattened in dict order, so which target entry meets which data entry depends on
PYTHONHASHSEED.  Here the target is always flattened in the order of the data vector (the first sample's keys), and
``flatten(cov)`` without ``order`` uses the order in which the row keys first appear in ``cov``.
"""

from __future__ import annotations

import itertools
from dataclasses import replace

import numpy as np

from . import _lib
from .core import Result

__all__ = [
    "sample_covariance", "jackknife_covariance", "delete2_correction", "debias_covariance", "gaussian_covariance",
    "shrinkage_factor", "shrink", "flatten", "impose_correlation", "get_cl", "bias", "jackknife_bias",
]


# ---- layout helpers ----------------------------------------------------------------------------------------------------------------
def _axis(result):
    axis = result.axis
    if axis is None:
        return (np.ndim(result.array) - 1,)
    if isinstance(axis, int):
        axis = (axis,)
    return tuple(a % np.ndim(result.array) for a in axis)


def _ell(result):
    """The ``ell`` tuple of a result, with the reference's defaults (heracles/result.py:53-73): one array per angular axis."""
    axis = _axis(result)
    ell = getattr(result, "ell", None)
    if ell is None:
        return tuple(np.arange(result.array.shape[a]) for a in axis)
    if isinstance(ell, tuple):
        return ell
    return (ell,) * len(axis)


class _Layout:
    """Where each key's block sits in the data vector: the array is moved to (dof..., l...) and raveled, so a block is dof-major
    then l -- the layout of heracles/utils.py:_flatten for spectra whose l axis is last."""

    def __init__(self, first):
        self.keys = list(first)
        self.offset, self.size, self.dofs, self.ells, self.axis = {}, {}, {}, {}, {}
        n = 0
        for key in self.keys:
            r = first[key]
            arr = np.asarray(r.array)
            axis = _axis(r)
            self.axis[key] = axis
            self.dofs[key] = tuple(s for a, s in enumerate(arr.shape) if a not in axis)
            self.ells[key] = tuple(arr.shape[a] for a in axis)
            self.offset[key], self.size[key] = n, arr.size
            n += arr.size
        self.n = n

    def vector(self, key, result):
        arr = np.asarray(result.array if hasattr(result, "array") else result, dtype=np.float64)
        axis = self.axis[key]
        if arr.ndim != len(self.dofs[key]) + len(axis):
            raise ValueError(f"sample of {key} has shape {arr.shape}, the first sample {self.dofs[key] + self.ells[key]}")
        arr = np.moveaxis(arr, axis, tuple(range(arr.ndim - len(axis), arr.ndim)))
        if arr.shape != self.dofs[key] + self.ells[key]:
            raise ValueError(f"sample of {key} has shape {arr.shape}, the first sample {self.dofs[key] + self.ells[key]}")
        return arr.reshape(-1)

    def pack(self, samples, out=None):
        """X (len(samples), N): one data vector per sample dict."""
        X = np.empty((len(samples), self.n)) if out is None else out
        for s, sample in enumerate(samples):
            for key in self.keys:
                if key not in sample:
                    raise ValueError(f"sample {s} has no key {key}")
                o = self.offset[key]
                X[s, o:o + self.size[key]] = self.vector(key, sample[key])
        return X

    def block(self, C, k1, k2):
        """The (k1, k2) block of a data-vector matrix as (dof1..., dof2..., l1..., l2...)."""
        o1, o2 = self.offset[k1], self.offset[k2]
        return self.arrange(C[o1:o1 + self.size[k1], o2:o2 + self.size[k2]], k1, k2)

    def arrange(self, b, k1, k2):
        """A (size1, size2) block as (dof1..., dof2..., l1..., l2...)."""
        d1, d2, e1, e2 = self.dofs[k1], self.dofs[k2], self.ells[k1], self.ells[k2]
        b = b.reshape(d1 + e1 + d2 + e2)
        n1, m1, n2 = len(d1), len(e1), len(d2)
        perm = list(range(n1)) + list(range(n1 + m1, n1 + m1 + n2)) + list(range(n1, n1 + m1)) + list(range(n1 + m1 + n2, b.ndim))
        return np.ascontiguousarray(b.transpose(perm))


def _cov_result(first, k1, k2, array):
    """The covariance Result of a key pair in the reference's format (heracles/dices/jackknife.py:476-500)."""
    r1, r2 = first[k1], first[k2]
    sa1, sb1 = r1.spin
    sa2, sb2 = r2.spin
    a1, b1, i1, j1 = k1
    a2, b2, i2, j2 = k2
    nax = len(_axis(r1)) + len(_axis(r2))
    res = Result(array, axis=tuple(range(-nax, 0)), spin=(sa1, sb1, sa2, sb2), ell=_ell(r1) + _ell(r2))
    return (a1, b1, a2, b2, i1, j1, i2, j2), res


# ---- memory guard ------------------------------------------------------------------------------------------------------------------
def _hbm_budget():
    """Bytes of device memory free for one dense product, or None when there is no device (the kernels then raise HxError)."""
    try:
        import torch

        if not torch.cuda.is_available():
            return None
        free, _ = torch.cuda.mem_get_info()
        return int(free)
    except Exception:  # noqa: BLE001 - no usable device: the library call reports it
        return None


def _check_dense(N, copies, what):
    need = 8 * N * N * copies
    budget = _hbm_budget()
    if budget is not None and need > 0.9 * budget:
        raise ValueError(f"{what}: the dense {N} x {N} FP64 matrix needs {need / 2**30:.1f} GiB of device memory, "
                         f"{budget / 2**30:.1f} GiB are free; bin the spectra (fewer l values) or select fewer keys")


# ---- the three entry points into the kernels ---------------------------------------------------------------------------------------
def _device():
    import torch

    _lib.ensure_init()
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(a, dtype=None):
    import torch

    if hasattr(a, "data_ptr"):
        return a.contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_device())


def _gram(X, Y=None, alpha=1.0):
    """alpha Dx^T Dy (numpy, N1 x N2) of the centred columns of X (n x N1) and Y (n x N2, default X) -- hx_cov_gram."""
    import torch

    n, n1 = X.shape
    n2 = n1 if Y is None else Y.shape[1]
    dx = _to_device(X, np.float64)
    dy = None if Y is None else _to_device(Y, np.float64)
    out = torch.empty((n1, n2), dtype=torch.float64, device=dx.device)
    _lib.check(_lib.load().hx_cov_gram(n, n1, n2, _lib.ptr(dx), _lib.ptr(dy), float(alpha), _lib.ptr(out)))
    host = np.empty((n1, n2))
    if host.size:
        _lib.copy(host, out)
    return host


def _delete2_q(njk, c0, c1, c2, pairs, perm, bstart, alpha):
    """The per-l Gram matrices of the delete-2 ensemble, back to back (numpy, sum of n_b^2) -- hx_cov_delete2.
    Q[k] = njk c0 - (njk - 1) (c1[pairs[k, 0]] + c1[pairs[k, 1]]) + (njk - 2) c2[k]; column p of the product is data column perm[p];
    batch b covers the columns [bstart[b], bstart[b + 1])."""
    import torch

    m, N = c2.shape
    pairs, perm, bstart = np.asarray(pairs), np.asarray(perm), np.asarray(bstart)
    if pairs.shape != (m, 2) or pairs.min(initial=0) < 0 or pairs.max(initial=0) >= len(c1):
        raise ValueError("delete-2 pairs must index the delete-1 samples")
    if perm.shape != (N,) or perm.min(initial=0) < 0 or perm.max(initial=0) >= N:
        raise ValueError("perm must be a column order of the data vector")
    if bstart[0] < 0 or bstart[-1] > N or np.any(np.diff(bstart) < 0):
        raise ValueError("bstart must be non-decreasing within the data vector")
    widths = np.diff(bstart)
    total = int(np.sum(widths.astype(np.int64) ** 2))
    d0, d1, d2 = _to_device(c0, np.float64), _to_device(c1, np.float64), _to_device(c2, np.float64)
    dp, dm, db = _to_device(pairs, np.int32), _to_device(perm, np.int32), _to_device(bstart, np.int32)
    out = torch.empty(max(total, 1), dtype=torch.float64, device=d0.device)
    _lib.check(_lib.load().hx_cov_delete2(int(njk), m, N, _lib.ptr(d0), _lib.ptr(d1), _lib.ptr(d2), _lib.ptr(dp), _lib.ptr(dm),
                                          len(bstart) - 1, _lib.ptr(db), float(alpha), _lib.ptr(out)))
    host = np.empty(total)
    if total:
        _lib.copy(host, out[:total])
    return host


def _shrink_sums(X, T):
    """(numerator, denominator) of the optimal shrinkage factor of the samples X (n x N) against the dense target T (N x N numpy
    array or CUDA tensor, data-vector order) -- hx_cov_shrink_sums."""
    import torch

    n, N = X.shape
    dx = _to_device(X, np.float64)
    dt = _to_device(T, np.float64)
    if dt.dtype != torch.float64:
        raise ValueError("target must be float64")
    out = torch.empty(2, dtype=torch.float64, device=dx.device)
    _lib.check(_lib.load().hx_cov_shrink_sums(n, N, _lib.ptr(dx), _lib.ptr(dt), N, _lib.ptr(out)))
    num, den = out.cpu().tolist()
    return num, den


# ---- jackknife covariance ----------------------------------------------------------------------------------------------------------
def _nd_alpha(m, nd):
    """Scale of D^T D: the unbiased sample covariance (1 / (m - 1)) times the jackknife factor (jackknife.py:480-486)."""
    if nd > 2:
        raise ValueError("number of deletions must be 0, 1, or 2")
    if nd == 1:
        return (m - 1) / m
    if nd == 2:
        njk = (1 + np.sqrt(1 + 8 * m)) / 2
        return (njk * (njk - 1) - 2) / (2 * njk * (njk + 1)) / (m - 1)
    return 1.0 / (m - 1)


def sample_covariance(samples, samples2=None):
    """Unbiased (n - 1) sample covariance of *samples* (n, *dim), or the cross-covariance with *samples2* (n, *dim2):
    shape (*dim, *dim2) (heracles/dices/jackknife.py:504-528)."""
    x = np.asarray(samples, dtype=np.float64)
    y = None if samples2 is None else np.asarray(samples2, dtype=np.float64)
    n, *dim = x.shape
    dim2 = dim if y is None else list(y.shape[1:])
    if y is not None and y.shape[0] != n:
        raise ValueError("different numbers of samples")
    c = _gram(x.reshape(n, -1), None if y is None else y.reshape(n, -1), 1.0 / (n - 1))
    return c.reshape(*dim, *dim2)


def jackknife_covariance(samples_dict, nd=1):
    """Jackknife covariance of the spectra dicts in ``samples_dict.values()`` (heracles/dices/jackknife.py:449-501):
    ``{(a1, b1, a2, b2, i1, j1, i2, j2): Result}`` over ``combinations_with_replacement`` of the first sample's keys, arrays
    (dof1..., dof2..., l1, l2) with ``axis=(-2, -1)``.  nd = 1 scales by (njk - 1)^2 / njk, nd = 2 by the delete-2 factor."""
    samples = list(samples_dict.values())
    if nd > 2:
        raise ValueError("number of deletions must be 0, 1, or 2")
    if len(samples) < 2:
        return {}
    first = samples[0]
    lay = _Layout(first)
    _check_dense(lay.n, 1, "jackknife_covariance")
    X = lay.pack(samples)
    C = _gram(X, None, _nd_alpha(len(samples), nd))
    cov = {}
    for k1, k2 in itertools.combinations_with_replacement(lay.keys, 2):
        key, res = _cov_result(first, k1, k2, lay.block(C, k1, k2))
        cov[key] = res
    return cov


# ---- delete-2 correction -----------------------------------------------------------------------------------------------------------
def delete2_correction(cls0, cls1, cls2):
    """The delete-2 correction Q of the jackknife covariance (heracles/dices/jackknife.py:531-566): the nd = 2 covariance of the
    ensemble Njk c0 - (Njk - 1) (c1[(k1,)] + c1[(k2,)]) + (Njk - 2) c2[(k1, k2)], of which only the l1 = l2 diagonal of every
    block is kept (dense blocks, zeros elsewhere).  Only those diagonals are computed: one Gram matrix per l index."""
    njk = len(cls1)
    pairs_keys = list(cls2)
    if len(pairs_keys) < 2:
        return {}
    for key in cls2[pairs_keys[0]]:
        if key not in cls0:
            raise ValueError(f"delete2_correction: cls0 has no key {key}")
    # the ensemble's results are dressed as cls0's (jackknife.py:552), so the layout and the metadata are cls0's
    first = {key: cls0[key] for key in cls2[pairs_keys[0]]}
    lay = _Layout(first)
    for key in lay.keys:
        if len(lay.axis[key]) != 1:
            raise ValueError(f"delete2_correction: {key} has {len(lay.axis[key])} angular axes, one is supported")
    c0 = lay.pack([cls0])[0]
    rows = {k: r for r, k in enumerate(cls1)}
    c1 = lay.pack(list(cls1.values()))
    pairs = np.empty((len(pairs_keys), 2), dtype=np.int32)
    for q, kk in enumerate(pairs_keys):
        k1, k2 = kk
        if (k1,) not in rows or (k2,) not in rows:
            raise ValueError(f"delete2_correction: cls1 has no delete-1 sample for region pair {kk}")
        pairs[q] = rows[(k1,)], rows[(k2,)]
    c2 = lay.pack([cls2[kk] for kk in pairs_keys])
    # l-major column order: for each l index b, the columns (key, dof) of every key with more than b values of l
    L = {k: lay.ells[k][0] for k in lay.keys}
    nd = {k: lay.size[k] // L[k] for k in lay.keys}
    lmax = max(L.values()) if L else 0
    perm, bstart, pos = [], [0], {k: np.zeros(L[k], dtype=np.int64) for k in lay.keys}
    for b in range(lmax):
        for k in lay.keys:
            if L[k] > b:
                pos[k][b] = len(perm) - bstart[-1]
                perm.extend(lay.offset[k] + np.arange(nd[k]) * L[k] + b)
        bstart.append(len(perm))
    perm = np.asarray(perm, dtype=np.int32)
    bstart = np.asarray(bstart, dtype=np.int32)
    m = len(pairs_keys)
    flat = _delete2_q(njk, c0, c1, c2, pairs, perm, bstart, _nd_alpha(m, 2))
    width = np.diff(bstart).astype(np.int64)
    goff = np.concatenate([[0], np.cumsum(width**2)[:-1]]).astype(np.int64)
    Q = {}
    for k1, k2 in itertools.combinations_with_replacement(lay.keys, 2):
        L1, L2 = L[k1], L[k2]
        bs = np.arange(min(L1, L2))
        e1, e2 = np.arange(nd[k1]), np.arange(nd[k2])
        idx = (goff[bs] + (pos[k1][bs] + e1[:, None, None]) * width[bs] + pos[k2][bs] + e2[None, :, None])
        q = np.zeros((nd[k1], nd[k2], L1, L2))
        q[:, :, bs, bs] = flat[idx]
        key, res = _cov_result(first, k1, k2, q.reshape(lay.dofs[k1] + lay.dofs[k2] + (L1, L2)))
        Q[key] = res
    return Q


def debias_covariance(cov_jk, cls0, cls1, cls2):
    """cov_jk - Q with Q the delete-2 correction (heracles/dices/jackknife.py:569-593)."""
    Q = delete2_correction(cls0, cls1, cls2)
    return {key: replace(cov_jk[key], array=cov_jk[key].array - Q[key].array) for key in cov_jk}


# ---- host helpers of heracles/utils.py and the bias bookkeeping ----------------------------------------------------------------------
def bias(cls):
    """{key: the ``bias`` entry of the dtype metadata, 0 if absent} (heracles/dices/jackknife.py:307-320)."""
    out = {}
    for key, res in cls.items():
        meta = res.dtype.metadata or {}
        out[key] = meta.get("bias", 0)
    return out


def jackknife_bias(bias, fsky, fields):
    """The biases scaled by the relative sky fraction (heracles/dices/jackknife.py:340-356)."""
    return {key: b * fsky for key, b in bias.items()}


def get_cl(key, cls):
    """``cls[key]``, or the symmetric key (b, a, j, i) with its dof axes and spins swapped (heracles/utils.py:28-52)."""
    if key in cls:
        return cls[key]
    a, b, i, j = key
    sym = (b, a, j, i)
    if sym not in cls:
        raise KeyError(f"Key {key} not found in Cls.")
    res = cls[sym]
    arr = res.array
    s1, s2 = res.spin
    if s1 != 0 and s2 != 0:
        arr = np.transpose(arr, axes=(1, 0, 2))
    return replace(res, array=arr, spin=(s2, s1))


def _expand_spin0(res):
    """A length-1 axis in place of every spin-0 component (heracles/utils.py:87-99)."""
    shape = list(res.array.shape)
    nzero = 0
    for pos, s in enumerate(res.spin):
        if s == 0:
            shape.insert(pos, 1)
            nzero += 1
    return replace(res, array=res.array.reshape(shape), axis=tuple(a + nzero for a in _axis(res)))


def _squeeze_spin0(res):
    """Drop the length-1 axes of spin-0 components (heracles/utils.py:102-115)."""
    shape = list(res.array.shape)
    keep = [d for pos, d in enumerate(shape[:len(res.spin)]) if res.spin[pos] != 0] + shape[len(res.spin):]
    nzero = sum(1 for s in res.spin if s == 0)
    return replace(res, array=res.array.reshape(keep), axis=tuple(a - nzero for a in _axis(res)))


def impose_correlation(cov_a, cov_b):
    """cov_a with the diagonal of cov_b: a_ij sqrt(b_ii b_jj) / sqrt(a_ii a_jj) per block (heracles/utils.py:118-138).
    Negative or zero diagonals give NaN / inf as in the reference."""
    out = {}
    for key in cov_a:
        a = np.asarray(cov_a[key].array)
        b = np.asarray(cov_b[key].array)
        sa = np.sqrt(np.diagonal(a, axis1=-2, axis2=-1)[..., None, :])
        sb = np.sqrt(np.diagonal(b, axis1=-2, axis2=-1)[..., None, :])
        c = a * (sb * np.swapaxes(sb, -1, -2))
        c /= sa * np.swapaxes(sa, -1, -2)
        out[key] = replace(cov_a[key], array=c)
    return out


def _dof(s):
    return 1 if s == 0 else 2


def _flatten_block(res):
    a = np.asarray(res.array)
    nax = len(_axis(res))
    L = a.shape[-1]
    if nax == 1:
        s1, s2 = res.spin
        return a.reshape(_dof(s1) * _dof(s2) * L)
    if nax == 2:
        s1, s2, s3, s4 = res.spin
        r, c = _dof(s1) * _dof(s2), _dof(s3) * _dof(s4)
        return a.reshape(r, c, L, L).transpose(0, 2, 1, 3).reshape(r * L, c * L)
    raise NotImplementedError("Flattening for >2 axes not implemented yet.")


def flatten(results, order=None):
    """Spectra -> one data vector (blocks in key order, each dof-major then l); covariances -> the dense matrix of the blocks in
    ``order`` (row keys (a, b, i, j)), a missing block taken as the transpose of its symmetric partner (heracles/utils.py:141-206).
    Without ``order`` the row keys are taken in the order of their first appearance (the reference: ``list(set(...))``)."""
    blocks = {key: _flatten_block(res) for key, res in results.items()}
    naxes = np.unique([len(_axis(res)) for res in results.values()])
    if len(naxes) != 1:
        raise ValueError("All results must have the same length axis to flatten.")
    if naxes[0] == 1:
        return np.concatenate(list(blocks.values()))
    if order is None:
        order = list(dict.fromkeys((k[0], k[1], k[4], k[5]) for k in blocks))
    rows = []
    for a1, b1, i1, j1 in order:
        row = []
        for a2, b2, i2, j2 in order:
            blk = blocks.get((a1, b1, a2, b2, i1, j1, i2, j2))
            if blk is None:
                blk = blocks.get((a2, b2, a1, b1, i2, j2, i1, j1))
                if blk is None:
                    raise KeyError(f"Missing block for {(a1, b1, a2, b2, i1, j1, i2, j2)}")
                blk = blk.T
            row.append(blk)
        rows.append(row)
    return np.block(rows)


# ---- Gaussian target and shrinkage -------------------------------------------------------------------------------------------------
def _with_bias(cls):
    """The fiducial spectra of the Gaussian covariances: every spectrum with its ``bias`` metadata added to every element
    (heracles/dices/shrinkage.py:112-116); shared by ``gaussian_covariance`` and ``gausscov.gaussian_covariance_coupled``."""
    bs = bias(cls)
    return {key: replace(res, array=res.array + bs[key]) for key, res in cls.items()}


def gaussian_covariance(cls):
    """Gaussian covariance of the spectra (heracles/dices/shrinkage.py:101-144), as the reference computes it: the auto-spectrum
    ``bias`` metadata added to every element, C(a1 a2) C(b1 b2) + C(a1 b2) C(b1 a2) on the l diagonal, no 1 / (2l + 1)."""
    cls = _with_bias(cls)
    cov = {}
    for k1, k2 in itertools.combinations_with_replacement(list(cls), 2):
        a1, b1, i1, j1 = k1
        a2, b2, i2, j2 = k2
        (ell1,) = _ell(cls[k1])
        (ell2,) = _ell(cls[k2])
        e1, e2 = _expand_spin0(cls[k1]), _expand_spin0(cls[k2])
        c13 = _expand_spin0(get_cl((a1, a2, i1, i2), cls)).array
        c24 = _expand_spin0(get_cl((b1, b2, j1, j2), cls)).array
        c14 = _expand_spin0(get_cl((a1, b2, i1, j2), cls)).array
        c23 = _expand_spin0(get_cl((b1, a2, j1, i2), cls)).array
        da1, db1, _ = e1.array.shape
        da2, db2, _ = e2.array.shape
        n = min(len(ell1), len(ell2))
        r = np.empty((da1, db1, da2, db2, n))
        # r[p, q, s, t] = c13[p, s] c24[q, t] + c14[p, t] c23[q, s]
        r[...] = c13[:, None, :, None, :] * c24[None, :, None, :, :] + c14[:, None, None, :, :] * c23[None, :, :, None, :]
        r = r[..., :, None] * np.eye(n)
        res = Result(r, spin=(*e1.spin, *e2.spin), ell=(ell1, ell2), axis=(-2, -1))
        cov[(a1, b1, a2, b2, i1, j1, i2, j2)] = _squeeze_spin0(res)
    return cov


def shrinkage_factor(cls1, target):
    """Optimal linear shrinkage factor lambda* of the delete-1 spectra ``cls1`` towards ``target`` (heracles/dices/shrinkage.py:66-98),
    not clipped to [0, 1].  ``target`` is a covariance dict -- flattened in the order of the data vector (the first sample's keys),
    not the reference's hash-seed dependent set order -- or a dense N x N float64 numpy array / CUDA tensor already in that order."""
    samples = list(cls1.values())
    lay = _Layout(samples[0])
    X = lay.pack(samples)
    if isinstance(target, dict):
        _check_dense(lay.n, 1, "shrinkage_factor")
        T = flatten(target, order=lay.keys)
    else:
        T = target
    if tuple(T.shape) != (lay.n, lay.n):
        raise ValueError(f"target has shape {tuple(T.shape)}, the data vector has {lay.n} entries")
    num, den = _shrink_sums(X, T)
    return num / den


def shrink(cov, target, shrinkage_factor):
    """lambda T' + (1 - lambda) C per block, T' the target with the correlation imposed from ``cov``'s diagonals
    (heracles/dices/shrinkage.py:46-63)."""
    tc = impose_correlation(target, cov)
    out = {}
    for key in cov:
        c = cov[key].array
        out[key] = replace(cov[key], array=shrinkage_factor * tc[key].array + (1 - shrinkage_factor) * c)
    return out
