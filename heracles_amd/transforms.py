"""Cl <-> correlation function transforms on the GPU.

Mirrors heracles/transforms.py: ``_cl2corr`` / ``_corr2cl`` (transforms.py:115-204) and the
dict-level ``cl2corr`` / ``corr2cl`` (transforms.py:207-363).  The reference loops over
lmax+1 Gauss-Legendre nodes in Python; here all nodes and all spectra go in one launch.
"""

from __future__ import annotations

from dataclasses import replace

import numpy as np

from . import _lib

_gl_cache: dict = {}


def gauss_legendre(n: int):
    """Nodes and weights; usable as the reference's ``transforms.gauss_legendre`` hook."""
    if n not in _gl_cache:
        x = np.empty(n)
        w = np.empty(n)
        _lib.ensure_init()
        _lib.check(_lib.load().hx_gauss_legendre(int(n), _lib.ptr(x), _lib.ptr(w)))
        x.flags.writeable = False
        w.flags.writeable = False
        _gl_cache[n] = (x, w)
    return _gl_cache[n]


def wigner_d_table(lmax, a, b, x):
    """d^l_{ab}(x_k) for l=0..lmax at all x: array (len(x), lmax+1)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty((x.shape[0], lmax + 1))
    _lib.ensure_init()
    _lib.check(_lib.load().hx_wigner_d_table(int(lmax), int(a), int(b), x.shape[0], _lib.ptr(x), _lib.ptr(out)))
    return out


def legendre_funcs(lmax, x, m=(0, 2), lfacs=None, lfacs2=None, lrootfacs=None):
    """``heracles.transforms.legendre_funcs`` (heracles/transforms.py:46-112) for a scalar ``x``: the list
    ``[(P, P'), (d11, dm11), (d20, d22, d2m2)]`` restricted to the requested ``m``; P starts at l = 0, the spin-1 arrays at
    l = 1, the spin-2 arrays at l = 2.  The values come from the Wigner-d tables of the mixing-matrix kernels (three-term
    recursions in l, stable also where the reference switches to its small-angle series); ``lfacs*`` are accepted and ignored."""
    xs = np.array([float(x)])
    res = []
    if 0 in m:
        P = wigner_d_table(lmax, 0, 0, xs)[0]
        dP = np.zeros(lmax + 1)
        # P'_l = P'_{l-2} + (2l - 1) P_{l-1}
        inc = (2.0 * np.arange(1, lmax + 1) - 1.0) * P[:-1]
        dP[1::2] = np.cumsum(inc[0::2])
        dP[2::2] = np.cumsum(inc[1::2])
        res.append((P, dP))
    if 1 in m:
        res.append((wigner_d_table(lmax, 1, 1, xs)[0, 1:], wigner_d_table(lmax, -1, 1, xs)[0, 1:]))
    if 2 in m:
        res.append((wigner_d_table(lmax, 2, 0, xs)[0, 2:], wigner_d_table(lmax, 2, 2, xs)[0, 2:], wigner_d_table(lmax, 2, -2, xs)[0, 2:]))
    return res


def _as4(arr):
    arr = np.asarray(arr, dtype=np.float64)
    if arr.ndim == 1:
        z = np.zeros_like(arr)
        arr = np.array([arr, z, z, z]).T
    return arr


def _cl2corr(cls, lmax=None, sampling_factor=1):
    """(L,4) [TT,EE,BB,TE] -> (N,4) [T, Q+U, Q-U, cross] at N=lmax+1 GL nodes."""
    if sampling_factor != 1:
        raise NotImplementedError("sampling_factor != 1")
    cls = _as4(cls)
    if lmax is None:
        lmax = cls.shape[0] - 1
    c = np.ascontiguousarray(cls[: lmax + 1])[None]
    out = np.empty_like(c)
    _lib.ensure_init()
    _lib.check(_lib.load().hx_cl2corr(int(lmax), 1, _lib.ptr(c), _lib.ptr(out)))
    return out[0]


def _corr2cl(corrs, lmax=None, sampling_factor=1):
    if sampling_factor != 1:
        raise NotImplementedError("sampling_factor != 1")
    corrs = _as4(corrs)
    if lmax is None:
        lmax = corrs.shape[0] - 1
    c = np.ascontiguousarray(corrs)[None]
    out = np.empty((1, lmax + 1, 4))
    _lib.ensure_init()
    _lib.check(_lib.load().hx_corr2cl(int(lmax), 1, _lib.ptr(c), _lib.ptr(out)))
    return out[0]


def _batch(fn, specs, lmax):
    """Run cl2corr/corr2cl on a list of (L,4) arrays in one launch."""
    c = np.ascontiguousarray(np.stack(specs))
    out = np.empty_like(c)
    _lib.ensure_init()
    _lib.check(fn(int(lmax), c.shape[0], _lib.ptr(c), _lib.ptr(out)))
    return out


def _ell_len(res):
    ell = getattr(res, "ell", None)
    if ell is None:
        return res.shape[res.axis[0]]
    if isinstance(ell, tuple):
        ell = ell[0]
    return len(ell)


def _exact_key(spin):
    """Whether a key of these spins leaves the reference's "like spin 2" rule under ``exact_spin``: any spin outside {0, 2}."""
    return any(abs(int(s)) not in (0, 2) for s in spin)


def spin_pairs(spin):
    """The (a, b) of the columns of a spectrum of spins (s1, s2), one row per column: (0,0) on T_00; one spin zero: two columns on
    T_{s,0}; both non-zero: two on T_{s1,s2}, two on T_{s1,-s2}, in the key's own order of the spins."""
    s1, s2 = (int(s) for s in spin)
    if s1 != 0 and s2 != 0:
        return [(s1, s2), (s1, s2), (s1, -s2), (s1, -s2)]
    if s1 != 0 or s2 != 0:
        return [(s1 or s2, 0)] * 2
    return [(0, 0)]


def _exact_columns(fn, items, pack):
    """Columns of the keys of ``items`` ({key: Result}) through the pair path, one call per band limit: {key: (ncols, length)}."""
    out = {}
    for lm in sorted({_ell_len(r) - 1 for r in items.values()}):
        keys = [k for k, r in items.items() if _ell_len(r) - 1 == lm]
        cols = [pack(np.asarray(items[k].array, dtype=np.float64), items[k].spin) for k in keys]
        pairs = np.concatenate([np.asarray(spin_pairs(items[k].spin), dtype=np.int32) for k in keys])
        res = fn(np.concatenate(cols), pairs, lm)
        at = 0
        for k, c in zip(keys, cols):
            out[k] = res[at : at + len(c)]
            at += len(c)
    return out


def _pack_fwd(a, spin):
    s1, s2 = spin
    if s1 != 0 and s2 != 0:
        return np.stack([a[0, 0] + a[1, 1], a[1, 0] - a[0, 1], -a[0, 1] - a[1, 0], a[0, 0] - a[1, 1]])
    return np.stack([a[0] + a[1], a[0] - a[1]])


def _pack_back(a, spin):
    s1, s2 = spin
    if s1 != 0 and s2 != 0:
        return np.stack([a[0, 0], a[0, 1], a[1, 0], a[1, 1]])
    return np.stack([a[0], a[1]])


def cl2corr(cls, exact_spin=False):
    """Dict of Result spectra -> dict of correlation functions (transforms.py:207-283).

    The reference transforms every non-zero spin "like spin 2".  With ``exact_spin`` a key with a spin outside {0, 2} runs on the
    Wigner functions of its own spins instead (``cl2corr_columns`` with pairs: d^l_{s,0}, d^l_{s1,s2}, d^l_{s1,-s2}), placed as the
    spin-2 cases are; keys of spins {0, 2} go as without it, bit for bit."""
    L = _lib.load()
    exact = {key: cl for key, cl in cls.items() if exact_spin and _exact_key(cl.spin)}
    xi_exact = _exact_columns(cl2corr_columns, exact, _pack_fwd) if exact else {}
    work, plan = [], []
    for key, cl in cls.items():
        if key in exact:
            continue
        s1, s2 = cl.spin
        lmax = _ell_len(cl) - 1
        a = np.asarray(cl.array)
        z = np.zeros(lmax + 1)
        if s1 != 0 and s2 != 0:
            specs = [np.array([z, a[0, 0], a[1, 1], z]).T, np.array([z, -a[0, 1], a[1, 0], z]).T]
        elif s1 != 0 or s2 != 0:
            specs = [np.array([z, z, z, a[0] + a[1]]).T, np.array([z, z, z, a[0] - a[1]]).T]
        else:
            specs = [np.array([a, z, z, z]).T]
        plan.append((key, lmax, len(work), len(specs)))
        work.extend((lmax, s) for s in specs)
    outs = [None] * len(work)
    for lm in sorted({w[0] for w in work}):
        ids = [i for i, w in enumerate(work) if w[0] == lm]
        res = _batch(L.hx_cl2corr, [work[i][1] for i in ids], lm)
        for i, r in zip(ids, res):
            outs[i] = r
    plan = {p[0]: p for p in plan}
    wds = {}
    for key, cl in cls.items():
        s1, s2 = cl.spin
        a = np.asarray(cl.array)
        if key in exact:
            lmax = _ell_len(cl) - 1
            xvals, _ = gauss_legendre(lmax + 1)
            wd = np.zeros_like(a)
            wd[...] = np.asarray(xi_exact[key]).reshape(a.shape)  # (column j is flat position j, as in the spin-2 placement below)
            wds[key] = replace(cl, ell=xvals, array=np.array(list(wd), dtype=a.dtype))
            continue
        _, lmax, start, n = plan[key]
        xvals, _ = gauss_legendre(lmax + 1)
        wd = np.zeros_like(a)
        if s1 != 0 and s2 != 0:
            r, i = outs[start].T, outs[start + 1].T
            wd[0, 0], wd[1, 1], wd[0, 1], wd[1, 0] = r[1], r[2], i[1], i[2]
        elif s1 != 0 or s2 != 0:
            wd[0], wd[1] = outs[start].T[3], outs[start + 1].T[3]
        else:
            wd = outs[start].T[0]
        wd = np.array(list(wd), dtype=a.dtype)
        wds[key] = replace(cl, ell=xvals, array=wd)
    return wds


def corr2cl(wds, exact_spin=False):
    """Dict of correlation functions -> dict of spectra (transforms.py:286-363); ``exact_spin`` as in ``cl2corr``."""
    L = _lib.load()
    exact = {key: wd for key, wd in wds.items() if exact_spin and _exact_key(wd.spin)}
    b_exact = _exact_columns(corr2cl_columns, exact, _pack_back) if exact else {}
    work, plan = [], []
    for key, wd in wds.items():
        if key in exact:
            continue
        s1, s2 = wd.spin
        lmax = _ell_len(wd) - 1
        a = np.asarray(wd.array)
        z = np.zeros(lmax + 1)
        if s1 != 0 and s2 != 0:
            specs = [np.array([z, a[0, 0], a[1, 1], z]).T, np.array([z, a[0, 1], a[1, 0], z]).T]
        elif s1 != 0 or s2 != 0:
            specs = [np.array([z, z, z, a[0]]).T, np.array([z, z, z, a[1]]).T]
        else:
            specs = [np.array([a, z, z, z]).T]
        plan.append((key, lmax, len(work), len(specs)))
        work.extend((lmax, s) for s in specs)
    outs = [None] * len(work)
    for lm in sorted({w[0] for w in work}):
        ids = [i for i, w in enumerate(work) if w[0] == lm]
        res = _batch(L.hx_corr2cl, [work[i][1] for i in ids], lm)
        for i, r in zip(ids, res):
            outs[i] = r
    plan = {p[0]: p for p in plan}
    cls = {}
    for key, wd in wds.items():
        s1, s2 = wd.spin
        a = np.asarray(wd.array)
        if key in exact:
            lmax = _ell_len(wd) - 1
            b = b_exact[key]
            cl = np.zeros_like(a)
            if s1 != 0 and s2 != 0:
                cl[0, 0], cl[1, 1], cl[0, 1], cl[1, 0] = (b[0] + b[3]) / 2, (b[0] - b[3]) / 2, -(b[1] + b[2]) / 2, (b[1] - b[2]) / 2
            else:
                cl[0], cl[1] = (b[0] + b[1]) / 2, (b[0] - b[1]) / 2
            cls[key] = replace(wd, ell=np.arange(lmax + 1), array=np.array(list(cl), dtype=a.dtype))
            continue
        _, lmax, start, n = plan[key]
        cl = np.zeros_like(a)
        if s1 != 0 and s2 != 0:
            r, i = outs[start].T, outs[start + 1].T
            cl[0, 0], cl[1, 1], cl[0, 1], cl[1, 0] = r[1], r[2], -i[1], i[2]
        elif s1 != 0 or s2 != 0:
            p, m = outs[start].T[3], outs[start + 1].T[3]
            cl[0], cl[1] = (p + m) / 2, (p - m) / 2
        else:
            cl = outs[start].T[0]
        cl = np.array(list(cl), dtype=a.dtype)
        cls[key] = replace(wd, ell=np.arange(lmax + 1), array=cl)
    return cls


# ---- batches of single columns on the matrix unit (hx_xi_cols.hip) -------------------------------------------------------------------
def _is_tensor(a):
    return hasattr(a, "data_ptr")


def _columns_in(a, what):
    """A (ncol, length) float64 operand: a contiguous tensor (host or device) as it is, anything else as a C-contiguous numpy array."""
    if _is_tensor(a):
        import torch

        if a.dtype != torch.float64 or a.dim() != 2 or not a.is_contiguous():
            raise ValueError(f"{what}: tensors must be contiguous float64 of shape (ncol, length)")
        return a
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"{what}: expected shape (ncol, length), got {a.shape}")
    return a


def _columns_out(like, shape, out):
    if out is None and _is_tensor(like):
        import torch

        return torch.empty(shape, dtype=torch.float64, device=like.device)
    return _lib.result_array(shape, out)


def _index(ix, ncol, what):
    ix = np.ascontiguousarray(ix, dtype=np.int32)
    if ix.shape != (ncol,):
        raise ValueError(f"{what}: expected {ncol} entries, got shape {ix.shape}")
    return ix


def _families(families, ncol):
    """(array, entry point suffix): ``families`` of shape (ncol,) are table families, of shape (ncol, 2) pairs (a, b)."""
    fam = np.ascontiguousarray(families, dtype=np.int32)
    if fam.ndim == 2:
        if fam.shape != (ncol, 2):
            raise ValueError(f"families: expected {ncol} pairs (a, b), got shape {fam.shape}")
        return fam, "_spin"
    return _index(fam, ncol, "families"), ""


def cl2corr_columns(a, families, lmax, out=None):
    """xi[c][k] = sum_l (2l + 1) / 4 pi a[c][l] T_f[l][k] at the lmax + 1 Gauss-Legendre nodes for a batch of columns ``a`` (ncol, nl),
    column c tied to table family ``families[c]`` (0: P_l, 1: d^l_22, 2: d^l_2-2, 3: d^l_20; l from 2 for the last three): one FP64 GEMM per
    family against the tables ``cl2corr`` caches.  nl = a.shape[-1] <= lmax + 1 (no zero-padding needed).  numpy arrays or contiguous
    CUDA tensors; a tensor is used in place and the result is a tensor on its device unless ``out`` says otherwise.

    ``families`` of shape (ncol, 2) ties column c to the pair (a, b) = families[c] instead: T_ab[l][k] = d^l_ab(x_k) as
    ``wigner_d_table(lmax, a, b, x)`` gives it, l from max(|a|, |b|), for fields of any spin weight (hx_cl2corr_cols_spin; tables in
    double-double, ``HX_XI_TABLES`` of them cached)."""
    a = _columns_in(a, "cl2corr_columns")
    ncol, nl = a.shape
    fam, suffix = _families(families, ncol)
    out = _columns_out(a, (ncol, int(lmax) + 1), out)
    _lib.ensure_init()
    fn = getattr(_lib.load(), "hx_cl2corr_cols" + suffix)
    _lib.check(fn(int(lmax), int(nl), int(ncol), _lib.ptr(fam), _lib.ptr(a), _lib.ptr(out)))
    return out


def corr2cl_columns(xi, families, lmax, nl=None, out=None):
    """b[c][l] = 2 pi sum_k w_k xi[c][k] T_f[l][k] for l < nl (default lmax + 1; 0 below l = 2 for families 1 .. 3) of a batch of
    columns ``xi`` (ncol, lmax + 1): the way back of ``cl2corr_columns``, (ncol, nl).  ``families`` of shape (ncol, 2): pairs (a, b), 0
    below max(|a|, |b|)."""
    xi = _columns_in(xi, "corr2cl_columns")
    ncol = xi.shape[0]
    if xi.shape[1] != int(lmax) + 1:
        raise ValueError(f"corr2cl_columns: xi has {xi.shape[1]} nodes, lmax + 1 = {int(lmax) + 1}")
    nl = int(lmax) + 1 if nl is None else int(nl)
    fam, suffix = _families(families, ncol)
    out = _columns_out(xi, (ncol, nl), out)
    _lib.ensure_init()
    fn = getattr(_lib.load(), "hx_corr2cl_cols" + suffix)
    _lib.check(fn(int(lmax), nl, int(ncol), _lib.ptr(fam), _lib.ptr(xi), _lib.ptr(out)))
    return out


def xi_ratio(xi_d, xi_num, num_col, ndamp, xi_den=None, den_col=None, x0=-5.0, k=50.0, out=None):
    """out[c] = xi_d[c] / D^ndamp[c](alpha_c), alpha_c = xi_num[num_col[c]] (/ xi_den[den_col[c]] where den_col[c] >= 0),
    D(alpha) = alpha (1 + exp(-k (log10 |alpha| - x0))): the damped mask division of ``naturalspice`` for a batch of columns, element-wise
    in plain IEEE arithmetic (hx_xi_ratio).  ``out`` may be ``xi_d`` itself."""
    xi_d = _columns_in(xi_d, "xi_ratio")
    xi_num = _columns_in(xi_num, "xi_ratio")
    ncol, n = xi_d.shape
    num_col = _index(num_col, ncol, "num_col")
    ndamp = _index(ndamp, ncol, "ndamp")
    if xi_num.shape[1] != n or (num_col.size and int(num_col.max()) >= xi_num.shape[0]):
        raise ValueError("xi_ratio: num_col points outside xi_num, or the node counts differ")
    if xi_den is not None:
        xi_den = _columns_in(xi_den, "xi_ratio")
        den_col = _index(den_col, ncol, "den_col")
        if xi_den.shape[1] != n or int(den_col.max()) >= xi_den.shape[0]:
            raise ValueError("xi_ratio: den_col points outside xi_den, or the node counts differ")
    else:
        den_col = None
    out = _columns_out(xi_d, (ncol, n), out)
    _lib.ensure_init()
    _lib.check(_lib.load().hx_xi_ratio(int(n), int(ncol), _lib.ptr(xi_d), _lib.ptr(xi_num), _lib.ptr(num_col), _lib.ptr(xi_den), _lib.ptr(den_col),
                                       _lib.ptr(ndamp), float(x0), float(k), _lib.ptr(out)))
    return out
