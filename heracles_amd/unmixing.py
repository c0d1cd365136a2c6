"""NaturalSpice real-space unmixing on top of the GPU Cl <-> xi transforms.

Mirrors heracles/unmixing.py:32-102.  The reference regularises the mask correlation
function IN PLACE through the object returned by ``get_cl`` (unmixing.py:99), so a mask
pair shared by two data keys is regularised twice; that behaviour is kept.
"""

from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from . import transforms as _tr
from .transforms import cl2corr, corr2cl, gauss_legendre


def logistic(x, x0=-2, k=50):
    return 1.0 + np.exp(-k * (x - x0))


def _get_cl(key, cls):
    """Symmetric lookup with spin/axis swap (heracles/utils.py:28-52)."""
    if key in cls:
        return cls[key]
    a, b, i, j = key
    sym = (b, a, j, i)
    if sym not in cls:
        raise KeyError(f"Key {key} not found in Cls.")
    arr = cls[sym].array
    s1, s2 = cls[sym].spin
    if s1 != 0 and s2 != 0:
        arr = np.transpose(arr, axes=(1, 0, 2))
    return replace(cls[sym], array=arr, spin=(s2, s1))


def _pad(d, n):
    """Zero-pad / truncate spectra to n multipoles; equals binned(d, arange(0, n+1)) of
    heracles/unmixing.py:53,63 for unit-width bins."""
    out = {}
    for key, r in d.items():
        a = np.asarray(r.array)
        m = a.shape[-1]
        if m >= n:
            b = np.array(a[..., :n])
        else:
            b = np.concatenate([a, np.zeros(a.shape[:-1] + (n - m,), dtype=a.dtype)], axis=-1)
        out[key] = replace(r, array=b, ell=np.arange(n), lower=np.arange(n), upper=np.arange(1, n + 1),
                           weight=np.ones(n))
    return out


def _cutoff_exponent(wm, theta_max):
    """log10 of the mask correlation below which it is damped: 1e-5, or its value at the Gauss-Legendre node closest
    to ``theta_max`` degrees in the first mask spectrum (heracles/unmixing.py:83-91)."""
    if theta_max is None:
        return -5
    first = next(iter(wm.values()))
    nodes, _ = gauss_legendre(first.shape[first.axis[0]])
    nearest = np.abs(np.degrees(np.arccos(nodes)) - theta_max).argmin()
    return np.log10(abs(first[nearest]))


def _damp_in_place(xi_mask, x0):
    """xi_m <- xi_m (1 + exp(-50 (log10 |xi_m| - x0))), written through to the caller's array: the reference modifies
    the object its lookup returns (heracles/unmixing.py:99), so a mask pair shared by two data keys is damped twice."""
    xi_mask *= logistic(np.log10(abs(xi_mask)), x0=x0)
    return xi_mask


def _naturalspice(wd, wm, fields, theta_max=None):
    """xi_d / damped xi_m for every data key (a, b, i, j) with the masks of fields a and b (heracles/unmixing.py:66-102)."""
    mask_of = {name: f.mask for name, f in fields.items() if f.mask is not None}
    x0 = _cutoff_exponent(wm, theta_max)

    def corrected(key):
        a, b, i, j = key
        xi_mask = _damp_in_place(_get_cl((mask_of[a], mask_of[b], i, j), wm).array, x0)
        return replace(wd[key], array=wd[key].array / xi_mask)

    return {key: corrected(key) for key in wd}


def naturalspice(d, m, fields, theta_max=None, exact_spin=False):
    """Natural unmixing of data spectra d by mask spectra m (heracles/unmixing.py:36-64): both go to correlation
    functions on the mask's band limit, the ratio comes back and is cut to the data's band limit.  ``exact_spin``: keys with a spin
    outside {0, 2} are transformed on the Wigner functions of their own spins instead of "like spin 2" (``transforms.cl2corr``)."""
    def band_limit(spectra):
        first = next(iter(spectra.values()))
        return first.shape[first.axis[0]]

    n_data, n_mask = band_limit(d), band_limit(m)
    ratio = _naturalspice(cl2corr(_pad(d, n_mask), exact_spin=exact_spin), cl2corr(m, exact_spin=exact_spin), fields, theta_max=theta_max)
    return _pad(corr2cl(ratio, exact_spin=exact_spin), n_data)


# ---- the same pipeline for many samples at once: columns on the matrix unit ----------------------------------------------------------
# A spectrum of spin (s1, s2) is 1 (0 x 0), 2 (0 x 2) or 4 (2 x 2) COLUMNS, each tied to one Wigner table (hx_cl2corr_cols): column j is
# what the dict driver cl2corr puts at flat position j of the key's correlation array, so that the division by the mask's array is a
# division column by column.  The combinations either side are the dict drivers' (transforms.cl2corr / corr2cl):
#   0 x 2: a0 + a1, a0 - a1 on d20;  back (b0 + b1) / 2, (b0 - b1) / 2
#   2 x 2: a00 + a11, a10 - a01 on d22; -a01 - a10, a00 - a11 on d2-2;  back cl00, cl11 = (b0 +- b3) / 2, cl01 = -(b1 + b2) / 2, cl10 = (b1 - b2) / 2
# With exact_spin a column is tied to a PAIR (a, b) instead (hx_cl2corr_cols_spin; transforms.spin_pairs): (s, 0) for the two columns of
# 0 x s, (s1, s2), (s1, s2), (s1, -s2), (s1, -s2) for the four of s1 x s2, same combinations.  Keys of spins {0, 2} keep their family
# beside their pair (``codes``) and stay on the family path, so that they do not change a bit.
_FAMILIES = {1: (0,), 2: (3, 3), 4: (1, 1, 2, 2)}


def _ncols(spin):
    s1, s2 = spin
    return 4 if (s1 != 0 and s2 != 0) else 2 if (s1 != 0 or s2 != 0) else 1


def _shape_of(spin):
    return {1: (), 2: (2,), 4: (2, 2)}[_ncols(spin)]


def _pack(array, spin):
    """(ncols, nl) columns of a spectrum array (..., nl)."""
    a = np.asarray(array, dtype=np.float64)
    n = _ncols(spin)
    if a.shape[:-1] != _shape_of(spin):
        raise ValueError(f"a spectrum of spin {spin} has shape {_shape_of(spin)} + (nl,), got {a.shape}")
    if n == 1:
        return a[None]
    if n == 2:
        return np.stack([a[0] + a[1], a[0] - a[1]])
    return np.stack([a[0, 0] + a[1, 1], -a[0, 1] + a[1, 0], -a[0, 1] - a[1, 0], a[0, 0] - a[1, 1]])


def _unpack(b, spin):
    """Spectrum array (..., nl) of the (ncols, nl) columns that came back."""
    n = _ncols(spin)
    if n == 1:
        return np.array(b[0])
    if n == 2:
        return np.stack([(b[0] + b[1]) / 2, (b[0] - b[1]) / 2])
    return np.stack([np.stack([(b[0] + b[3]) / 2, -(b[1] + b[2]) / 2]), np.stack([(b[1] - b[2]) / 2, (b[0] - b[3]) / 2])])


@dataclass
class SpicePlan:
    """Column layout of one sample: ``columns[key] = (start, count)`` in the data batch, ``mask_key[key]`` the mask key as it is in the
    mask dict, ``families`` per data column, the same for the
    mask spectra (``mask_columns``, ``mask_families``), ``mask_col[c]`` the mask column data column c divides by and ``ndamp[c]`` how
    often that mask has been damped when it does (the reference damps the looked-up mask in place, heracles/unmixing.py:99: the n-th
    data key that looks a mask pair up divides by its n-fold damping)."""

    columns: dict
    mask_key: dict
    families: np.ndarray
    mask_columns: dict
    mask_families: np.ndarray
    mask_col: np.ndarray
    ndamp: np.ndarray
    #: set where ``families`` / ``mask_families`` hold pairs (ncol, 2) (``spice_plan(exact_spin=True)`` with a spin outside {0, 2}): the
    #: family of every column that stays on the family path (keys of spins {0, 2}), -1 for the columns that run on their pair
    codes: np.ndarray | None = None
    mask_codes: np.ndarray | None = None

    @property
    def ncol(self):
        return len(self.families)

    @property
    def ncol_mask(self):
        return len(self.mask_families)


def _column_tables(spins, exact_spin):
    """(families, codes) of the columns of ``spins`` ({key: spin}, dict order): family codes and None, or -- with ``exact_spin`` and a
    spin outside {0, 2} among them -- pairs (ncol, 2) and the family codes of the columns that keep theirs (-1: none)."""
    as_i32 = lambda v: np.asarray(v, dtype=np.int32)  # noqa: E731
    fam = [f for spin in spins.values() for f in _FAMILIES[_ncols(spin)]]
    if not (exact_spin and any(_tr._exact_key(spin) for spin in spins.values())):
        return as_i32(fam), None
    pairs = [p for spin in spins.values() for p in _tr.spin_pairs(spin)]
    exact = [_tr._exact_key(spin) for spin in spins.values() for _ in range(_ncols(spin))]
    return as_i32(pairs).reshape(-1, 2), np.where(exact, -1, as_i32(fam)).astype(np.int32)


def spice_plan(d_spins, m_spins, fields, exact_spin=False):
    """The plan of ``naturalspice`` for data keys ``d_spins`` ({key: spin}, in dict order) and mask keys ``m_spins`` with the masks of
    ``fields``: pure host logic.  The mask of data key (a, b, i, j) is (mask_a, mask_b, i, j), found as ``_get_cl`` finds it (also as
    (mask_b, mask_a, j, i), then with its two spin-2 axes swapped); KeyError if neither is there.

    ``exact_spin``: where a data (mask) key has a spin outside {0, 2}, ``families`` (``mask_families``) are pairs (ncol, 2) and ``codes``
    (``mask_codes``) say which columns stay on the family path; a plan of spins {0, 2} alone is the same plan with or without it."""
    mask_of = {name: f.mask for name, f in fields.items() if f.mask is not None}
    mask_columns, c = {}, 0
    for mk, spin in m_spins.items():
        n = _ncols(spin)
        mask_columns[mk] = (c, n)
        c += n
    columns, mask_key, mask_col, ndamp, uses, c = {}, {}, [], [], {}, 0
    for key, spin in d_spins.items():
        a, b, i, j = key
        mk = (mask_of[a], mask_of[b], i, j)
        swapped = mk not in m_spins
        if swapped:
            if (mk[1], mk[0], j, i) not in m_spins:
                raise KeyError(f"Key {mk} not found in Cls.")
            mk = (mk[1], mk[0], j, i)
        start, nm = mask_columns[mk]
        idx = start + np.arange(nm).reshape(_shape_of(m_spins[mk]))
        if swapped and nm == 4:
            idx = idx.T
        n = _ncols(spin)
        uses[mk] = uses.get(mk, 0) + 1
        columns[key] = (c, n)
        mask_key[key] = mk
        mask_col.extend(np.broadcast_to(idx, _shape_of(spin)).ravel().tolist())  # (numpy's broadcast of data array / mask array)
        ndamp.extend([uses[mk]] * n)
        c += n
    as_i32 = lambda v: np.asarray(v, dtype=np.int32)  # noqa: E731
    fam, codes = _column_tables(d_spins, exact_spin)
    mfam, mcodes = _column_tables(m_spins, exact_spin)
    return SpicePlan(columns, mask_key, fam, mask_columns, mfam, as_i32(mask_col), as_i32(ndamp), codes, mcodes)


def _gpu_ops():
    """forward / ratio / back on the device: spectra go up as numpy arrays, correlation functions stay in HBM, spectra come back."""
    import torch

    from . import _lib

    dev = torch.device("cuda", _lib.device())

    def forward(a, families, lmax):
        return _tr.cl2corr_columns(a, families, lmax, out=torch.empty((a.shape[0], lmax + 1), dtype=torch.float64, device=dev))

    def ratio(xi_d, xi_num, num_col, ndamp, xi_den, den_col, x0):
        return _tr.xi_ratio(xi_d, xi_num, num_col, ndamp, xi_den=xi_den, den_col=den_col, x0=x0, out=xi_d)

    def back(xi, families, lmax, nl):
        return _tr.corr2cl_columns(xi, families, lmax, nl=nl, out=np.empty((xi.shape[0], nl)))

    return forward, ratio, back


def _tile(f, ns):
    return np.tile(f, ns) if f.ndim == 1 else np.tile(f, (ns, 1))


def _rows(x, idx):
    if _tr._is_tensor(x):
        import torch

        return x.index_select(0, torch.as_tensor(idx, dtype=torch.int64, device=x.device))
    return np.ascontiguousarray(x[idx])


def _transform(op, x, fam, codes, *args):
    """``op(x, fam, *args)`` (forward or back) over the columns x.  Where ``fam`` holds pairs and ``codes`` names columns that keep
    their family, those go through ``op`` with their families and the others with their pairs, two calls, and the rows are put back in
    place: a column's result does not depend on its batch, so the split costs copies and changes no bit."""
    if codes is None or not (codes >= 0).any():
        return op(x, fam, *args)
    keep, exact = np.flatnonzero(codes >= 0), np.flatnonzero(codes < 0)
    parts = [(keep, op(_rows(x, keep), np.ascontiguousarray(codes[keep]), *args)), (exact, op(_rows(x, exact), np.ascontiguousarray(fam[exact]), *args))]
    first = parts[0][1]
    if _tr._is_tensor(first):
        import torch

        out = torch.empty((len(codes), first.shape[1]), dtype=first.dtype, device=first.device)
        for idx, r in parts:
            out.index_copy_(0, torch.as_tensor(idx, dtype=torch.int64, device=first.device), r)
        return out
    out = np.empty((len(codes), first.shape[1]))
    for idx, r in parts:
        out[idx] = r
    return out


def _hbm_budget():
    from .covariance import _hbm_budget as budget

    return budget()


def run_spice_plan(plan, data, num, lmax, *, den=None, x0=-5, num_per_sample=False, max_columns=None, ops=None):
    """Run ``plan`` on S samples: ``data`` (S, plan.ncol, nl) columns of the data spectra, ``num`` the columns of the mask spectra at
    lmax + 1 multipoles -- (plan.ncol_mask, lmax + 1) shared by all samples, or (S, plan.ncol_mask, lmax + 1) with ``num_per_sample`` --
    and ``den`` (plan.ncol_mask, lmax + 1) the shared spectra the mask correlation is divided by first (or None).  ``x0``: the damping
    exponent, or a function of the shared mask correlation functions that returns it.  Returns (S, plan.ncol, nl): the spectra of
    xi_data / damped xi_mask, cut at the data's band limit.

    ``ops`` = (forward(a, families, lmax) -- ``families`` (ncol,) family codes or (ncol, 2) pairs, as the plan has them --, ratio(xi_d, xi_num, num_col, ndamp, xi_den, den_col, x0), back(xi, families, lmax, nl));
    the default runs them on the GPU.  Samples are processed in chunks of at most ``max_columns`` data columns (default: what fits
    half of the free HBM); a column's result does not depend on its batch, so the chunking does not change a bit."""
    forward, ratio, back = ops if ops is not None else _gpu_ops()
    data = np.ascontiguousarray(data, dtype=np.float64)
    num = np.ascontiguousarray(num, dtype=np.float64)
    S, ncol, nl = data.shape
    n, ncm = lmax + 1, plan.ncol_mask
    if ncol != plan.ncol or num.shape[-2:] != (ncm, n) or (num.ndim == 3) != bool(num_per_sample):
        raise ValueError("run_spice_plan: the columns do not match the plan")
    xi_den = _transform(forward, np.ascontiguousarray(den, dtype=np.float64), plan.mask_families, plan.mask_codes, lmax) if den is not None else None
    xi_num = None if num_per_sample else _transform(forward, num, plan.mask_families, plan.mask_codes, lmax)
    if callable(x0):
        x0 = x0(xi_num)
    if max_columns is None:
        free = _hbm_budget()
        per_sample = 8 * (ncol * (2 * nl + 2 * n) + (2 * n * ncm if num_per_sample else 0))
        step = S if free is None else max(1, int(0.5 * free // per_sample))
    else:
        step = max(1, int(max_columns) // ncol)
    out = np.empty((S, ncol, nl))
    for s0 in range(0, S, step):
        s1 = min(S, s0 + step)
        ns = s1 - s0
        codes = None if plan.codes is None else np.tile(plan.codes, ns)
        xi_d = _transform(forward, data[s0:s1].reshape(ns * ncol, nl), _tile(plan.families, ns), codes, lmax)
        num_col = np.tile(plan.mask_col, ns)
        if num_per_sample:
            xi_n = _transform(forward, num[s0:s1].reshape(ns * ncm, n), _tile(plan.mask_families, ns), None if plan.mask_codes is None else np.tile(plan.mask_codes, ns), lmax)
            num_col = num_col + np.repeat(np.arange(ns, dtype=np.int32) * ncm, ncol)
        else:
            xi_n = xi_num
        xi_r = ratio(xi_d, xi_n, num_col, np.tile(plan.ndamp, ns), xi_den, np.tile(plan.mask_col, ns) if xi_den is not None else None, x0)
        out[s0:s1] = np.asarray(_transform(back, xi_r, _tile(plan.families, ns), codes, lmax, nl)).reshape(ns, ncol, nl)
    return out


def _band_limit(spectra):
    first = next(iter(spectra.values()))
    return first.shape[first.axis[0]]


def _result_dtype(a, n, mask_dtype):
    """dtype of the array the dict drivers end with for a spectrum array ``a`` padded to n multipoles and divided by a mask array of
    ``mask_dtype``: whether dtype metadata survives is decided by numpy in ``_pad``'s concatenate and in the division; every later step
    keeps the dtype it is given."""
    dt = a.dtype if a.shape[-1] >= n else np.concatenate([a[..., :1], np.zeros(a.shape[:-1] + (1,), dtype=a.dtype)], axis=-1).dtype
    return (np.ones(1, dtype=dt) / np.ones(1, dtype=mask_dtype)).dtype


def _pack_spectra(spectra, n):
    """(ncol, n) columns of all spectra of a dict in dict order, zero-padded or cut to n multipoles."""
    cols = []
    for r in spectra.values():
        c = _pack(r.array, r.spin)
        if c.shape[-1] >= n:
            c = c[:, :n]
        else:
            c = np.concatenate([c, np.zeros((c.shape[0], n - c.shape[-1]))], axis=-1)
        cols.append(c)
    return np.concatenate(cols)


def _dress(plan, like, b, n_data, n_mask, mask_dtype):
    """The dict ``_pad(corr2cl(...), n_data)`` returns, from the columns b (plan.ncol, n_data) of one sample; ``mask_dtype(mask key)``:
    the dtype of the array the data's correlation function was divided by."""
    out = {}
    for key, (start, count) in plan.columns.items():
        r = like[key]
        a = np.asarray(r.array)
        cl = _unpack(b[start : start + count], r.spin)
        arr = np.empty(cl.shape, dtype=_result_dtype(a, n_mask, mask_dtype(plan.mask_key[key])))  # (np.array(cl, dtype=...) keeps cl's own dtype where no cast is needed)
        arr[...] = cl
        out[key] = replace(r, array=arr, ell=np.arange(n_data), lower=np.arange(n_data), upper=np.arange(1, n_data + 1), weight=np.ones(n_data))
    return out


def _check_samples(samples):
    ids = list(samples)
    if not ids:
        raise ValueError("no samples")
    first = samples[ids[0]]
    n = _band_limit(first)
    for i in ids:
        if list(samples[i]) != list(first) or any(_band_limit({k: r}) != n or tuple(r.spin) != tuple(first[k].spin) for k, r in samples[i].items()):
            raise ValueError("all samples must have the same keys, spins and band limit")
    return ids, first, n


def naturalspice_batch(samples, m, fields, theta_max=None, max_columns=None, ops=None, exact_spin=False):
    """``{id: naturalspice(samples[id], fresh copy of m, fields, theta_max)}`` for samples ``{id: {key: Result}}`` that share keys and
    band limit and one mask dict ``m``: one forward GEMM over the data columns of all samples, one over the mask columns, one ratio launch
    and one GEMM back that stops at the data's band limit (in chunks of ``max_columns`` data columns when they do not fit the HBM
    together).  ``m`` is not modified: every sample sees the undamped masks.  ``exact_spin`` as in ``naturalspice``."""
    ids, first, n_data = _check_samples(samples)
    n_mask = _band_limit(m)
    if n_data > n_mask:
        raise ValueError("the masks' band limit is below the data's")
    plan = spice_plan({k: tuple(r.spin) for k, r in first.items()}, {k: tuple(r.spin) for k, r in m.items()}, fields, exact_spin=exact_spin)
    x0 = -5
    if theta_max is not None:
        if _ncols(next(iter(m.values())).spin) != 1:
            raise NotImplementedError("theta_max reads the first mask's correlation function at one node: that mask must be scalar")
        nodes, _ = gauss_legendre(n_mask)
        nearest = int(np.abs(np.degrees(np.arccos(nodes)) - theta_max).argmin())
        x0 = lambda xi_mask: np.log10(abs(float(xi_mask[0][nearest])))  # noqa: E731  (_cutoff_exponent: the one value the reference reads)
    data = np.stack([_pack_spectra(samples[i], n_data) for i in ids])
    b = run_spice_plan(plan, data, _pack_spectra(m, n_mask), n_mask - 1, x0=x0, max_columns=max_columns, ops=ops)
    return {i: _dress(plan, samples[i], b[s], n_data, n_mask, lambda mk: np.asarray(m[mk].array).dtype) for s, i in enumerate(ids)}
