"""numpy restatement of the mask-aware Gaussian covariance of pseudo-Cl: the direct double sum over (l, l') of every
block, nothing shared with the two-stage GPU form.

    Cov_{bb'} = sum_{l in b, l' in b'} w_l w_l' Xi_{ll'} sum_terms Sbar_{ll'} Tbar_{ll'} / (norm_b norm_b'),  Sbar_{ll'} = (S_l + S_l') / 2

and beside it the absolute sum every rounding-error bound of the tests is quoted on,

    A_{bb'} = 1/4 sum |w_l w_l' Xi_{ll'}| sum_terms (|S_l| + |S_l'|) (|T_l| + |T_l'|) / |norm_b norm_b'|.

``Xi`` of a mask-product spectrum W is the oracle's (0,0) mixing matrix with its column factor divided out (``xi_table``)."""

import itertools

import numpy as np

from heracles_amd.covariance import _expand_spin0, bias, get_cl


def xi_table(oracle, w_cl, L):
    """Xi_{ll'} = sum_l'' (2l'' + 1) / (4 pi) W_l'' (l l' l''; 0 0 0)^2 for l, l' <= L: oracle.mixmat(W) / (2l' + 1)."""
    w_cl = np.asarray(w_cl, dtype=float)[: 2 * L + 1]
    return oracle.mixmat(w_cl, L, L, 2 * L) / (2 * np.arange(L + 1) + 1)[None, :]


def _bin_operator(n, plan):
    """(nb, n) weights B[b, l] = w_l for l in b, and norm (nb); plan None: every l its own bin."""
    if plan is None:
        return np.eye(n), np.ones(n)
    B = np.zeros((plan.nbins, n))
    for l in range(n):
        if plan.which[l] >= 0:
            B[plan.which[l], l] = plan.w[l]
    return B, np.asarray(plan.norm, dtype=float)


def block(xi, terms, plan=None):
    """(Cov, A) of one block: ``terms`` is a list of (S, T) spectra pairs (one or two), ``xi`` the (n, n) table."""
    n = xi.shape[0]
    v = np.zeros((n, n))
    va = np.zeros((n, n))
    for S, T in terms:
        S, T = np.asarray(S, dtype=float), np.asarray(T, dtype=float)
        # element (l, l') of the double sum, all at once
        v += xi * (0.5 * (S[:, None] + S[None, :])) * (0.5 * (T[:, None] + T[None, :]))
        va += 0.25 * np.abs(xi) * (np.abs(S)[:, None] + np.abs(S)[None, :]) * (np.abs(T)[:, None] + np.abs(T)[None, :])
    # sum_{l in b, l' in b'} w_l w_l' (.) / (norm_b norm_b') for all (b, b') at once; a bin without members holds 0
    B, norm = _bin_operator(n, plan)
    live = np.abs(B).sum(axis=1) > 0
    den = np.where(np.outer(live, live), np.outer(norm, norm), 1.0)
    cov = np.where(np.outer(live, live), (B @ v @ B.T) / den, 0.0)
    A = np.where(np.outer(live, live), (np.abs(B) @ va @ np.abs(B).T) / np.abs(den), 0.0)
    return cov, A


def bin_sizes(n, plan):
    """Members per bin (unbinned: ones)."""
    if plan is None:
        return np.ones(n, dtype=int)
    return np.bincount(plan.which[plan.which >= 0], minlength=plan.nbins)[: plan.nbins]


def rounding_bound(A, n, plan):
    """4 (n_b n_b' + 16) 2^-53 A: the bound of the kernel tests."""
    nb = bin_sizes(n, plan).astype(float)
    return 4 * (np.outer(nb, nb) + 16) * 2.0**-53 * A


def _units(cls, fields):
    units = []
    for key in cls:
        a, b, i, j = key
        da, db = (1 if fields[a].spin == 0 else 2), (1 if fields[b].spin == 0 else 2)
        for x in range(da):
            for y in range(db):
                units.append(((a, i, x), (b, j, y)))
    return units


def covariance(oracle, cls, mask_cls, fields, plan=None, tables=None, table_error=False):
    """The dense covariance of the data vector of ``cls`` in its order (each key dof-major then l), and its absolute sum:
    every block (all of them, no mirroring) from the formula.  ``mask_cls``: a function (k1, k2, k3, k4) -> W, mask keys
    (mask name, bin).  ``tables`` (a dict) caches the Xi tables by the W array's bytes.
    ``table_error``: a third matrix, the absolute sum with max |M| / (2l' + 1) in place of |Xi_{ll'}|, M = Xi (2l' + 1) the mixing
    matrix of the table: times the relative bound a table build is pinned to, it bounds what the table's error adds to a block."""
    bs = bias(cls)
    full = {key: _replace_array(res, np.asarray(res.array) + bs[key]) for key, res in cls.items()}
    nl = np.asarray(next(iter(cls.values())).array).shape[-1]
    L = nl - 1
    units = _units(cls, fields)
    tables = {} if tables is None else tables

    def spectrum(p, q):
        (a, i, x), (c, k, y) = p, q
        return np.asarray(_expand_spin0(get_cl((a, c, i, k), full)).array)[x, y]

    def mask(p):
        return (fields[p[0]].mask, p[1])

    def xi(p, q, r, s):
        w = np.asarray(mask_cls(mask(p), mask(q), mask(r), mask(s)), dtype=float)
        tag = w.tobytes()
        if tag not in tables:
            tables[tag] = xi_table(oracle, w, L)
        return tables[tag]

    nbe = nl if plan is None else plan.nbins
    N = len(units) * nbe
    cov, A, E = np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, N))
    col = 2 * np.arange(nl) + 1

    def unit_error(x):
        return np.broadcast_to(np.abs(x * col[None, :]).max() / col[None, :], x.shape)

    for (u1, (a, b)), (u2, (c, d)) in itertools.product(enumerate(units), repeat=2):
        here = (slice(u1 * nbe, (u1 + 1) * nbe), slice(u2 * nbe, (u2 + 1) * nbe))
        for x, pair in ((xi(a, c, b, d), (spectrum(a, c), spectrum(b, d))), (xi(a, d, b, c), (spectrum(a, d), spectrum(b, c)))):
            c1, a1 = block(x, [pair], plan)
            cov[here] += c1
            A[here] += a1
            if table_error:
                E[here] += block(unit_error(x), [pair], plan)[1]
    return (cov, A, E) if table_error else (cov, A)


def _replace_array(res, array):
    from dataclasses import replace

    return replace(res, array=array)


# ---- the Monte Carlo check ----------------------------------------------------------------------------------------------------------
MC = dict(nside=16, lmax_field=32, L=24, nreal=600, lmin=4, spectra=((1.0, 0.7), (0.7, 2.0)), mask_lmax=3, niter=3, seed=20191)


def smooth_masks(oracle, nside, count, lmax, seed):
    """``count`` different smooth positive masks of band limit ``lmax``: 1 + 0.3 x a random band-limited field over its largest value."""
    rng = np.random.default_rng(seed)
    nlm = (lmax + 1) * (lmax + 2) // 2
    masks = []
    for _ in range(count):
        alm = rng.standard_normal(nlm) + 1j * rng.standard_normal(nlm)
        alm[: lmax + 1] = alm[: lmax + 1].real  # m = 0
        alm[0] = 0.0
        f = oracle.alm2map(alm[None, :], nside, lmax)[0]
        masks.append(1.0 + 0.3 * f / np.abs(f).max())
    return masks


def white_alms(rng, lmax, cmat):
    """Gaussian alms (ncomp, nlm), m-major, of white spectra with the component covariance ``cmat``."""
    cmat = np.asarray(cmat, dtype=float)
    chol = np.linalg.cholesky(cmat)
    nlm = (lmax + 1) * (lmax + 2) // 2
    z = (rng.standard_normal((len(cmat), nlm)) + 1j * rng.standard_normal((len(cmat), nlm))) / np.sqrt(2.0)
    z[:, : lmax + 1] = rng.standard_normal((len(cmat), lmax + 1))  # m = 0: real, unit variance
    return chol @ z


def z_statistic(samples, analytic, keep):
    """z_ij = (sample - analytic) / sigma_ij, sigma_ij^2 = (C_ii C_jj + C_ij^2) / (n - 1), over the entries ``keep`` of the data vector:
    (max |z|, rms z, mean ratio of the diagonals)."""
    n = samples.shape[0]
    x = samples[:, keep]
    c = analytic[np.ix_(keep, keep)]
    s = np.cov(x, rowvar=False, ddof=1)
    d = np.diag(c)
    sigma = np.sqrt((np.outer(d, d) + c**2) / (n - 1))
    z = (s - c) / sigma
    return float(np.abs(z).max()), float(np.sqrt(np.mean(z**2))), float(np.mean(np.diag(s) / d))
