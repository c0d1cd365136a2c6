"""The numpy restatement of the lognormal mocks: no GPU, no oracle.  Long sums (the Legendre transforms) run in
np.longdouble on the recursion of tests/corr_reference.py; what the kernels define element-wise (log1p / expm1 of an f64 argument, the
map pass) is restated in float64, because there numpy IS the definition.  The matrix repair is restated with numpy.linalg.eigh.

Matrices of spectra are (N, N, nl) symmetric here; tests/synalm_reference.py packs and unpacks them."""

import numpy as np

import corr_reference as cr

LD = np.longdouble
U = 2.0**-53  # unit roundoff of f64


def gl_nodes(n):
    """Gauss-Legendre nodes and weights (float64)."""
    return np.polynomial.legendre.leggauss(int(n))


def legendre_table(lmax, x):
    """P_l(x_k) as a long double array (lmax + 1, len(x))."""
    return np.stack([rows[0] + np.zeros(len(x), dtype=LD) for rows in cr.wigner_rows(int(lmax), x)])


def cl2xi(cl, x, table=None):
    """xi_k = sum_l (2l + 1) / (4 pi) cl_l P_l(x_k) for columns cl (ncol, nl): (xi, A) long double, A the absolute sum of the terms."""
    cl = np.atleast_2d(np.asarray(cl)).astype(LD)
    nl = cl.shape[1]
    P = legendre_table(nl - 1, x) if table is None else table[:nl]
    c = cl * ((2 * np.arange(nl).astype(LD) + 1) / (4 * cr.PI_LD))[None, :]
    return c @ P, np.abs(c) @ np.abs(P)


def xi2cl(xi, x, w, lmax, table=None):
    """b_l = 2 pi sum_k w_k xi_k P_l(x_k), l <= lmax, for columns xi (ncol, len(x)): (b, A) long double."""
    xi = np.atleast_2d(np.asarray(xi)).astype(LD)
    P = legendre_table(lmax, x) if table is None else table[: lmax + 1]
    a = xi * np.asarray(w, dtype=np.float64).astype(LD)[None, :]
    return 2 * cr.PI_LD * (a @ P.T), 2 * cr.PI_LD * (np.abs(a) @ np.abs(P).T)


def xi_forward(xi, factors):
    """The definition of hx_lognormal_xi, direction 0 (float64)."""
    return np.log1p(np.asarray(xi, dtype=np.float64) * np.asarray(factors, dtype=np.float64)[:, None])


def xi_inverse(xi, factors):
    """The definition of hx_lognormal_xi, direction 1 (float64)."""
    return np.asarray(factors, dtype=np.float64)[:, None] * np.expm1(np.asarray(xi, dtype=np.float64))


def convert(C, lam, x, w, inverse=False, c=4.0):
    """The matrix of Gaussian spectra of the targets C (N, N, nl) with shifts lam (N; 0 = Gaussian) on the nodes (x, w) -- or, with
    ``inverse``, the realised spectra of the Gaussian spectra C -- and a rounding bound for a float64 evaluation of the same chain:
    per transform c (terms + 16) 2^-53 A with A the absolute sum of its terms, the first transform's bound and the 2 ulp of the
    element-wise pass carried through the derivative of log1p / expm1 and through the second transform, whose own bound is added.
    Lognormal x lognormal entries are long double; the others are float64 and exact restatements (bound 0).  ValueError if an
    argument of log1p is <= -1.  A long double C is taken as it is (a round trip without the rounding to float64 in between)."""
    C = np.asarray(C)
    C = C if C.dtype == LD else C.astype(np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    n, nl = C.shape[0], C.shape[2]
    out = C.astype(LD)
    bound = np.zeros(C.shape)
    P = legendre_table(max(nl - 1, 0), x)
    for i in range(n):
        for j in range(n):
            if lam[i] > 0 and lam[j] > 0:
                f = lam[i] * lam[j]
                xi, A1 = cl2xi(C[i, j], x, P)
                e1 = c * (nl + 16) * U * A1
                if inverse:
                    y = LD(f) * np.expm1(xi)
                    ey = f * (np.exp(xi) * e1 + 2 * 2 * U * np.abs(np.expm1(xi)))
                else:
                    arg = xi / LD(f)
                    if (arg <= -1).any():
                        raise ValueError(f"pair ({i}, {j}): log1p argument <= -1 at node {int(np.flatnonzero((arg <= -1)[0])[0])}")
                    y = np.log1p(arg)
                    ey = (e1 / f + U * np.abs(arg)) / (1 + arg) + 2 * 2 * U * np.abs(y)
                b, A2 = xi2cl(y, x, w, nl - 1, P)
                carried = 2 * np.pi * (np.asarray(w)[None, :] * ey.astype(np.float64)) @ np.abs(P).T.astype(np.float64)
                out[i, j] = b[0]
                bound[i, j] = (carried + c * (len(x) + 16) * U * A2.astype(np.float64))[0]
            elif lam[i] > 0 or lam[j] > 0:
                s = lam[i] if lam[i] > 0 else lam[j]
                out[i, j] = C[i, j] * s if inverse else C[i, j] / s
    return out, bound


def sigma2(g_l):
    g_l = np.asarray(g_l, dtype=np.float64)
    return float(np.sum((2.0 * np.arange(g_l.size) + 1.0) / (4.0 * np.pi) * g_l))


def maps(g, s2, lam):
    """The definition of hx_lognormal_maps (float64): rows of g with sigma^2 and shift per row."""
    g = np.atleast_2d(np.asarray(g, dtype=np.float64))
    s2, lam = (np.broadcast_to(np.asarray(v, dtype=np.float64), (g.shape[0],))[:, None] for v in (s2, lam))
    return lam * np.expm1(g - 0.5 * s2)


def nearest_psd(C, floor=None):
    """(C', change, repaired) of the matrices C (N, N, nl): per l the components of C_jj > 0 are scaled to unit diagonal, eigenvalues
    below ``floor`` (default 64 N^2 2^-52) raised to it; a matrix with none is returned as it is.  Rows and columns of components with
    C_jj = 0 come back zero; change = max |C' - C| / sqrt(C_ii C_jj) over the kept components, +inf if a non-zero entry beside a zero
    diagonal was removed.  ValueError: a negative or non-finite entry on a diagonal, a non-finite entry anywhere."""
    C = np.asarray(C, dtype=np.float64)
    n, nl = C.shape[0], C.shape[2]
    floor = 64.0 * n * n * 2.0**-52 if floor is None else float(floor)
    bad = [l for l in range(nl) if not np.isfinite(C[:, :, l]).all() or (np.diagonal(C[:, :, l]) < 0).any()]
    if bad:
        raise ValueError(f"l = {bad[0]}")
    out, change, repaired = C.copy(), np.zeros(nl), np.zeros(nl, dtype=bool)
    for l in range(nl):
        M = C[:, :, l]
        d = np.diagonal(M).copy()
        on = d > 0
        dirty = bool((M[~on] != 0).any() or (M[:, ~on] != 0).any())
        k = np.flatnonzero(on)
        if k.size:
            s = np.sqrt(d[k])
            R = M[np.ix_(k, k)] / s[:, None] / s[None, :]
            np.fill_diagonal(R, 1.0)
            lamb, V = np.linalg.eigh(R)
        else:
            lamb = np.ones(0)
        if not dirty and (lamb >= floor).all():
            continue
        repaired[l] = True
        new = np.zeros((n, n))
        if k.size:
            new[np.ix_(k, k)] = (V * np.maximum(lamb, floor)) @ V.T * s[:, None] * s[None, :]
            new = 0.5 * (new + new.T)
            change[l] = np.max(np.abs(new[np.ix_(k, k)] - M[np.ix_(k, k)]) / s[:, None] / s[None, :])
        if dirty:
            change[l] = np.inf
        out[:, :, l] = new
    return out, change, repaired


def smooth_spectra(n, lmax, seed, variances, rho=0.6):
    """Smooth positive-definite targets (N, N, lmax + 1): C^{ij}_l = r_ij sqrt(v_i v_j) s_l with sum_l (2l + 1) / (4 pi) s_l = 1 and
    r a fixed correlation matrix (rho^|i - j|, mixed with a seeded perturbation), so that component i has pixel variance v_i."""
    rng = np.random.default_rng(seed)
    l = np.arange(lmax + 1)
    s = 1.0 / (l + 3.0) ** 2.2
    s[0] = 0.0
    s /= np.sum((2 * l + 1) / (4 * np.pi) * s)
    B = rng.standard_normal((n, n + 3))
    r = B @ B.T
    r = r / np.sqrt(np.outer(np.diagonal(r), np.diagonal(r)))
    base = rho ** np.abs(np.subtract.outer(np.arange(n), np.arange(n)))
    r = 0.7 * base + 0.3 * r
    v = np.asarray(variances, dtype=np.float64)
    return r[:, :, None] * np.sqrt(np.outer(v, v))[:, :, None] * s[None, None, :]


# ---- the statistical case shared by the host experiment and the GPU test of the driver ------------------------------------------------------
STAT_NSIDE, STAT_LMAX, STAT_SEED, STAT_N = 32, 32, (1 << 41) + 2718, 200
STAT_SHIFTS = np.array([1.0, 0.3, 0.0, 0.0])  # two lognormal fields, then E and B of a Gaussian spin-2 field
STAT_ELLS = slice(2, 17)


def statistical_targets():
    """(N, N, lmax + 1) targets: pixel variance of g about 0.1 for both lognormal fields, correlated at 0.6; E correlated with the
    first at 0.5 (0.3 with the second), B on its own; the spin-2 rows vanish below l = 2."""
    l = np.arange(STAT_LMAX + 1)
    s = 1.0 / (l + 3.0) ** 2.2  # (with a monopole: the logarithm lowers G_0 below C_0, and a target without one has no Gaussian field)
    s /= np.sum((2 * l + 1) / (4 * np.pi) * s)
    r = np.array([[1, 0.6, 0.5, 0], [0.6, 1, 0.3, 0], [0.5, 0.3, 1, 0], [0, 0, 0, 1.0]])
    v = np.array([np.expm1(0.1), 0.09 * np.expm1(0.1), 0.05, 0.01])
    C = r[:, :, None] * np.sqrt(np.outer(v, v))[:, :, None] * s[None, None, :]
    C[2:, :, :2] = 0.0
    C[:, 2:, :2] = 0.0
    return C


def z_scores(samples, expected):
    """samples (n, ...) spectra estimates, expected (...): z = (mean - expected) / (sample sigma / sqrt n), and (max |z|, rms z)."""
    n = samples.shape[0]
    z = (samples.mean(axis=0) - expected) / (samples.std(axis=0, ddof=1) / np.sqrt(n))
    return z, float(np.abs(z).max()), float(np.sqrt(np.mean(z**2)))


def indefinite_targets(lmax=16):
    """Three lognormal fields with target correlations 0.99, 0.99, 0.90 at every l and shifts 0.2, 0.1, 0.05 (pixel variance of g about
    0.3): (C (3, 3, lmax + 1), shifts).  The Gaussianised matrices are indefinite (tests/test_lognormal_host.py checks that)."""
    l = np.arange(lmax + 1)
    s = 1.0 / (l + 3.0) ** 2.2
    s /= np.sum((2 * l + 1) / (4 * np.pi) * s)
    lam = np.array([0.2, 0.1, 0.05])
    r = np.array([[1, 0.99, 0.99], [0.99, 1, 0.90], [0.99, 0.90, 1.0]])
    v = lam**2 * np.expm1(0.3)
    return r[:, :, None] * np.sqrt(np.outer(v, v))[:, :, None] * s[None, None, :], lam
