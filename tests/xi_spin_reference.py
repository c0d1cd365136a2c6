"""Ground truth of the Cl <-> xi transforms of columns tied to ANY pair (a, b) (numpy only, no GPU, no oracle): d^l_{ab}(x) in
np.longdouble by the three-term recursion of tests/corr_reference.py::recursion_rows, generalised to any pair, from the closed-form seed
at l0 = max(|a|, |b|):
    (A, B) = the pair brought to A >= |B|, A >= 0 by d_{ab} = (-1)^{a-b} d_{ba} = d_{-b,-a},  s = the sign that took it there,
    d^A_{AB}(x) = sqrt((2A)! / ((A+B)! (A-B)!)) ((1+x)/2)^{(A+B)/2} ((1-x)/2)^{(A-B)/2},      d^{l0}_{ab} = s d^A_{AB}
(the sign convention of corr_reference's four families and of heracles_amd.wigner_d_table: d^2_{20} = +sqrt(6)/4 (1 - x^2)).  The sums
are those of hx_cl2corr_cols_spin / hx_corr2cl_cols_spin:
    xi[c][k] = sum_{l0 <= l < nl} (2l + 1) / 4 pi a[c][l] d^l_{ab}(x_k),    b[c][l] = 2 pi sum_k w_k xi[c][k] d^l_{ab}(x_k)  (0 below l0).
Tables are (lmax + 1, n) long doubles: for the small sizes of the tests only (corr_reference streams over l for the large ones)."""

import math

import numpy as np

from corr_reference import LD, PI_LD


def normal_pair(a, b):
    """(A, B, sign) with A >= |B| and d_{ab} = sign d_{AB}."""
    flip = -1 if (a - b) & 1 else 1
    if abs(a) >= abs(b):
        return (a, b, 1) if a >= 0 else (-a, -b, flip)
    return (b, a, flip) if b > 0 else (-b, -a, 1)


def seed(a, b, x):
    """d^{l0}_{ab}(x), l0 = max(|a|, |b|), long double; x long double array."""
    A, B, sign = normal_pair(a, b)
    pp, pm = A + B, A - B
    hp, hm = (1 + x) / 2, (1 - x) / 2
    v = hp ** (pp // 2) * hm ** (pm // 2)
    if pp & 1:  # (pp and pm are odd together)
        v = v * np.sqrt(hp * hm)
    return sign * np.sqrt(LD(math.comb(2 * A, pp))) * v  # (the binomial is below 2^64 up to A = 32: exact in the 64-bit mantissa)


def wigner_table(lmax, a, b, x):
    """d^l_{ab}(x_k), l = 0 .. lmax: long double (lmax + 1, len(x)), zero below max(|a|, |b|).  x: float64 nodes, or long double ones."""
    x = np.asarray(x)
    x = x.astype(LD) if x.dtype != LD else x
    out = np.zeros((lmax + 1, len(x)), dtype=LD)
    l0 = max(abs(a), abs(b))
    if l0 > lmax:
        return out
    out[l0] = seed(a, b, x)
    for k in range(l0, lmax):  # step k -> l = k + 1, coefficients as in corr_reference.recursion_rows
        l = k + 1
        if k == 0:
            out[1] = x * out[0]
            continue
        den = LD(k) * np.sqrt(LD(l * l - a * a) * LD(l * l - b * b))
        c1 = LD(2 * k + 1) * (LD(k * l) * x - LD(a * b)) / den
        c2 = LD(l) * np.sqrt(LD(k * k - a * a) * LD(k * k - b * b)) / den
        out[l] = c1 * out[k] - c2 * out[k - 1]  # (c2 = 0 at k = l0, and the row below l0 is zero)
    return out


class Tables:
    """Tables by pair at fixed nodes, built once each."""

    def __init__(self, lmax, x, w):
        self.lmax, self.x, self.w = lmax, np.asarray(x), np.asarray(w)
        self._t = {}

    def __call__(self, a, b):
        key = (int(a), int(b))
        if key not in self._t:
            self._t[key] = wigner_table(self.lmax, key[0], key[1], self.x)
        return self._t[key]

    def forward(self, cols, pairs):
        """xi (ncol, n) long double of columns (ncol, nl) on their pairs."""
        cols = np.asarray(cols, dtype=np.float64).astype(LD)
        nl = cols.shape[1]
        f = (2 * np.arange(nl).astype(LD) + 1) / (4 * PI_LD)
        out = np.zeros((len(cols), len(self.x)), dtype=LD)
        for c, (a, b) in enumerate(pairs):
            l0 = max(abs(a), abs(b))
            if l0 < nl:
                out[c] = (f[l0:] * cols[c, l0:]) @ self(a, b)[l0:nl]
        return out

    def back(self, xi, pairs, nl):
        """b (ncol, nl) long double of correlation columns (ncol, n)."""
        xw = np.asarray(xi, dtype=np.float64).astype(LD) * self.w.astype(LD)
        out = np.zeros((len(xw), nl), dtype=LD)
        for c, (a, b) in enumerate(pairs):
            l0 = max(abs(a), abs(b))
            if l0 < nl:
                out[c, l0:] = 2 * PI_LD * (self(a, b)[l0:nl] @ xw[c])
        return out


def forward_bound(cols, pairs):
    """(16 eps + 1e-13) sum_{l >= l0} |(2l + 1) / 4 pi a_l| per column: the rounding floor of corr_reference.cl2corr_floor plus the 1e-13
    at which tests/test_gpu_mixmat_spin.py pins the tables (|d| <= 1)."""
    cols = np.abs(np.asarray(cols, dtype=np.float64))
    f = (2.0 * np.arange(cols.shape[1]) + 1.0) / (4.0 * np.pi)
    l0 = np.array([max(abs(a), abs(b)) for a, b in pairs])
    live = np.arange(cols.shape[1])[None, :] >= l0[:, None]
    return (16 * np.finfo(np.float64).eps + 1e-13) * (f * cols * live).sum(axis=1)


def back_bound(xi, w):
    """(16 eps + 1e-13) 2 pi sum_k w_k |xi_k| per column."""
    return (16 * np.finfo(np.float64).eps + 1e-13) * 2 * np.pi * (np.abs(np.asarray(xi)) * np.asarray(w)).sum(axis=1)
