"""Direct-sum reference of the point transform for a field of any spin weight s >= 1, in np.longdouble.

For value rows read in pairs (Q, U) at points (theta_p, phi_p):

    (+s)a_lm = sum_p (Q_p + i U_p) conj((+s)Y_lm(theta_p, phi_p))
    (-s)a_lm = sum_p (Q_p - i U_p) conj((-s)Y_lm(theta_p, phi_p))
    E_lm = -((+s)a_lm + (-1)^s (-s)a_lm) / 2
    B_lm = i ((+s)a_lm - (-1)^s (-s)a_lm) / 2        for l >= max(m, s), m >= 0;  E_lm = B_lm = 0 for l < s

(the convention of HEALPix's map2alm_spin / libsharp; at s = 2 it is ``oracle.points2alm(spin=2)``).  tY_lm(theta, phi) =
tlambda_lm(theta) e^{i m phi} with a real tlambda_lm, evaluated for the signed weight t = +-s from

* seeds at l0 = max(m, s), in log form, with sh = sin(theta / 2), ch = cos(theta / 2):
    m >= s:  tlambda_mm = (-1)^m sqrt((2m+1)/4pi (2m)!/((m+s)!(m-s)!)) sh^(m+t) ch^(m-t)
    m <  s:  K = sqrt((2s+1)/4pi (2s)!/((s+m)!(s-m)!)),  (+s)lambda_sm = (-1)^m K sh^(s+m) ch^(s-m),
             (-s)lambda_sm = (-1)^s K sh^(s-m) ch^(s+m)
* the normalised Wigner-d step of the oracle's ``wd_coef(l, m, n = -t)``:
    lambda_{l+1} = (c1x x + c1c) lambda_l - c2 lambda_{l-1},  x = cos(theta).

np.longdouble has a 64-bit mantissa and a 2^+-16384 range: sin^m(theta) stays a normal number down to 1e-4932, so no scaling
is needed.  tests/test_spin_reference.py ties this file to ``helpers.sYlm`` and to the oracle before any device result is
compared with it.
"""

import numpy as np

ld = np.longdouble
_PI = ld("3.141592653589793238462643383279502884")


def _wd_coef(l, m, n):
    """Coefficients of the step l -> l + 1 (oracle/hx_oracle.c: wd_coef), in long double."""
    dl, lp, dm, dn = ld(l), ld(l + 1), ld(m), ld(n)
    den = dl * np.sqrt((lp * lp - dm * dm) * (lp * lp - dn * dn))
    r1 = np.sqrt((2 * dl + 3) / (2 * dl + 1))
    c1x = r1 * (2 * dl + 1) * dl * lp / den
    c1c = -r1 * (2 * dl + 1) * dm * dn / den
    c2 = ld(0)
    if l >= 1:
        r2 = np.sqrt((2 * dl + 3) / (2 * dl - 1))
        c2 = r2 * lp * np.sqrt((dl * dl - dm * dm) * (dl * dl - dn * dn)) / den
    return c1x, c1c, c2


def _log_power(log_base, n):
    """n log(base), with 0 log(0) = 0."""
    if n == 0:
        return np.zeros_like(log_base)
    return ld(n) * log_base


def spin_lambda(t, m, lmax, theta):
    """tlambda_lm(theta) for the signed weight t != 0, l = max(m, |t|) .. lmax: array (lmax - l0 + 1, npoints), long double."""
    s = abs(t)
    theta = np.asarray(theta, dtype=ld)
    x, sh, ch = np.cos(theta), np.sin(theta / 2), np.cos(theta / 2)
    logfact = np.concatenate([[ld(0)], np.cumsum(np.log(np.arange(1, 2 * max(m, s) + 2, dtype=ld)))])
    with np.errstate(divide="ignore"):
        lsh, lch = np.log(sh), np.log(ch)
    l0 = max(m, s)
    if m >= s:
        lognorm = ld(0.5) * (np.log(ld(2 * m + 1) / (4 * _PI)) + logfact[2 * m] - logfact[m + s] - logfact[m - s])
        sign = -1 if m & 1 else 1
        logv = lognorm + _log_power(lsh, m + t) + _log_power(lch, m - t)
    else:
        lognorm = ld(0.5) * (np.log(ld(2 * s + 1) / (4 * _PI)) + logfact[2 * s] - logfact[s + m] - logfact[s - m])
        if t > 0:
            sign = -1 if m & 1 else 1
            logv = lognorm + _log_power(lsh, s + m) + _log_power(lch, s - m)
        else:
            sign = -1 if s & 1 else 1
            logv = lognorm + _log_power(lsh, s - m) + _log_power(lch, s + m)
    cur = ld(sign) * np.exp(logv)
    out = np.empty((max(lmax - l0 + 1, 0),) + theta.shape, dtype=ld)
    if lmax < l0:
        return out
    out[0] = cur
    prev = np.zeros_like(cur)
    for l in range(l0, lmax):
        c1x, c1c, c2 = _wd_coef(l, m, -t)
        prev, cur = cur, (c1x * x + c1c) * cur - c2 * prev
        out[l + 1 - l0] = cur
    return out


def _orders(orders, lmax):
    """All orders 0 .. lmax, or the given ones in ascending order, each once."""
    if orders is None:
        return range(lmax + 1)
    ms = sorted({int(m) for m in orders})
    if ms and (ms[0] < 0 or ms[-1] > lmax):
        raise ValueError("orders: 0 <= m <= lmax")
    return ms


def points2alm_spin(theta, phi, values, lmax, s, orders=None):
    """values (ncomp, npoints), ncomp even, rows (Q, U) -> (E, B) alms (ncomp, nlm) complex128, m-major.  ``orders``: an iterable
    of m; only those orders are computed, the other rows stay zero (a long transform on a sample of m costs what the sample costs)."""
    if s < 1:
        raise ValueError("points2alm_spin: s >= 1")
    values = np.asarray(values, dtype=ld)
    if values.ndim != 2 or values.shape[0] % 2:
        raise ValueError("points2alm_spin: an even number of value rows")
    theta, phi = np.asarray(theta, dtype=ld), np.asarray(phi, dtype=ld)
    nlm = (lmax + 1) * (lmax + 2) // 2
    alm = np.zeros((values.shape[0], nlm), dtype=np.complex128)
    q, u = values[0::2], values[1::2]
    sgn = -1 if s & 1 else 1
    for m in _orders(orders, lmax):
        l0 = max(m, s)
        if l0 > lmax:
            continue
        ph_re, ph_im = np.cos(m * phi), -np.sin(m * phi)  # e^{-i m phi}
        lam_p, lam_m = spin_lambda(+s, m, lmax, theta), spin_lambda(-s, m, lmax, theta)
        # (Q +- iU) e^{-i m phi}: real and imaginary parts, (nfield, npoints)
        pr, pi = q * ph_re - u * ph_im, q * ph_im + u * ph_re
        mr, mi = q * ph_re + u * ph_im, q * ph_im - u * ph_re
        ap_r, ap_i = pr @ lam_p.T, pi @ lam_p.T  # (nfield, nl)
        am_r, am_i = sgn * (mr @ lam_m.T), sgn * (mi @ lam_m.T)
        e_r, e_i = -(ap_r + am_r) / 2, -(ap_i + am_i) / 2
        b_r, b_i = -(ap_i - am_i) / 2, (ap_r - am_r) / 2  # i (x + i y) = -y + i x
        lo = m * (2 * lmax + 1 - m) // 2 + l0
        hi = lo + lmax - l0 + 1
        alm[0::2, lo:hi] = e_r.astype(np.float64) + 1j * e_i.astype(np.float64)
        alm[1::2, lo:hi] = b_r.astype(np.float64) + 1j * b_i.astype(np.float64)
    return alm
