"""Direct-sum reference of the synthesis of a field of any spin weight s >= 1, in np.longdouble: the inverse convention of
tests/spin_reference.py (HEALPix's alm2map_spin / libsharp).

From (E, B) alms (m >= 0, m-major; rows l < s are not read), with sigma = (-1)^s:

    (+s)a_lm = -(E_lm + i B_lm),        (-s)a_lm = -sigma (E_lm - i B_lm)
    P+_m(theta) = sum_l (+s)lambda_lm(theta) (+s)a_lm,    P-_m(theta) = sum_l (-s)lambda_lm(theta) (-s)a_lm     (l >= max(m, s))
    Q_m = (P+_m + P-_m) / 2,            U_m = (P+_m - P-_m) / 2i
    Q(theta, phi) = Re sum_{m >= 0} c_m Q_m e^{i m phi},  U likewise;  c_0 = 1, c_m = 2.

This is Q + iU = sum over l and ALL m of (+s)a_lm (+s)Y_lm with a_{l,-m} = (-1)^m conj(a_lm) for E and B: the orders -m are the
complex conjugates of the orders +m of the other weight, conj(tY_lm) = (-1)^(t+m) (-t)Y_{l,-m}.  tlambda_lm comes from
``spin_reference.spin_lambda``.  tests/test_spin_synthesis_reference.py ties this file to ``helpers.sYlm``, to the oracle at
s = 2 and to ``points2alm_spin`` (adjointness) before any device result is compared with it.
"""

import numpy as np

from spin_reference import _orders, ld, spin_lambda


def alm2points_spin(theta, phi, alm, lmax, s, orders=None):
    """alm (ncomp, nlm) complex, ncomp even, rows (E, B) -> values (ncomp, npoints) float64, rows (Q, U).  ``orders``: an iterable
    of m; only those orders of the alms are read, as if every other row were zero."""
    if s < 1:
        raise ValueError("alm2points_spin: s >= 1")
    alm = np.asarray(alm)
    if alm.ndim != 2 or alm.shape[0] % 2 or alm.shape[1] != (lmax + 1) * (lmax + 2) // 2:
        raise ValueError("alm2points_spin: an even number of rows of nlm coefficients")
    theta, phi = np.asarray(theta, dtype=ld), np.asarray(phi, dtype=ld)
    out = np.zeros((alm.shape[0], theta.size), dtype=ld)
    sgn = -1 if s & 1 else 1
    for m in _orders(orders, lmax):
        l0 = max(m, s)
        if l0 > lmax:
            continue
        lo = m * (2 * lmax + 1 - m) // 2 + l0
        hi = lo + lmax - l0 + 1
        e_r, e_i = alm[0::2, lo:hi].real.astype(ld), alm[0::2, lo:hi].imag.astype(ld)
        b_r, b_i = alm[1::2, lo:hi].real.astype(ld), alm[1::2, lo:hi].imag.astype(ld)
        # a+ = -(E + iB), a- = -sigma (E - iB)
        ap_r, ap_i = -(e_r - b_i), -(e_i + b_r)
        am_r, am_i = -sgn * (e_r + b_i), -sgn * (e_i - b_r)
        lam_p, lam_m = spin_lambda(+s, m, lmax, theta), spin_lambda(-s, m, lmax, theta)  # (nl, npoints)
        pp_r, pp_i = ap_r @ lam_p, ap_i @ lam_p  # (nfield, npoints)
        pm_r, pm_i = am_r @ lam_m, am_i @ lam_m
        q_r, q_i = (pp_r + pm_r) / 2, (pp_i + pm_i) / 2
        u_r, u_i = (pp_i - pm_i) / 2, -(pp_r - pm_r) / 2  # (x + i y) / i = y - i x
        c = ld(1 if m == 0 else 2)
        cs, sn = np.cos(m * phi), np.sin(m * phi)
        out[0::2] += c * (q_r * cs - q_i * sn)
        out[1::2] += c * (u_r * cs - u_i * sn)
    return out.astype(np.float64)


def harmonic_inner(a, b, lmax):
    """sum over l and ALL m of Re(a_lm conj(b_lm)), summed over the rows, for alms of real fields given at m >= 0: the orders
    m > 0 count twice."""
    w = np.full(a.shape[-1], 2.0)
    w[: lmax + 1] = 1.0
    return float(np.sum(w * (a.real * b.real + a.imag * b.imag)))
