"""numpy restatement of the rotation of alms; not a test.  tests/test_rotation_host.py pins it on its own through the
defining identity f'(n) = f(R^-1 n), tests/test_gpu_rotate_alm.py holds ``hx.rotate_alm`` against it.

R = Rz(phi) Ry(theta) Rz(psi) on column vectors, a'_lm = sum_m' exp(-i m phi) d^l_mm'(theta) exp(-i m' psi) a_lm' with
d^l(theta) = exp(-i theta J_y) in the Condon-Shortley basis and a_l,-m = (-1)^m conj(a_lm).  The alm layout is the project's:
m-major, idx(l, m) = m (2 lmax + 1 - m) / 2 + l.

Two restatements.  ``rotate_alm_ref`` takes d^l from ``numpy.linalg.eigh`` of J_y: nothing but the definition, O(l^3) per multipole,
good to about 5e-14 at l = 200 and out of reach beyond a few hundred.  ``rotate_column_ref`` reaches any lmax in long double, one
output column m at a time, from three facts about d^l(theta) = exp(-i theta J_y):

- the highest-weight column: d^j_{j,m'} = (-1)^(j-m') sqrt(C(2j, j+m')) cos^(j+m')(theta/2) sin^(j-m')(theta/2), all real theta;
- the symmetries d^l_{m,m'} = (-1)^(m-m') d^l_{m',m} = d^l_{-m',-m}, which turn that into d^A_{m,+A} = sqrt(C(2A, A+m)) c^(A+m) s^(A-m)
  and d^A_{m,-A} = (-1)^(A+m) sqrt(C(2A, A+m)) c^(A-m) s^(A+m) for A >= |m|;
- the three-term recurrence in l at fixed (m, m'), upwards from l0 = max(|m|, |m'|) where d^(l0-1) = 0 (the stable direction),
    s_(l+1) d^(l+1) = ((2l+1)/l) (l(l+1) x - m m') d^l - ((l+1)/l) s_l d^(l-1),   s_l = sqrt((l^2 - m^2)(l^2 - m'^2)),  x = cos(theta).

The seeds leave the range of a long double (below 1e-4932 at theta = 0.02, l = 6144), so every chain value is (mantissa, integer
exponent); the seeds are running products (binomial ratios, powers of c and s), no logarithm anywhere.  l(l+1) x - m m' is formed
as (l(l+1) - m m') - l(l+1) 2 s^2 for x >= 0 and -(l(l+1) + m m') + l(l+1) 2 c^2 for x < 0: the integer part is exact and the rest
is small where the two cancel, which cos(theta) rounded to 64 bits does not give at small theta (1 - x = 5e-17 at theta = 1e-8).
theta is the double it was given, with no range reduction: the three facts hold for every real theta and cosl / sinl reduce their
argument themselves.

The long-double chains carry the recurrence in differences (``_column_in_differences``): the three-term form loses 1 / sin(theta)
of its accuracy to rounding, in any precision (row norms at lmax 2048, theta = pi - 1e-3 off by 1.2e-15 .. 3.9e-15), the difference
form does not (8e-17, which is the seeds).  The float64 yardstick keeps the three-term form: it models plain FP64 chains."""

import functools

import numpy as np

LD = np.longdouble


def lm_index(lmax):
    """(l, m) of every coefficient in the project's layout."""
    m = np.concatenate([np.full(lmax + 1 - mm, mm) for mm in range(lmax + 1)])
    l = np.concatenate([np.arange(mm, lmax + 1) for mm in range(lmax + 1)])
    return l, m


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def rotation_matrix(psi, theta, phi):
    return rot_z(phi) @ rot_y(theta) @ rot_z(psi)


@functools.lru_cache(maxsize=None)
def _jy_eig(l):
    """Eigen-decomposition of J_y on the basis |l, m>, m = -l .. l: <m + 1| J_y |m> = sqrt((l - m)(l + m + 1)) / (2 i)."""
    m = np.arange(-l, l)
    off = np.sqrt((l - m) * (l + m + 1.0)) / 2j
    jy = np.diag(off, -1) + np.diag(off.conj(), 1)
    return np.linalg.eigh(jy)


def wigner_d(l, theta):
    """d^l(theta)[m + l, m' + l] = <l m| exp(-i theta J_y) |l m'>, real."""
    lam, v = _jy_eig(int(l))
    return ((v * np.exp(-1j * theta * lam)) @ v.conj().T).real


def full_orders(row, l):
    """a_lm for m = -l .. l from the stored m = 0 .. l."""
    m = np.arange(1, l + 1)
    return np.concatenate([((-1.0) ** m * row[1:].conj())[::-1], row])


def rotate_rows(rows, l, psi, theta, phi):
    """The definition at one l: rows (..., l + 1) holds a_lm, m = 0 .. l; the same shape comes back."""
    mm = np.arange(-l, l + 1)
    big = np.exp(-1j * mm * phi)[:, None] * wigner_d(l, theta) * np.exp(-1j * mm * psi)[None, :]
    flat = rows.reshape(-1, l + 1)
    out = np.stack([(big @ full_orders(r, l))[l:] for r in flat])
    return out.reshape(rows.shape)


def rotate_alm_ref(alm, lmax, psi, theta, phi):
    """The definition with the full (2 l + 1)^2 matrices, every l; alm (..., nlm)."""
    alm = np.asarray(alm, dtype=np.complex128)
    l, m = lm_index(lmax)
    out = np.empty_like(alm)
    for ll in range(lmax + 1):
        sel = np.flatnonzero(l == ll)  # ascending m
        out[..., sel] = rotate_rows(alm[..., sel], ll, psi, theta, phi)
    return out


def values(alm, lmax, theta, phi):
    """f(theta_i, phi_i) = sum_lm a_lm Y_lm of the real field with coefficients alm (nlm,), summed directly."""
    from scipy.special import sph_harm_y

    theta, phi = np.asarray(theta, dtype=float), np.asarray(phi, dtype=float)
    l, m = lm_index(lmax)
    y = sph_harm_y(l[:, None], m[:, None], theta[None, :], phi[None, :])
    w = np.where(m == 0, 1.0, 2.0)[:, None]
    return (w * (np.asarray(alm)[:, None] * y).real).sum(axis=0)


def random_alm(rng, lmax, ncomp=None):
    """Random coefficients of real fields: a_l0 real."""
    l, m = lm_index(lmax)
    shape = (l.size,) if ncomp is None else (ncomp, l.size)
    a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    a[..., m == 0] = a[..., m == 0].real
    return a


def directions(theta, phi):
    return np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])


def angles(xyz):
    return np.arccos(np.clip(xyz[2], -1.0, 1.0)), np.arctan2(xyz[1], xyz[0])


# ---- the long-double restatement, one output column at a time ---------------------------------------------------------------------------

_CHUNK = 4096  # mantissas in [1/2, 1): a chunk's running product stays above 2^-4097, far inside the long-double range
_RENORM = 32   # a chain grows by less than 2^15 per step: 32 steps stay inside the range of a double as well


def running_product(r):
    """(mantissa, exponent) of r[0], r[0] r[1], ...: long-double mantissas in [1/2, 1) with the sign (0 stays 0), int64 exponents."""
    mr, er = np.frexp(np.asarray(r, dtype=LD))
    mant, expo = np.empty_like(mr), np.cumsum(er.astype(np.int64))
    carry, ce = LD(1), 0
    for i in range(0, mr.size, _CHUNK):
        pm, pe = np.frexp(np.cumprod(mr[i : i + _CHUNK]) * carry)
        mant[i : i + _CHUNK] = pm
        expo[i : i + _CHUNK] += pe + ce
        carry, ce = pm[-1], ce + int(pe[-1])
    return mant, expo


def _sqrt_me(mant, expo):
    odd = expo & 1
    return np.sqrt(np.where(odd == 1, 2 * mant, mant)), (expo - odd) // 2


def half_angle(theta):
    """cos(theta / 2), sin(theta / 2) of the double theta in long double."""
    h = LD(theta) / 2
    return np.cos(h), np.sin(h)


def chain_seeds(lmax, m, theta):
    """d^(l0)_(m,m') for m' = -lmax .. lmax (index m' + lmax), l0 = max(m, |m'|), as (mantissa, exponent) in long double."""
    return _seeds(lmax, m, *half_angle(theta))


def _seeds(lmax, m, c, s):
    """``chain_seeds`` from c = cos(theta / 2) and s = sin(theta / 2)."""
    cm, ce = running_product(np.concatenate([[LD(1)], np.full(2 * lmax, c, dtype=LD)]))  # c^k, k = 0 .. 2 lmax
    sm, se = running_product(np.concatenate([[LD(1)], np.full(2 * lmax, s, dtype=LD)]))
    mant, expo = np.zeros(2 * lmax + 1, dtype=LD), np.zeros(2 * lmax + 1, dtype=np.int64)

    # |m'| <= m: sqrt(C(2m, m + m')) from the ratios C(n, k) / C(n, k - 1) = (n - k + 1) / k
    k = np.arange(1, 2 * m + 1)
    bm, be = _sqrt_me(*running_product(np.concatenate([[LD(1)], (2 * m - k + 1).astype(LD) / k.astype(LD)])))
    b = np.arange(-m, m + 1)
    sign = np.where((m - b) & 1, LD(-1), LD(1))
    mant[b + lmax] = sign * bm * cm[m + b] * sm[m - b]
    expo[b + lmax] = be + ce[m + b] + se[m - b]

    # |m'| = A > m: sqrt(C(2A, A + m)) from C(2A + 2, A + 1 + m) / C(2A, A + m) = (2A + 2)(2A + 1) / ((A + 1 + m)(A + 1 - m))
    if lmax > m:
        a = np.arange(m, lmax)
        ratio = ((2 * a + 2) * (2 * a + 1)).astype(LD) / ((a + 1 + m) * (a + 1 - m)).astype(LD)
        bm, be = _sqrt_me(*running_product(ratio))
        a = a + 1
        mant[lmax + a] = bm * cm[a + m] * sm[a - m]
        expo[lmax + a] = be + ce[a + m] + se[a - m]
        mant[lmax - a] = np.where((a + m) & 1, LD(-1), LD(1)) * bm * cm[a - m] * sm[a + m]
        expo[lmax - a] = be + ce[a - m] + se[a + m]
    mant, shift = np.frexp(mant)
    return mant, expo + shift


def wigner_d_column(lmax, m, theta, dtype=LD):
    """Yields (l, d) for l = m .. lmax with d[m' + l] = d^l_(m,m')(theta), m' = -l .. l, as long doubles (0 below their range).

    ``dtype=np.float64`` is the yardstick for plain-FP64 chains: the coefficient l(l+1) x - m m' and the seeds are formed in long
    double and rounded once, everything else of a chain (the square roots, the two products, the difference) runs in float64."""
    m, lmax = int(m), int(lmax)
    assert 0 <= m <= lmax and dtype in (LD, np.float64)
    c, s = half_angle(theta)
    if dtype is LD:
        yield from _column_in_differences(lmax, m, c, s)
        return
    near_zero = abs(s) <= abs(c)  # x >= 0
    w = 2 * s * s if near_zero else 2 * c * c  # 1 - x or 1 + x
    mp = np.arange(-lmax, lmax + 1, dtype=np.int64)
    mp2, mmp = mp * mp, m * mp
    seed_m, seed_e = chain_seeds(lmax, m, theta)
    seed_m = seed_m.astype(dtype)
    n = 2 * lmax + 1
    dc, dp, ex, sl = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=dtype)
    for l in range(m, lmax + 1):
        lo, hi = lmax - l, lmax + l + 1
        if l == m:
            dc[lo:hi], ex[lo:hi] = seed_m[lo:hi], seed_e[lo:hi]
        else:
            for i in (lo, hi - 1):
                dc[i], ex[i] = seed_m[i], seed_e[i]
        yield l, np.ldexp(dc[lo:hi].astype(LD), ex[lo:hi])
        if l == lmax:
            break
        ll = l * (l + 1)
        if near_zero:
            coef = (ll - mmp[lo:hi]).astype(LD) - ll * w
        else:
            coef = ll * w - (ll + mmp[lo:hi]).astype(LD)
        coef = coef.astype(dtype)
        p1 = ((l + 1) ** 2 - m * m) * ((l + 1) ** 2 - mp2[lo:hi])  # exact in int64
        s1 = np.sqrt(p1.astype(dtype))
        if l == 0:  # d^1_00 = x d^0_00
            new = dtype(1 - w if near_zero else w - 1) * dc[lo:hi]
        else:
            new = (dtype(2 * l + 1) * coef * dc[lo:hi] - dtype(l + 1) * sl[lo:hi] * dp[lo:hi]) / (dtype(l) * s1)
        dp[lo:hi] = dc[lo:hi]
        dc[lo:hi] = new
        sl[lo:hi] = s1
        if (l - m) % _RENORM == _RENORM - 1:
            _, k = np.frexp(np.maximum(np.abs(dc[lo:hi]), np.abs(dp[lo:hi])))
            dc[lo:hi] = np.ldexp(dc[lo:hi], -k)
            dp[lo:hi] = np.ldexp(dp[lo:hi], -k)
            ex[lo:hi] += k


def _column_in_differences(lmax, m, c, s):
    """The long-double chains of ``wigner_d_column`` from c = cos(theta / 2), s = sin(theta / 2), carried as (d^l, D^l = d^l - d^(l-1)).

    For l theta >> 1 a step in l turns the phase of d^l by about theta, so at small theta consecutive values are nearly equal and a
    rounding error of the three-term form comes back 1 / sin(theta) larger.  The same recurrence in differences,
        D^(l+1) = (g d^l + (l+1) s_l D^l) / (l s_(l+1)),   g = (2l+1)(l(l+1) x - m m') - l s_(l+1) - (l+1) s_l,
    does not lose that if g is formed without its cancellation: with p = l^2 - m^2, q = l^2 - m'^2,
        s_l = sqrt(p q) = (p + q) / 2 - e_l,   e_l = (m'^2 - m^2)^2 / (2 (sqrt(p) + sqrt(q))^2),
    and the integers of g add up to (2l+1)(m - m')^2 / 2 exactly:
        g = (2l+1)(m - m')^2 / 2 + l e_(l+1) + (l+1) e_l - (2l+1) l(l+1) (1 - x),   1 - x = 2 s^2.
    What is left to cancel in g is the turning point of the chain, not rounding.  Near theta = pi consecutive values alternate
    instead, so x < 0 goes through pi - theta (c and s change places): d^l_(m,m')(theta) = (-1)^(l+m) d^l_(m,-m')(pi - theta)."""
    if abs(s) > abs(c):
        for l, d in _column_in_differences(lmax, m, s, c):
            yield l, (-d[::-1] if (l + m) & 1 else d[::-1])
        return
    w = 2 * s * s
    mp = np.arange(-lmax, lmax + 1, dtype=np.int64)
    mp2 = mp * mp
    half_sq = ((m - mp) ** 2).astype(LD) / 2
    dm2 = ((mp2 - m * m) ** 2).astype(LD)
    seed_m, seed_e = _seeds(lmax, m, c, s)
    n = 2 * lmax + 1
    dc, dl, ex = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=np.int64)
    el, sl = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)

    def e_and_s(l, sel):
        rp, rq = np.sqrt(LD(l * l - m * m)), np.sqrt((l * l - mp2[sel]).astype(LD))
        den = np.atleast_1d(2 * (rp + rq) ** 2)
        den[den == 0] = 1  # p = q = 0 is m'^2 = m^2: e = 0
        return dm2[sel] / den, rp * rq

    for l in range(m, lmax + 1):
        lo, hi = lmax - l, lmax + l + 1
        new = slice(lo, hi) if l == m else [lo, hi - 1]  # the chains that begin at this l: d^(l-1) = 0
        dc[new] = dl[new] = seed_m[new]
        ex[new] = seed_e[new]
        el[new], sl[new] = e_and_s(l, new)
        yield l, np.ldexp(dc[lo:hi], ex[lo:hi])
        if l == lmax:
            break
        if l == 0:  # d^1_00 = x d^0_00
            step = -w * dc[lo:hi]
            e1, s1 = e_and_s(1, slice(lo, hi))
        else:
            e1, s1 = e_and_s(l + 1, slice(lo, hi))
            g = (2 * l + 1) * half_sq[lo:hi] + l * e1 + (l + 1) * el[lo:hi] - ((2 * l + 1) * l * (l + 1)) * w
            step = (g * dc[lo:hi] + (l + 1) * sl[lo:hi] * dl[lo:hi]) / (l * s1)
        dc[lo:hi] += step
        dl[lo:hi] = step
        el[lo:hi], sl[lo:hi] = e1, s1
        if (l - m) % _RENORM == _RENORM - 1:
            _, k = np.frexp(np.maximum(np.abs(dc[lo:hi]), np.abs(dl[lo:hi])))
            dc[lo:hi] = np.ldexp(dc[lo:hi], -k)
            dl[lo:hi] = np.ldexp(dl[lo:hi], -k)
            ex[lo:hi] += k


def phase_table(lmax, alpha):
    """exp(-i m alpha), m = 0 .. lmax, as long-double (cos, -sin) of the long-double product m alpha."""
    arg = np.arange(lmax + 1).astype(LD) * LD(alpha)
    return np.cos(arg), -np.sin(arg)


def phased_rows(alm, lmax, psi, lmin=0):
    """c_lm' = exp(-i m' psi) a_lm' for l = lmin .. lmax, m' = 0 .. l of one component, as long-double (re, im)[l - lmin, m'];
    what every column of one alm and one psi shares.  Rows below lmin are taken to be zero and are not read."""
    alm = np.asarray(alm)
    assert alm.shape == ((lmax + 1) * (lmax + 2) // 2,)
    pr, pi = phase_table(lmax, psi)
    re, im = np.zeros((lmax + 1 - lmin, lmax + 1), dtype=LD), np.zeros((lmax + 1 - lmin, lmax + 1), dtype=LD)
    for mp in range(lmax + 1):
        l0 = max(mp, lmin)
        at = mp * (2 * lmax + 1 - mp) // 2
        a = alm[at + l0 : at + lmax + 1]
        ar, ai = a.real.astype(LD), (a.imag.astype(LD) if mp else np.zeros(a.size, dtype=LD))  # a_l0 of a real field
        re[l0 - lmin :, mp] = ar * pr[mp] - ai * pi[mp]
        im[l0 - lmin :, mp] = ar * pi[mp] + ai * pr[mp]
    return lmin, re, im


def rotate_column_ref(alm, lmax, m, psi, theta, phi, dtype=LD, *, lmin=0, rows=None):
    """a'_lm for l = m .. lmax of one component (complex long double), from ``wigner_d_column``.  ``rows=phased_rows(alm, lmax, psi,
    lmin)`` may be handed in where several columns share it; output rows l < lmin are exactly zero."""
    lmin, cre, cim = phased_rows(alm, lmax, psi, lmin) if rows is None else rows
    out_re, out_im = np.zeros(lmax + 1 - m, dtype=LD), np.zeros(lmax + 1 - m, dtype=LD)
    sg = np.where(np.arange(lmax + 1) & 1, LD(-1), LD(1))
    for l, d in wigner_d_column(lmax, m, theta, dtype):
        if l < lmin:
            continue
        # a_l,-m' = (-1)^m' conj(a_lm'):  sum_m' d_mm' c_m' = sum_(m' >= 0) (d+ + (-1)^m' d-) Re c + i (d+ - (-1)^m' d-) Im c
        dpos, dneg = d[l:], sg[1 : l + 1] * d[:l][::-1]
        e, f = dpos.copy(), dpos.copy()
        e[1:] += dneg
        f[1:] -= dneg
        out_re[l - m] = np.sum(e * cre[l - lmin, : l + 1])
        out_im[l - m] = np.sum(f * cim[l - lmin, : l + 1])
    pr, pi = phase_table(lmax, phi)
    out = np.empty(lmax + 1 - m, dtype=np.clongdouble)
    out.real = out_re * pr[m] - out_im * pi[m]
    out.imag = out_re * pi[m] + out_im * pr[m] if m else 0
    return out


def column_slice(lmax, m):
    """Where column m (l = m .. lmax) sits in the project's layout."""
    at = m * (2 * lmax + 1 - m) // 2
    return slice(at + m, at + lmax + 1)


def sparse_alm(rng, lmax, lmin=0):
    """One component in the project's layout: zeros except random rows l >= lmin, a_l0 real.  Only the live rows are drawn."""
    alm = np.zeros((lmax + 1) * (lmax + 2) // 2, dtype=np.complex128)
    for m in range(lmax + 1):
        sel = slice(m * (2 * lmax + 1 - m) // 2 + max(m, lmin), m * (2 * lmax + 1 - m) // 2 + lmax + 1)
        n = sel.stop - sel.start
        alm[sel] = rng.standard_normal(n) + (1j * rng.standard_normal(n) if m else 0)
    return alm
