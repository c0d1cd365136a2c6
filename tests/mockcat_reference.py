"""Plain numpy restatement of the definition of a Poisson-sampled mock catalogue: the count of every pixel
(inversion below lambda = 32, Hoermann's PTRS from there on), the points of a pixel (sub-pixel offsets through HEALPix's face map)
and their values.  It is the reference of tests/test_mockcat_host.py and tests/test_gpu_mockcat.py and is never compared with
itself: its samplers are pinned by their moments, its positions by ``oracle.ang2pix_ring`` returning the source pixel.

The pixel -> (face, ix, iy) step follows the projection of the pixel centre (the relations of ``pixel_reference.ring2nest_exact``,
which hold for any nside), not the ring2xyf route the library takes.

Every comparison and floor of the count samplers reports its margin: a library whose exp / log / lgamma differ from numpy's in the
last places may take the other branch where the margin is below ``COMPARE_RTOL`` (comparisons, relative to the largest term that
entered either side) or ``FLOOR_RTOL * max(1, |argument|)`` (floors); ``counts`` returns those pixels as ``unsafe``."""

import math

import numpy as np

import synalm_reference as sr

STREAM_BIT = 0x80000000
LAMBDA_SWITCH, LAMBDA_MAX = 32.0, 2.0**30
INVERSION_KMAX, PTRS_MAXIT = 200, 64
COMPARE_RTOL = FLOOR_RTOL = 1e-9

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def _key(seed):
    seed = int(seed)
    return seed & 0xFFFFFFFF, seed >> 32


def _words(pixel, index, stream, realisation, seed):
    return sr.philox4x32_10(pixel, index, STREAM_BIT | stream, realisation, *_key(seed))


def _cmp_margin(lhs, rhs, scale=None):
    scale = np.maximum(np.abs(lhs), np.abs(rhs)) if scale is None else scale
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.abs(lhs - rhs) / scale
    return np.where(np.isnan(m), np.inf, m)


def poisson_inversion(lam, u):
    """(k, margin) of the sequential search on u in [0, 1): p = exp(-lam), cdf = p; while u >= cdf: k += 1, p *= lam / k, cdf += p;
    at most INVERSION_KMAX steps."""
    lam, u = np.broadcast_arrays(np.asarray(lam, dtype=np.float64), np.asarray(u, dtype=np.float64))
    p = np.exp(-lam)
    cdf = p.copy()
    k = np.zeros(lam.shape, dtype=np.int64)
    margin = np.full(lam.shape, np.inf)
    live = np.ones(lam.shape, dtype=bool)
    for step in range(INVERSION_KMAX + 1):
        margin = np.where(live, np.minimum(margin, _cmp_margin(u, cdf)), margin)
        live = live & (u >= cdf)
        if step == INVERSION_KMAX or not live.any():
            break
        k = np.where(live, k + 1, k)
        p = np.where(live, p * (lam / np.maximum(k, 1)), p)
        cdf = np.where(live, cdf + p, cdf)
    return k, margin


def poisson_ptrs(lam, pixel, realisation, seed):
    """(k, margin, iterations) of Hoermann's PTRS, 32 <= lam <= 2^30, (u1, u2) of one call per iteration."""
    lam = np.asarray(lam, dtype=np.float64)
    pixel = np.broadcast_to(np.asarray(pixel), lam.shape)
    slam, loglam = np.sqrt(lam), np.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    inva = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    out = np.floor(lam).astype(np.int64)
    margin = np.full(lam.shape, np.inf)
    iters = np.zeros(lam.shape, dtype=np.int64)
    live = np.ones(lam.shape, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for it in range(PTRS_MAXIT):
            if not live.any():
                break
            iters = np.where(live, it + 1, iters)
            u1, V = sr.uniforms(*_words(pixel, it, 0, realisation, seed))
            U = u1 - 0.5
            us = 0.5 - np.abs(U)
            arg = (2.0 * a / us + b) * U + lam + 0.43
            kf = np.floor(arg)
            m = np.minimum(arg - kf, kf + 1.0 - arg) / (FLOOR_RTOL * np.maximum(1.0, np.abs(arg))) * COMPARE_RTOL
            m = np.where(np.isfinite(arg), m, np.inf)
            m = np.minimum(m, _cmp_margin(us, 0.07))
            m = np.minimum(m, _cmp_margin(V, vr))
            fast = (us >= 0.07) & (V <= vr)
            m_slow = np.minimum(_cmp_margin(us, 0.013), _cmp_margin(V, us))
            m_slow = np.minimum(m_slow, np.where(np.abs(arg) < 1.0, np.abs(arg) / FLOOR_RTOL * COMPARE_RTOL, np.inf))  # (kf < 0)
            retry = (kf < 0) | ((us < 0.013) & (V > us))
            t1, t2, t3 = np.log(V), np.log(inva), np.log(a / (us * us) + b)
            kl = kf * loglam
            lg = _lgamma(np.where(np.isfinite(kf) & (kf >= 0), kf, 0.0) + 1.0)
            lhs = t1 + t2 - t3
            rhs = -lam + kl - lg
            scale = np.maximum.reduce([np.abs(t1), np.abs(t2), np.abs(t3), lam, np.abs(kl), np.abs(lg)])
            m_log = _cmp_margin(lhs, rhs, scale)
            accept = fast | (~retry & (lhs <= rhs))
            m = np.where(fast, m, np.minimum(m, np.where(retry, m_slow, np.minimum(m_slow, m_log))))
            margin = np.where(live, np.minimum(margin, m), margin)
            take = live & accept
            out = np.where(take, np.where(np.isfinite(kf), kf, 0).astype(np.int64), out)
            live = live & ~accept
    return out, margin, iters


def counts(lam, pixel, seed, realisation=0):
    """(n, unsafe) of the pixels ``pixel`` (RING indices, the counter word) with expected counts ``lam``: n int64, unsafe True where a
    comparison or floor was taken within its threshold.  ValueError naming the first pixel with an invalid lam."""
    lam = np.asarray(lam, dtype=np.float64)
    pixel = np.asarray(pixel, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        bad = ~((lam >= 0) & (lam <= LAMBDA_MAX))
    if bad.any():
        raise ValueError(f"invalid expected count at pixel {int(pixel[np.argmax(bad)])}")
    n = np.zeros(lam.shape, dtype=np.int64)
    margin = np.full(lam.shape, np.inf)
    low = (lam > 0) & (lam < LAMBDA_SWITCH)
    if low.any():
        _, u2 = sr.uniforms(*_words(pixel[low], 0, 0, realisation, seed))
        n[low], margin[low] = poisson_inversion(lam[low], u2)
    high = lam >= LAMBDA_SWITCH
    if high.any():
        n[high], margin[high], _ = poisson_ptrs(lam[high], pixel[high], realisation, seed)
    return n, margin < COMPARE_RTOL


# ---- positions --------------------------------------------------------------------------------------------------------------------------
JRLL = np.array([2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4])
JPLL = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7])


def _isqrt(v):
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    return np.where((r + 1) * (r + 1) <= v, r + 1, r)


def ring2xyf(nside, p):
    """(face, ix, iy) of the RING pixels p, any nside: from the centre of pixel j of ring i put into the point rule."""
    p = np.asarray(p, dtype=np.int64)
    nside = int(nside)
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    # ring i = 1 .. 4 nside - 1 and position j = 1 .. in it
    i_n = (1 + _isqrt(1 + 2 * p)) // 2
    j_n = p + 1 - 2 * i_n * (i_n - 1)
    q = np.maximum(npix - p, 1)
    i_s = (1 + _isqrt(2 * q - 1)) // 2
    j_s = 4 * i_s + 1 - (q - 2 * i_s * (i_s - 1))
    i_b = (p - ncap) // (4 * nside) + nside
    j_b = (p - ncap) % (4 * nside) + 1
    north, south = p < ncap, p >= npix - ncap
    # belt
    fodd2 = np.where((i_b - nside) % 2 == 0, 1, 2)
    jp = (2 * j_b - fodd2 + i_b - nside) // 2
    jm = (2 * j_b - fodd2 + 3 * nside - i_b) // 2
    ifp, ifm = jp // nside, jm // nside
    face_b = np.where(ifp == ifm, (ifp & 3) + 4, np.where(ifp < ifm, ifp, ifm + 8))
    ix_b, iy_b = jm % nside, nside - 1 - jp % nside
    # caps, ring counted from the pole of its hemisphere
    ic = np.where(south, i_s, np.maximum(i_n, 1))
    j = np.where(south, j_s, j_n)
    ntt = np.minimum(3, (j - 1) // ic)
    jpc, jmc = j - 1 - ntt * ic, ic - j + ntt * ic
    face = np.where(north, ntt, np.where(south, ntt + 8, face_b))
    ix = np.where(north, nside - 1 - jmc, np.where(south, jpc, ix_b))
    iy = np.where(north, nside - 1 - jpc, np.where(south, jmc, iy_b))
    return face, ix, iy


def offsets(x0, x1):
    return ((x0 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0**-24, ((x1 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0**-24


def xyf2lonlat(nside, face, ix, iy, u, v):
    """(lon, lat) in degrees of the point (u, v) of pixel (face, ix, iy): HEALPix's area-preserving face map."""
    x = (ix.astype(np.float64) + u) / float(nside)
    y = (iy.astype(np.float64) + v) / float(nside)
    jr = (JRLL[face].astype(np.float64) - x) - y
    north, south = jr < 1.0, jr > 3.0
    nr = np.where(north, jr, np.where(south, 4.0 - jr, 1.0))
    t = nr * nr / 3.0
    z_belt = (2.0 - jr) * 2.0 / 3.0
    z = np.where(north, 1.0 - t, np.where(south, t - 1.0, z_belt))
    sth = np.sqrt(np.where(north | south, t * (2.0 - t), (1.0 - z_belt) * (1.0 + z_belt)))
    tmp = (JPLL[face].astype(np.float64) * nr + x) - y
    tmp = np.where(tmp < 0.0, tmp + 8.0, tmp)
    tmp = np.where(tmp >= 8.0, tmp - 8.0, tmp)
    phi = 0.7853981633974483 * tmp / nr
    return phi * 57.29577951308232, np.arctan2(z, sth) * 57.29577951308232


def positions(nside, pixel, index, seed, realisation=0):
    """(lon, lat) of point ``index`` of RING pixel ``pixel`` (arrays broadcast)."""
    pixel, index = np.broadcast_arrays(np.asarray(pixel, dtype=np.int64), np.asarray(index, dtype=np.int64))
    x0, x1, _, _ = _words(pixel, index, 1, realisation, seed)
    return xyf2lonlat(nside, *ring2xyf(nside, pixel), *offsets(x0, x1))


def noise(pixel, index, column, seed, realisation=0):
    """The standard normal of value column ``column`` of that point: the first of the Box-Muller pair of stream 2 + column."""
    u1, u2 = sr.uniforms(*_words(pixel, index, 2 + int(column), realisation, seed))
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def catalog(nside, pix_begin, count, seed, realisation=0, maps=None, sigma=None):
    """The catalogue of the counts ``count`` of pixels pix_begin ..: dict of pix, index, lon, lat and values [nval][total]."""
    count = np.asarray(count, dtype=np.int64)
    local = np.repeat(np.arange(count.size), count)
    pix = local + int(pix_begin)
    start = np.cumsum(count) - count
    index = np.arange(pix.size) - start[local]
    lon, lat = positions(nside, pix, index, seed, realisation) if pix.size else (np.zeros(0), np.zeros(0))
    out = {"pix": pix, "index": index, "lon": lon, "lat": lat}
    if maps is not None:
        maps = np.atleast_2d(np.asarray(maps, dtype=np.float64))
        sigma = np.zeros(len(maps)) if sigma is None else np.asarray(sigma, dtype=np.float64)
        vals = np.empty((len(maps), pix.size))
        for j, (m, s) in enumerate(zip(maps, sigma)):
            vals[j] = m[local]
            if s != 0 and pix.size:
                vals[j] = vals[j] + s * noise(pix, index, j, seed, realisation)
        out["values"] = vals
    return out
