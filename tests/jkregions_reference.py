"""The rule of ``hx.jackknife_regions`` restated in numpy, independent of the library's code: recursive weighted
bisection of a footprint along the principal axis.  ``np.linalg.eigh`` for the axes, ``np.argsort(kind="stable")`` for the order,
Python integers for every weight sum and for ``Q n1``.  Also the footprints the tests share."""

import numpy as np

NJK_MAX = 4096


def pix2vec_ring(nside, pix):
    """Unit vectors (n, 3) of the centres of RING pixels, any integer nside (the pix2ang of the HEALPix paper)."""
    pix = np.asarray(pix, dtype=np.int64)
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    z, phi = np.empty(pix.shape), np.empty(pix.shape)
    sth = np.empty(pix.shape)
    north, south = pix < ncap, pix >= npix - ncap
    eq = ~north & ~south
    for cap, sign in ((north, 1.0), (south, -1.0)):
        if not cap.any():
            continue
        ip = pix[cap] + 1 if sign > 0 else npix - pix[cap]
        iring = (1 + np.sqrt(2 * ip - 1).astype(np.int64)) >> 1
        iring = np.where(2 * iring * (iring - 1) >= ip, iring - 1, iring)
        iring = np.where(2 * iring * (iring + 1) < ip, iring + 1, iring)
        iphi = ip - 2 * iring * (iring - 1)
        if sign < 0:
            iphi = 4 * iring + 1 - iphi
        t = iring * iring * (4.0 / npix)
        z[cap] = sign * (1.0 - t)
        sth[cap] = np.sqrt(t * (2.0 - t))
        phi[cap] = (iphi - 0.5) * (np.pi / 2) / iring
    if eq.any():
        ip = pix[eq] - ncap
        iring = ip // (4 * nside) + nside
        iphi = ip % (4 * nside) + 1
        fodd = np.where((iring + nside) & 1, 1.0, 0.5)
        zz = (2 * nside - iring) * (2.0 / (3.0 * nside))
        z[eq] = zz
        sth[eq] = np.sqrt((1.0 - zz) * (1.0 + zz))
        phi[eq] = (iphi - fodd) * (np.pi / 2) / nside
    return np.stack([sth * np.cos(phi), sth * np.sin(phi), z], axis=-1)


def quantise(weight, wmax):
    """q = max(1, rint(w / wmax 2^32)) as Python-sized integers (int64 holds them)."""
    return np.maximum(1, np.rint(np.asarray(weight, dtype=np.float64) / wmax * 2.0**32)).astype(np.int64)


def order_key(t):
    """The 64-bit key whose unsigned order is the order of the doubles t + 0.0."""
    b = (np.asarray(t, dtype=np.float64) + 0.0).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def split_target(Q, n1, n):
    return (int(Q) * int(n1)) // int(n)


def split_count(q_sorted, n1, n):
    """The clamped number of pixels that go left, from the integer weights in split order."""
    q = [int(x) for x in q_sorted]
    m, T = len(q), split_target(sum(q), n1, n)
    E = c = 0
    for qj in q:
        if 2 * E + qj <= 2 * T:
            c += 1
        E += qj
    return min(max(c, n1), m - (n - n1))


def principal_axis(C):
    """Unit eigenvector of the largest eigenvalue of the symmetric 3 x 3 C, its component of largest magnitude positive."""
    w, v = np.linalg.eigh(np.asarray(C, dtype=np.float64))
    a = v[:, np.argmax(w)]
    return a if a[np.argmax(np.abs(a))] > 0 else -a


def covariance(q, v):
    """C = S2 / S0 - (S1 / S0)(S1 / S0)^T of the unit vectors v (m, 3) with the integer weights q, in float64."""
    w = q.astype(np.float64)
    s0 = w.sum()
    mean = (w[:, None] * v).sum(axis=0) / s0
    return (w[:, None, None] * v[:, :, None] * v[:, None, :]).sum(axis=0) / s0 - np.outer(mean, mean)


def regions(nside, weight, njk, perturb=None):
    """(labels int32 [npix], region weights [njk], axes [njk - 1, 3]).  ``perturb``: a generator; every split axis then gets a
    random offset of size 1e-9 before it is used (the yardstick check: the labels must not depend on the last digits of an axis)."""
    weight = np.asarray(weight, dtype=np.float64)
    if weight.shape != (12 * nside * nside,):
        raise ValueError("weight is not a map of this nside")
    if not 1 <= njk <= NJK_MAX:
        raise ValueError("njk out of range")
    bad = np.flatnonzero(~(np.isfinite(weight) & (weight >= 0)))
    if bad.size:
        raise ValueError(f"pixel {bad[0]} has an invalid weight")
    pix = np.flatnonzero(weight > 0)
    if pix.size < njk:
        raise ValueError("fewer footprint pixels than njk")
    q = quantise(weight[pix], weight.max())
    vec = pix2vec_ring(nside, pix)
    labels = np.zeros(weight.size, dtype=np.int32)
    axes = np.zeros((njk - 1, 3))
    level = [(1, njk, np.arange(pix.size))]  # (first, n, indices into pix, ascending)
    while any(n >= 2 for _, n, _ in level):
        nxt = []
        for first, n, idx in level:
            if n < 2:
                nxt.append((first, n, idx))
                continue
            n1 = n // 2
            a = principal_axis(covariance(q[idx], vec[idx]))
            axes[first + n1 - 2] = a
            if perturb is not None:
                a = a + 1e-9 * perturb.standard_normal(3)
            t = (a[0] * vec[idx, 0] + a[1] * vec[idx, 1]) + a[2] * vec[idx, 2] + 0.0
            o = np.argsort(t, kind="stable")  # (idx ascends: ties keep ascending pixel order)
            c = split_count(q[idx][o], n1, n)
            nxt.append((first, n1, np.sort(idx[o[:c]])))
            nxt.append((first + n1, n - n1, np.sort(idx[o[c:]])))
        level = nxt
    for first, n, idx in level:
        labels[pix[idx]] = first
    rw = np.array([weight[labels == k].sum() for k in range(1, njk + 1)])
    return labels, rw, axes


def check_invariants(weight, labels, njk):
    """Labels 0 exactly outside the footprint, every label present, region weights within 2 ceil(log2 njk) wmax of each other."""
    weight, labels = np.asarray(weight), np.asarray(labels)
    assert ((labels == 0) == (weight <= 0)).all()
    assert labels.min() >= 0 and labels.max() <= njk
    present = np.bincount(labels[labels > 0], minlength=njk + 1)[1:]
    assert (present > 0).all(), np.flatnonzero(present == 0)[:5] + 1
    rw = np.bincount(labels, weights=weight, minlength=njk + 1)[1:]
    levels = int(np.ceil(np.log2(njk))) if njk > 1 else 0
    assert rw.max() - rw.min() <= 2 * levels * weight.max(), (rw.max() - rw.min(), 2 * levels * weight.max())
    return rw


# ---- the footprints of the tests --------------------------------------------------------------------------------------------------

C1 = np.array([0.3, 0.8, 0.5]) / np.linalg.norm([0.3, 0.8, 0.5])
C2 = np.array([-0.6, 0.1, -0.79]) / np.linalg.norm([-0.6, 0.1, -0.79])
C3 = np.array([0.6, -0.64, 0.48])


def all_vectors(nside):
    return pix2vec_ring(nside, np.arange(12 * nside * nside))


def parity_weight(nside, seed=2024):
    """The three-piece footprint of the parity cases with weights uniform(0.2, 1)."""
    v = all_vectors(nside)
    inside = (v @ C1 > 0.55) | (v @ C2 > 0.8) | ((np.abs(v @ C3) < 0.12) & (v[:, 0] > 0))
    w = np.random.default_rng(seed).uniform(0.2, 1.0, v.shape[0])
    return np.where(inside, w, 0.0)


def cap_weight(nside, cut):
    """The binary cap mask v . c1 > cut."""
    return (all_vectors(nside) @ C1 > cut).astype(np.float64)


def first_pixels_weight(nside, count, seed=7):
    """A footprint of exactly ``count`` pixels: the ``count`` pixels nearest to c2, weights uniform(0.2, 1)."""
    d = all_vectors(nside) @ C2
    w = np.zeros(d.size)
    w[np.argsort(-d, kind="stable")[:count]] = np.random.default_rng(seed).uniform(0.2, 1.0, count)
    return w


def clamp_weight(nside=16):
    """The cap v . c1 > 0.9 with weight 1e-6 everywhere but one pixel of weight 1: the targets cannot be met, the clamp decides."""
    w = cap_weight(nside, 0.9) * 1e-6
    w[np.flatnonzero(w > 0)[3]] = 1.0
    return w
