"""The rule of ``hx.mask_discs``, ``hx.mask_distance`` and ``hx.apodize_mask`` restated in numpy by brute force,
independent of the library's code: the full (npix x ndisc) table of h against the limit for the discs, the full minimum over all
masked pixels for the distance, the tapers from that minimum.  Also the masks and discs the tests share."""

import numpy as np

from jkregions_reference import pix2vec_ring

EPS = 2.0**-53


def centres(nside):
    return pix2vec_ring(nside, np.arange(12 * nside * nside))


def chord_h(u, v):
    """h(u, v) = ((u_x - v_x)^2 + (u_y - v_y)^2 + (u_z - v_z)^2) / 2, summed in that order; u (..., 3), v (..., 3) broadcast."""
    d = u - v
    return 0.5 * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def angle_h(deg):
    s = np.sin(0.5 * np.radians(np.asarray(deg, dtype=np.float64)))
    return 2.0 * s * s


def disc_centres(lon, lat):
    lon, lat = np.radians(np.asarray(lon, dtype=np.float64)), np.radians(np.asarray(lat, dtype=np.float64))
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=-1)


def disc_table(nside, lon, lat):
    """h of every pixel centre to every disc centre: (npix, ndisc)."""
    return chord_h(centres(nside)[:, None, :], disc_centres(lon, lat)[None, :, :])


def disc_gap(nside, lon, lat, radius):
    """The smallest |h - h(radius_k)| / h(radius_k) over all pixel / disc pairs: the margin by which the rule decides."""
    hr = angle_h(np.broadcast_to(radius, np.shape(lon)))
    return float((np.abs(disc_table(nside, lon, lat) - hr) / hr).min())


def mask_discs(mask, lon, lat, radius):
    mask = np.array(mask, dtype=np.float64)
    nside = int(round((mask.size / 12) ** 0.5))
    if np.size(lon) == 0:
        return mask
    hr = angle_h(np.broadcast_to(radius, np.shape(lon)))
    mask[(disc_table(nside, lon, lat) <= hr).any(axis=1)] = 0.0
    return mask


def mask_h(mask, max_distance):
    """H[p] = min(h(max_distance), min over masked q of h(v_p, v_q)); 0 on masked pixels."""
    mask = np.asarray(mask, dtype=np.float64)
    nside = int(round((mask.size / 12) ** 0.5))
    v = centres(nside)
    cap = float(angle_h(max_distance))
    masked = mask <= 0
    H = np.full(mask.size, cap)
    if masked.any() and not masked.all():
        vm = v[masked]
        for lo in range(0, mask.size, 1024):
            H[lo:lo + 1024] = np.minimum(cap, chord_h(v[lo:lo + 1024, None, :], vm[None, :, :]).min(axis=1))
    H[masked] = 0.0
    return H


def taper(kind, x):
    x = np.asarray(x, dtype=np.float64)
    if kind == "C1":
        return x - np.sin(2.0 * np.pi * x) / (2.0 * np.pi)
    if kind == "C2":
        return 0.5 * (1.0 - np.cos(np.pi * x))
    raise ValueError(kind)


def apodize(mask, aposize, kind, H=None):
    mask = np.asarray(mask, dtype=np.float64)
    H = mask_h(mask, aposize) if H is None else H
    w = taper(kind, np.sqrt(H / angle_h(aposize)))
    return np.where(mask <= 0, 0.0, mask * w)


def distance_bound(H):
    """|H - H_ref| <= 64 2^-53 (sqrt(2 H_ref) + H_ref): unit-vector components agree to 4 ulp of 1, a coordinate difference carries
    8 2^-53, over three coordinates dh <= chord sqrt(3) 8 2^-53 plus four roundings of the sum: 32 2^-53 (chord + H); twice that."""
    return 64 * EPS * (np.sqrt(2.0 * H) + H)


def taper_bound(mask, aposize):
    """|out - out_ref| <= 256 2^-53 |mask| / sqrt(h(aposize)): |dw/dx| <= 2 and dx = dH / (2 sqrt(H h(aposize)))."""
    return 256 * EPS * np.abs(mask) / np.sqrt(angle_h(aposize))


# ---- the inputs of the tests -----------------------------------------------------------------------------------------------------------

def ring_start(nside, ir):
    """First RING pixel and length of ring ir (1 .. 4 nside - 1)."""
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    if ir < nside:
        return 2 * ir * (ir - 1), 4 * ir
    if ir <= 3 * nside:
        return ncap + (ir - nside) * 4 * nside, 4 * nside
    irs = 4 * nside - ir
    return npix - 2 * irs * (irs + 1), 4 * irs


def named_discs(nside):
    """(lon, lat, radius) of the discs at the places the kernels can go wrong: one holding each pole, one across phi = 0, one on the
    cap / belt transition ring (z = 2/3), one on the equator, one tiny one."""
    lat_t = np.degrees(np.arcsin(2.0 / 3.0))
    lon = np.array([37.3, 211.9, 359.2, 123.4, 270.15, 0.7, 45.0])
    lat = np.array([86.1, -84.7, 12.3, lat_t + 0.4, 0.21, -33.0, lat_t])
    radius = np.array([9.3, 11.1, 13.7, 8.9, 10.3, 17.2, 3.1])
    return lon, lat, radius


def random_discs(count, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 360, count), np.degrees(np.arcsin(rng.uniform(-1, 1, count))), rng.uniform(3.0, 20.0, count)


def hole_masks(nside, seed=11):
    """{name: mask} of the distance and taper tests."""
    npix = 12 * nside * nside
    rng = np.random.default_rng(seed)
    out = {}
    lon, lat, radius = named_discs(nside)
    out["poles, phi = 0, transition and equator discs"] = mask_discs(np.ones(npix), lon[:5], lat[:5], radius[:5] * 0.6)
    m = np.ones(npix)
    m[1] = 0.0
    out["one pixel of ring 1"] = m
    m = np.ones(npix)
    first, n = ring_start(nside, 2 * nside)
    m[first + n - 1] = 0.0
    m[first + n // 2] = 0.0
    out["nearest across the phi wrap"] = m  # (pixels 0, 1, ... of the equator ring reach n - 1 across phi = 0)
    out["nothing masked"] = np.ones(npix)
    out["everything masked"] = np.zeros(npix)
    m = rng.uniform(0.05, 1.0, npix)
    m[rng.random(npix) < 0.02] = 0.0
    m[rng.random(npix) < 0.01] = -0.5
    out["non-binary with scattered holes"] = m
    return out
