"""Pixels of a HEALPix map in RING order picked by ring, from the oracle's ring table: nothing here touches an array of npix entries,
so the choices cost the same at nside 4096 as at nside 8."""

import numpy as np

from oracle import hxoracle as oracle

_TABLES = {}


def ring_table(nside):
    """First pixel, length, z, sin(theta) and phi_0 of the rings 1 .. 4 nside - 1 (index 0 .. 4 nside - 2, north to south)."""
    if nside not in _TABLES:
        rings = [oracle.ring_info(nside, r) for r in range(1, 4 * nside)]
        tab = tuple(np.array([r[k] for r in rings]) for k in range(5))
        for a in tab:
            a.setflags(write=False)
        _TABLES[nside] = tab
    return _TABLES[nside]


def ring_of(nside, pix):
    """0-based ring index of the given pixels."""
    return np.searchsorted(ring_table(nside)[0], np.asarray(pix), side="right") - 1


def pixel_angles(nside, pix):
    """(theta, phi) of the given pixels: the entries of oracle.pix2ang(nside), bit for bit."""
    start, nphi, z, sth, phi0 = ring_table(nside)
    pix = np.asarray(pix)
    r = ring_of(nside, pix)
    return np.arctan2(sth[r], z[r]), phi0[r] + 2 * np.pi * (pix - start[r]) / nphi[r]


def special_pixels(nside, rng, n=400):
    """At most n pixels where the ring geometry changes: all four pixels of the first and of the last ring; on ring nside (the
    cap meets the belt), on two neighbouring belt rings (one shifted, one not), on the equator and on the mirror of ring nside
    the first and the last pixel and a few between; random pixels for the rest.  Every pixel of a small map."""
    npix = 12 * nside * nside
    if npix <= n:
        return np.arange(npix)
    start = ring_table(nside)[0]
    end = np.concatenate([start[1:], [npix]])
    pix = [0, 1, 2, 3, npix - 4, npix - 3, npix - 2, npix - 1]
    for r in (nside - 2, nside - 1, nside, nside + 1, 2 * nside - 1, 3 * nside - 1, 3 * nside):  # (0-based ring numbers)
        pix += [start[r], end[r] - 1]
        pix += list(rng.integers(start[r], end[r], 6))
    pix = np.unique(np.array(pix, dtype=np.int64))
    rest = np.setdiff1d(rng.choice(npix, n, replace=False), pix)[: n - pix.size]
    return np.sort(np.concatenate([pix, rest]))
