"""Independent reference of the ring Fourier stage (numpy only): HEALPix RING geometry from the published formulas
(Gorski et al. 2005, ApJ 622, 759, section 4), per-ring DFTs by np.fft, the ring phase e^{-i m phi_0} and the quadrature
weight rw[rp] 4 pi / npix.  It shares nothing with the plan, the oracle's C code or any kernel.

Layout: ring pair rp = 0 .. 2 nside - 1 holds the northern ring i = rp + 1 and its mirror 4 nside - i (none for the equator
ring i = 2 nside).  Spectra are returned as F_N, F_S[comp][m][rp] (complex128)."""

import numpy as np


def ring_pair_geometry(nside):
    """Per ring pair: dict of int64 / bool arrays nphi, startN, startS (-1: no southern ring), shifted, and float64 phi0."""
    ns = int(nside)
    npix = 12 * ns * ns
    ncap = 2 * ns * (ns - 1)
    i = np.arange(1, 2 * ns + 1, dtype=np.int64)
    cap = i < ns
    nphi = np.where(cap, 4 * i, 4 * ns)
    startN = np.where(cap, 2 * i * (i - 1), ncap + (i - ns) * 4 * ns)
    shifted = np.where(cap, True, ((i - ns) & 1) == 0)
    startS = np.where(i == 2 * ns, -1, npix - startN - nphi)
    phi0 = np.where(shifted, np.pi / nphi, 0.0)
    return {"nphi": nphi, "startN": startN, "startS": startS, "shifted": shifted, "phi0": phi0}


def ring_cos_sin(nside):
    """(z, sin theta) of the northern ring of every ring pair (float64, the published closed forms)."""
    ns = int(nside)
    i = np.arange(1, 2 * ns + 1, dtype=np.float64)
    z = np.where(i < ns, 1.0 - i * i / (3.0 * ns * ns), (2 * ns - i) * 2.0 / (3.0 * ns))
    omz = np.where(i < ns, i * i / (3.0 * ns * ns), 1.0 - z)
    return z, np.sqrt(omz * (1.0 + z))


def fft_size_for(n):
    """In-LDS FFT length of a sub-DFT of length n (the ring has 4 n pixels): n itself for a power of two, else the Bluestein
    convolution length, the smallest power of two >= 2 n - 1."""
    n = int(n)
    if n & (n - 1) == 0:
        return n
    m = 1
    while m < 2 * n - 1:
        m <<= 1
    return m


def ring_phase(ms, nphi, shifted):
    """e^{-i m phi_0} for the orders ms on a ring of nphi pixels: phi_0 = pi / nphi on shifted rings, the exponent reduced as
    an exact integer (m mod 2 nphi) and the phase evaluated in extended precision."""
    ms = np.asarray(ms, dtype=np.int64)
    if not shifted:
        return np.ones(ms.shape, dtype=np.complex128)
    ld = np.longdouble
    a = -(np.mod(ms, 2 * nphi).astype(ld) * _PI_LD) / ld(nphi)
    return (np.cos(a).astype(np.float64) + 1j * np.sin(a).astype(np.float64)).astype(np.complex128)


_PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def _ring_blocks(geo, rp_list):
    """Groups the ring pairs of rp_list by ring length: one 2-D np.fft call per group (the belt is one group)."""
    out = {}
    for rp in rp_list:
        out.setdefault(int(geo["nphi"][rp]), []).append(int(rp))
    return out


def _rows(vec, starts, nphi):
    """vec[starts[t] + j], j < nphi, as a (len(starts), nphi) array: a view where the rings are adjacent in memory (the belt)."""
    if starts.size > 1 and np.all(np.diff(starts) == nphi):
        return vec[starts[0] : starts[-1] + nphi].reshape(starts.size, nphi)
    if starts.size > 1 and np.all(np.diff(starts) == -nphi):
        return vec[starts[-1] : starts[0] + nphi].reshape(starts.size, nphi)[::-1]
    return vec[starts[:, None] + np.arange(nphi)[None, :]]


def ring_spectra_ms(maps, nside, ms, pix_weights=None, ring_weights=None, rps=None, block=256):
    """F_N, F_S[comp][k][rp] at the orders ms (any integers >= 0, any order) for the ring pairs rps (default: all), with phase
    and quadrature weight applied.  Rings of one length go through np.fft as one 2-D call per block of ``block`` rings (memory:
    the spectra of one block plus the output)."""
    maps = np.asarray(maps, dtype=np.float64)
    maps = maps.reshape(-1, maps.shape[-1])
    ncomp = maps.shape[0]
    ns = int(nside)
    npix = 12 * ns * ns
    assert maps.shape[1] == npix
    ms = np.asarray(ms, dtype=np.int64)
    geo = ring_pair_geometry(ns)
    nrp = 2 * ns
    rps = np.arange(nrp) if rps is None else np.asarray(rps, dtype=np.int64)
    wq = (np.ones(nrp) if ring_weights is None else np.asarray(ring_weights, dtype=np.float64)) * (4.0 * np.pi / npix)
    FN = np.zeros((ncomp, ms.size, nrp), dtype=np.complex128)
    FS = np.zeros_like(FN)
    pw = None if pix_weights is None else np.asarray(pix_weights, dtype=np.float64)
    for nphi, group in _ring_blocks(geo, rps).items():
        bins = np.mod(ms, nphi)
        ph_shift = ring_phase(ms, nphi, True)
        for F, start in ((FN, geo["startN"]), (FS, geo["startS"])):
            live = np.asarray(group)
            live = live[start[live] >= 0]
            for b0 in range(0, live.size, block):
                sub = live[b0 : b0 + block]
                for c in range(ncomp):
                    f = _rows(maps[c], start[sub], nphi)
                    if pw is not None:
                        f = f * _rows(pw, start[sub], nphi)
                    v = np.fft.fft(f, axis=1)[:, bins]          # (rings, k)
                    v *= np.where(geo["shifted"][sub][:, None], ph_shift[None, :], 1.0)
                    v *= wq[sub][:, None]
                    F[c][:, sub] = v.T
    return FN, FS


def ring_spectra_ref(maps, nside, lmax, pix_weights=None, ring_weights=None):
    """F_N, F_S[comp][m][rp], m = 0 .. lmax (complex128): X = fft(f w_pix) per ring, F(m) = X[m mod nphi] e^{-i m phi_0}
    rw[rp] 4 pi / npix.  The equator (rp = 2 nside - 1) has F_S = 0."""
    return ring_spectra_ms(maps, nside, np.arange(lmax + 1), pix_weights, ring_weights)


def ring_spectra_chunks(maps, nside, lmax, chunk, pix_weights=None, ring_weights=None):
    """ring_spectra_ref in m-chunks: yields (m0, m1, F_N, F_S) with the orders [m0, m1), so that the spectra of a full-size map
    fit in host memory (the ring FFTs are taken again for every chunk: few, large chunks)."""
    maps = np.asarray(maps, dtype=np.float64).reshape(-1, 12 * int(nside) ** 2)
    for m0 in range(0, lmax + 1, chunk):
        m1 = min(lmax + 1, m0 + chunk)
        yield m0, m1, *ring_spectra_ms(maps, nside, np.arange(m0, m1), pix_weights, ring_weights)


def ring_dft_direct_ld(f, ms):
    """X[m] = sum_j f_j e^{-2 pi i j m / n} by the direct sum in extended precision (np.longdouble), j m reduced mod n as an exact
    integer: the spot check of np.fft itself."""
    f = np.asarray(f)
    n = f.shape[-1]
    ld = np.longdouble
    fr = np.real(f).astype(ld)
    fi = np.imag(f).astype(ld) if np.iscomplexobj(f) else np.zeros(n, dtype=ld)
    j = np.arange(n, dtype=np.int64)
    out = np.empty(len(ms), dtype=np.complex128)
    for t, m in enumerate(ms):
        a = -(ld(2) * _PI_LD) * (np.mod(j * int(m), n).astype(ld) / ld(n))
        c, s = np.cos(a), np.sin(a)
        re = np.sum(fr * c - fi * s)
        im = np.sum(fr * s + fi * c)
        out[t] = complex(float(re), float(im))
    return out
