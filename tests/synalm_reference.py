"""Plain numpy restatement of the definition of hx_synalm: Philox4x32-10 on uint64 arrays, the bits -> normal
conversion, the column Cholesky with the tau rule and the triangular sum in ascending j.  It is the reference of
tests/test_synalm_host.py and tests/test_gpu_synalm.py and is never compared with itself: its Philox is pinned by the known
answers, its factor by L L^T = C, its alms by their spectra."""

from itertools import combinations_with_replacement

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

#: (counter, key, output) of Philox4x32-10
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint64 arrays holding the 32-bit output words x0..x3 (inputs broadcast against each other)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # (32 x 32 bits: no overflow in uint64)
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & MASK, n2, p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniforms(x0, x1, x2, x3):
    """u1 in (0, 1], u2 in [0, 1), both exact in f64."""
    k1 = ((x0 >> np.uint64(5)) << np.uint64(26)) + (x1 >> np.uint64(6))
    k2 = ((x2 >> np.uint64(5)) << np.uint64(26)) + (x3 >> np.uint64(6))
    return (k1 + np.uint64(1)).astype(np.float64) * 2.0**-53, k2.astype(np.float64) * 2.0**-53


def complex_normals(l, m, j, realisation, seed):
    """z of the coefficients (l, m) of component j (arrays broadcast): real at m = 0, (first + i second) / sqrt 2 above."""
    seed = int(seed)
    u1, u2 = uniforms(*philox4x32_10(l, m, j, realisation, seed & 0xFFFFFFFF, seed >> 32))
    r = np.sqrt(-2.0 * np.log(u1))
    first, second = r * np.cos(6.283185307179586 * u2), r * np.sin(6.283185307179586 * u2)
    m = np.broadcast_to(m, first.shape)
    return np.where(m == 0, first + 0j, (first * 0.7071067811865476) + 1j * (second * 0.7071067811865476))


def pair_list(ncomp):
    return list(combinations_with_replacement(range(ncomp), 2))


def pack(full):
    """(N, N, nl) symmetric -> (N (N + 1) / 2, nl) in combinations_with_replacement order."""
    return np.ascontiguousarray(np.stack([full[a, b] for a, b in pair_list(full.shape[0])]))


def unpack(packed, ncomp, lower=False):
    """Packed rows -> (N, N, nl): symmetric, or the lower triangle L_ij at row (j, i) with zeros above."""
    full = np.zeros((ncomp, ncomp, packed.shape[-1]))
    for row, (a, b) in zip(packed, pair_list(ncomp)):
        full[b, a] = row
        if not lower:
            full[a, b] = row
    return full


def cholesky(packed, ncomp):
    """The factor of DESIGN.md 4.15, packed like the input; ValueError naming the smallest failing l."""
    packed = np.asarray(packed, dtype=np.float64)
    bad = ~np.isfinite(packed).all(axis=0)
    if bad.any():
        raise ValueError(f"NaN or Inf at l = {int(np.argmax(bad))}")
    C = unpack(packed, ncomp)
    nl = C.shape[-1]
    L = np.zeros_like(C)
    failed = np.full(nl, -1)
    for j in range(ncomp):
        d = C[j, j].copy()
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        tau = 4.0 * ncomp * 2.0**-52 * C[j, j]
        failed = np.where((failed < 0) & (d < -tau), j, failed)
        live = d > tau
        ljj = np.sqrt(np.where(live, d, 1.0))
        L[j, j] = np.where(live, ljj, 0.0)
        for i in range(j + 1, ncomp):
            s = C[i, j].copy()
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            L[i, j] = np.where(live, s / ljj, 0.0)
    if (failed >= 0).any():
        l = int(np.argmax(failed >= 0))
        raise ValueError(f"not positive semi-definite at l = {l} (component {int(failed[l])})")
    return np.ascontiguousarray(np.stack([L[b, a] for a, b in pair_list(ncomp)]))


def lm_index(lmax):
    """(l, m) of every entry of the m-major alm layout."""
    m = np.concatenate([np.full(lmax + 1 - mm, mm) for mm in range(lmax + 1)])
    l = np.concatenate([np.arange(mm, lmax + 1) for mm in range(lmax + 1)])
    return l, m


def synalm(packed, ncomp, seed, realisation=0):
    """(ncomp, nlm) complex128: a^i_lm = sum_{j <= i} L_ij(l) z^j_lm, ascending j."""
    packed = np.asarray(packed, dtype=np.float64)
    lmax = packed.shape[-1] - 1
    L = unpack(cholesky(packed, ncomp), ncomp, lower=True)
    l, m = lm_index(lmax)
    z = [complex_normals(l, m, j, realisation, seed) for j in range(ncomp)]
    alms = np.zeros((ncomp, l.size), dtype=np.complex128)
    for i in range(ncomp):
        for j in range(i + 1):
            alms[i] = alms[i] + L[i, j][l] * z[j]
    return alms


def alm2cl_matrix(alms):
    """(N, N, lmax + 1): the spectra estimates of N alm rows."""
    n = alms.shape[0]
    lmax = (int((8 * alms.shape[1] + 1) ** 0.5 + 0.01) - 3) // 2
    l, m = lm_index(lmax)
    w = np.where(m == 0, 1.0, 2.0)
    out = np.zeros((n, n, lmax + 1))
    for a in range(n):
        for b in range(n):
            out[a, b] = np.bincount(l, weights=w * (alms[a] * alms[b].conj()).real, minlength=lmax + 1) / (2 * np.arange(lmax + 1) + 1)
    return out


def conditioned_spectra(ncomp, lmax, seed, zero_below=None):
    """Well-conditioned test matrices (N, N, lmax + 1): C_l = B_l B_l^T / (l + 1)^2, B of shape N x (N + 2) from a seeded generator.
    zero_below = {component: l0}: that component has no power (row and column zero) below l0, as a field's rows below its spin."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((lmax + 1, ncomp, ncomp + 2))
    for comp, l0 in (zero_below or {}).items():
        B[:l0, comp, :] = 0.0
    C = np.einsum("lik,ljk->ijl", B, B) / (np.arange(lmax + 1) + 1.0) ** 2
    return 0.5 * (C + C.transpose(1, 0, 2))


def assert_spectra_statistics(C, est):
    """The estimates `est` (N, N, nl) are those of Gaussian alms with spectra `C`: over the elements a <= b with Gaussian variance
    (C_aa C_bb + C_ab^2) / (2 l + 1) > 0 the standardised residuals have max |r| < 5 and |rms - 1| < 0.1; where the variance is 0
    the estimate is exactly 0.  Returns (max, rms) for the record."""
    n, nl = C.shape[0], C.shape[-1]
    res = []
    for a in range(n):
        for b in range(a, n):
            var = (C[a, a] * C[b, b] + C[a, b] ** 2) / (2 * np.arange(nl) + 1)
            dead = var == 0
            assert (est[a, b][dead] == 0).all(), f"element ({a}, {b}): non-zero estimate where the variance is 0"
            res.append((est[a, b][~dead] - C[a, b][~dead]) / np.sqrt(var[~dead]))
    res = np.concatenate(res)
    worst, rms = float(np.abs(res).max()), float(np.sqrt(np.mean(res**2)))
    print(f"standardised residuals: {res.size} elements, max {worst:.3f}, rms {rms:.4f}")
    assert worst < 5, worst
    assert abs(rms - 1) < 0.1, rms
    return worst, rms


# ---- the round-trip case shared by the host and GPU tests: {POS (spin 0), SHE (spin 2)} x 2 bins, N = 6, lmax 130 ----------------
ROUNDTRIP_FIELDS = (("POS", 1, 0), ("POS", 2, 0), ("SHE", 1, 2), ("SHE", 2, 2))  # (name, bin, spin) in the order of the components
ROUNDTRIP_LMAX = 130
ROUNDTRIP_SEED = (1 << 40) + 12345  # chosen so that the reference passes assert_spectra_statistics (test_synalm_host.py)


def field_rows(fields):
    """{(name, bin): (first row, rows, spin)}"""
    out, n = {}, 0
    for name, i, spin in fields:
        rows = 1 if spin == 0 else 2
        out[name, i] = (n, rows, spin)
        n += rows
    return out, n


def roundtrip_matrix():
    rows, n = field_rows(ROUNDTRIP_FIELDS)
    zero_below = {first + r: spin for (first, nr, spin) in rows.values() for r in range(nr) if spin}
    return conditioned_spectra(n, ROUNDTRIP_LMAX, 77, zero_below)


def matrix_to_cls(C, fields):
    """The blocks of `C` keyed (k1, k2, i1, i2) and shaped as angular_power_spectra returns them, with spin_1 / spin_2 metadata."""
    rows, _ = field_rows(fields)
    cls = {}
    for (ka, ia), (kb, ib) in combinations_with_replacement(list(rows), 2):
        (fa, na, sa), (fb, nb, sb) = rows[ka, ia], rows[kb, ib]
        block = C[fa : fa + na, fb : fb + nb].reshape(*((na,) if sa else ()), *((nb,) if sb else ()), -1).copy()
        block.dtype = np.dtype(block.dtype.str, metadata={"spin_1": sa, "spin_2": sb})
        cls[ka, kb, ia, ib] = block
    return cls


def cls_to_matrix(cls, fields):
    """The inverse of matrix_to_cls for a dict that holds every pair in field order."""
    rows, n = field_rows(fields)
    nl = next(iter(cls.values())).shape[-1]
    C = np.zeros((n, n, nl))
    for (ka, kb, ia, ib), block in cls.items():
        (fa, na, _), (fb, nb, _) = rows[ka, ia], rows[kb, ib]
        block = np.asarray(block).reshape(na, nb, nl)
        C[fa : fa + na, fb : fb + nb] = block
        if (ka, ia) != (kb, ib):
            C[fb : fb + nb, fa : fa + na] = block.transpose(1, 0, 2)
    return C
