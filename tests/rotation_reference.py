"""numpy restatement of the rotation of alms; not a test.  tests/test_rotation_host.py pins it on its own through the
defining identity f'(n) = f(R^-1 n), tests/test_gpu_rotate_alm.py holds ``hx.rotate_alm`` against it.

R = Rz(phi) Ry(theta) Rz(psi) on column vectors, a'_lm = sum_m' exp(-i m phi) d^l_mm'(theta) exp(-i m' psi) a_lm' with
d^l(theta) = exp(-i theta J_y) in the Condon-Shortley basis and a_l,-m = (-1)^m conj(a_lm).  The alm layout is the project's:
m-major, idx(l, m) = m (2 lmax + 1 - m) / 2 + l."""

import functools

import numpy as np


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
