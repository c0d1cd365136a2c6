"""Covariance kernels (csrc/hx_covariance.hip) on the device: the reference's outputs (tests/golden/reference_covariance.npz),
tile edges against numpy, the production data vector (N = 14725, n = 128; delete-2 at n = 8128), repeatability, and the chain
jackknife_cls -> jackknife_covariance -> debias_covariance -> shrink."""

import itertools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_covariance_host as th  # noqa: E402

from heracles_amd import covariance as cv  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(th.GOLDEN)


def test_golden_parity(golden):
    import heracles_amd as hx

    cls0, cls1, cls2 = th.case_a(golden)
    th.check_dict(hx.jackknife_covariance(cls1, nd=1), golden, "a/jk1", ell=True)
    th.check_dict(hx.jackknife_covariance(cls2, nd=2), golden, "a/jk2")
    th.check_dict(hx.delete2_correction(cls0, cls1, cls2), golden, "a/q")
    deb = hx.debias_covariance(hx.jackknife_covariance(cls1, nd=1), cls0, cls1, cls2)
    th.check_dict(deb, golden, "a/debias")
    gauss = hx.gaussian_covariance(cls0)
    lam = hx.shrinkage_factor(cls1, gauss)
    want = float(golden["a/lambda"])
    assert abs(lam - want) <= 1e-10 * abs(want), (lam, want)
    with np.errstate(invalid="ignore", divide="ignore"):
        th.check_dict(hx.shrink(deb, gauss, lam), golden, "a/shrink", rtol=1e-11)


@pytest.mark.parametrize("n", [2, 3, 5, 129])
@pytest.mark.parametrize("N", [1, 7, 16, 100])
def test_gram_tile_edges(n, N):
    rng = np.random.default_rng(10 * n + N)
    X = rng.standard_normal((n, N)) + 3.0
    want = th.np_gram(X, None, 0.7)
    got = cv._gram(X, None, 0.7)
    assert np.abs(got - want).max() <= 1e-13 * max(np.abs(want).max(), 1e-300)
    Y = rng.standard_normal((n, N + 37))
    want = th.np_gram(X, Y, 1.3)
    got = cv._gram(X, Y, 1.3)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def ld_shrink_sums(X, T):
    """the formula of DESIGN.md 4.7 in long double"""
    X = X.astype(np.longdouble)
    T = np.asarray(T, dtype=np.longdouble)
    n, N = X.shape
    D = X - X.mean(axis=0)
    c, f = np.longdouble((n - 1) ** 2) / n, np.longdouble(n) / (n - 1) ** 3
    G1, G22, G31 = D.T @ D, (D * D).T @ (D * D), (D**3).T @ D
    Wb, S = c / n * G1, c / (n - 1) * G1
    wd, sd = np.diag(Wb), np.diag(S)
    t = T / np.sqrt(np.outer(np.diag(T), np.diag(T)))
    cw = f * (c * c * G22 - n * Wb**2)
    ci = f * (c * c * G31 - n * wd[:, None] * Wb)
    cj = f * (c * c * G31.T - n * wd[None, :] * Wb)
    fij = np.sqrt(wd[None, :] / wd[:, None]) * ci / 2 + np.sqrt(wd[:, None] / wd[None, :]) * cj / 2
    off = ~np.eye(N, dtype=bool)
    # magnitude of the pieces that cancel in the numerator (c^2 G22 against n Wb^2, ...): the scale of its rounding error
    mag = f * (c * c * np.abs(G22) + n * Wb**2) + np.abs(t) * f * (
        np.sqrt(wd[None, :] / wd[:, None]) * (c * c * np.abs(G31) + n * np.abs(wd[:, None] * Wb))
        + np.sqrt(wd[:, None] / wd[None, :]) * (c * c * np.abs(G31.T) + n * np.abs(wd[None, :] * Wb))) / 2
    return np.sum((cw - t * fij)[off]), np.sum(((S - t * np.sqrt(np.outer(sd, sd))) ** 2)[off]), np.sum(mag[off])


@pytest.mark.parametrize("n,N", [(2, 9), (3, 15), (5, 70), (129, 130), (64, 500)])
def test_shrink_sums_tile_edges_long_double(n, N):
    rng = np.random.default_rng(n * 1000 + N)
    X = rng.standard_normal((n, N)) * (1 + np.arange(N) % 7) + 5.0
    A = rng.standard_normal((N, N))
    T = A @ A.T / N + np.diag(1.0 + rng.random(N))
    T[0, 1] += 0.01  # not symmetric: the (j, i) terms must read T[j, i]
    num, den = cv._shrink_sums(X, T)
    wn, wd, scale = ld_shrink_sums(X, T)
    # the numerator is a sum of cancelling terms (identically zero for n = 2): its error is measured against their magnitude
    assert abs(num - float(wn)) <= 1e-12 * float(scale), (num, wn, scale)
    assert abs(den - float(wd)) <= 1e-11 * float(wd)
    if abs(wn) > 1e-3 * scale:
        assert abs(num / den - float(wn / wd)) <= 1e-10 * abs(float(wn / wd))


def test_repeatable():
    rng = np.random.default_rng(7)
    X = rng.standard_normal((33, 300))
    T = np.eye(300) + 0.1
    assert cv._shrink_sums(X, T) == cv._shrink_sums(X, T)
    a, b = cv._gram(X, None, 0.5), cv._gram(X, None, 0.5)
    assert np.array_equal(a, b)


# ---- production size: the bench's key layout (10 spin-0 + 10 spin-2 maps, 31 l bins) -------------------------------------------
def bench_keys():
    maps = [("POS", i) for i in range(10)] + [("SHE", i) for i in range(10)]
    return [(a, b, i, j) for (a, i), (b, j) in itertools.combinations_with_replacement(maps, 2)]


def synthetic_samples(n, L=31, seed=0):
    import heracles_amd as hx

    rng = np.random.default_rng(seed)
    keys = bench_keys()
    shape = {k: tuple(2 for f in k[:2] if f == "SHE") + (L,) for k in keys}
    base = {k: 1.0 + rng.random(shape[k]) for k in keys}
    spin = {"POS": 0, "SHE": 2}
    out = {}
    for s in range(n):
        out[(s + 1,)] = {k: hx.Result(base[k] * (1 + 0.05 * rng.standard_normal(shape[k])), spin=(spin[k[0]], spin[k[1]]), axis=-1)
                         for k in keys}
    return out


def test_production_size_jackknife_and_shrinkage():
    import torch

    import heracles_amd as hx

    samples = synthetic_samples(128)
    first = samples[(1,)]
    lay = cv._Layout(first)
    assert lay.n == 14725
    X = lay.pack(list(samples.values()))
    cov = hx.jackknife_covariance(samples, nd=1)
    assert len(cov) == 210 * 211 // 2
    D = X - X.mean(axis=0)
    rng = np.random.default_rng(1)
    pairs = list(itertools.combinations_with_replacement(lay.keys, 2))
    for q in rng.choice(len(pairs), 200, replace=False):
        k1, k2 = pairs[q]
        blk = lay.arrange((127 / 128) * (D[:, lay.offset[k1]:lay.offset[k1] + lay.size[k1]].T @ D[:, lay.offset[k2]:lay.offset[k2] + lay.size[k2]]), k1, k2)
        key = (k1[0], k1[1], k2[0], k2[1], k1[2], k1[3], k2[2], k2[3])
        got = cov[key].array
        assert got.shape == blk.shape
        assert np.abs(got - blk).max() <= 1e-12 * np.abs(blk).max(), key
    del cov
    # a dense target on the device: T_ij = s_i s_j rho^|i - j|
    N = lay.n
    s = 1.0 + np.arange(N) % 5
    idx = torch.arange(N, device="cuda", dtype=torch.float64)
    sd = torch.from_numpy(s).cuda()
    T = (sd[:, None] * sd[None, :]) * torch.pow(0.9, (idx[:, None] - idx[None, :]).abs())
    lam = hx.shrinkage_factor(samples, T)
    lam2 = hx.shrinkage_factor(samples, T)
    assert lam == lam2
    del T, idx
    torch.cuda.empty_cache()
    # blockwise numpy restatement (rows in chunks: host memory stays under ~2 GB)
    n = 128
    c, f = (n - 1) ** 2 / n, n / (n - 1) ** 3
    ss = np.sum(D * D, axis=0)
    wd, sdg = c / n * ss, c / (n - 1) * ss
    D2, D3 = D * D, D**3
    num = den = 0.0
    ar = np.arange(N)
    for r0 in range(0, N, 1024):
        r = slice(r0, min(r0 + 1024, N))
        G1 = D[:, r].T @ D
        Wb, S = c / n * G1, c / (n - 1) * G1
        cw = f * (c * c * (D2[:, r].T @ D2) - n * Wb**2)
        ci = f * (c * c * (D3[:, r].T @ D) - n * wd[r, None] * Wb)
        cj = f * (c * c * (D[:, r].T @ D3) - n * wd[None, :] * Wb)
        fij = 0.5 * np.sqrt(wd[None, :] / wd[r, None]) * ci + 0.5 * np.sqrt(wd[r, None] / wd[None, :]) * cj
        t = np.power(0.9, np.abs(ar[r, None] - ar[None, :]))
        off = ar[r, None] != ar[None, :]
        num += np.sum(np.where(off, cw - t * fij, 0.0))
        den += np.sum(np.where(off, (S - t * np.sqrt(np.outer(sdg[r], sdg))) ** 2, 0.0))
    assert abs(lam - num / den) <= 1e-9 * abs(num / den), (lam, num / den)


def test_delete2_at_size():
    rng = np.random.default_rng(5)
    njk, N = 128, 14725
    pairs = np.array(list(itertools.combinations(range(njk), 2)), dtype=np.int32)
    m = len(pairs)
    assert m == 8128
    c0 = 1.0 + rng.random(N)
    c1 = c0 * (1 + 0.01 * rng.standard_normal((njk, N)))
    c2 = (c0 * (1 + 0.01 * rng.standard_normal((m, N), dtype=np.float64)))
    # l-major groups of the bench layout: 475 columns per l index, 31 l indices
    L, nd = 31, 475
    perm = (np.arange(nd)[None, :] * L + np.arange(L)[:, None]).reshape(-1).astype(np.int32)
    bstart = (np.arange(L + 1) * nd).astype(np.int32)
    alpha = cv._nd_alpha(m, 2)
    flat = cv._delete2_q(njk, c0, c1, c2, pairs, perm, bstart, alpha)
    assert flat.shape == (L * nd * nd,)
    for b in np.random.default_rng(6).choice(L, 3, replace=False):
        cols = perm[bstart[b]:bstart[b + 1]]
        Q = njk * c0[cols] - (njk - 1) * c1[pairs[:, 0]][:, cols] - (njk - 1) * c1[pairs[:, 1]][:, cols] + (njk - 2) * c2[:, cols]
        D = Q - Q.mean(axis=0)
        want = alpha * (D.T @ D)
        got = flat[b * nd * nd:(b + 1) * nd * nd].reshape(nd, nd)
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max(), b


def test_end_to_end_from_jackknife_cls():
    import test_gpu_jackknife as tj

    import heracles_amd as hx

    fields, maps, jk = tj._setup(np.random.default_rng(11))
    cls0 = hx.jackknife_cls(maps, None, jk, fields, nd=0)[()]
    cls1 = hx.jackknife_cls(maps, None, jk, fields, nd=1)
    cls2 = hx.jackknife_cls(maps, None, jk, fields, nd=2)
    cov = hx.jackknife_covariance(cls1, nd=1)
    deb = hx.debias_covariance(cov, cls0, cls1, cls2)
    assert set(deb) == set(cov)
    gauss = hx.gaussian_covariance(cls0)
    lam = hx.shrinkage_factor(cls1, gauss)
    # (the spin-2 spectra are zero at l < 2: zero-variance entries make the reference's factor NaN, and this one with it)
    trim = {r: {k: hx.Result(v.array[..., 2:], spin=v.spin, axis=-1) for k, v in c.items()} for r, c in cls1.items()}
    lam_trim = hx.shrinkage_factor(trim, hx.gaussian_covariance({k: hx.Result(v.array[..., 2:], spin=v.spin, axis=-1) for k, v in cls0.items()}))
    assert np.isfinite(lam_trim)
    with np.errstate(invalid="ignore", divide="ignore"):
        shrunk = hx.shrink(deb, gauss, lam)
    for key, res in shrunk.items():
        assert res.array.shape == cov[key].array.shape and tuple(res.axis) == tuple(cov[key].axis)
    # the numpy restatement of the same chain
    from unittest import mock

    with mock.patch.object(cv, "_gram", th.np_gram), mock.patch.object(cv, "_delete2_q", th.np_delete2_q), \
            mock.patch.object(cv, "_shrink_sums", th.np_shrink_sums):
        lam_np = hx.shrinkage_factor(cls1, gauss)
        lam_trim_np = hx.shrinkage_factor(trim, hx.gaussian_covariance({k: hx.Result(v.array[..., 2:], spin=v.spin, axis=-1) for k, v in cls0.items()}))
        deb_np = hx.debias_covariance(hx.jackknife_covariance(cls1, nd=1), cls0, cls1, cls2)
    assert np.isnan(lam) == np.isnan(lam_np)
    assert abs(lam_trim - lam_trim_np) <= 1e-9 * abs(lam_trim_np)
    for key in deb:
        assert np.abs(deb[key].array - deb_np[key].array).max() <= 1e-10 * max(np.abs(deb_np[key].array).max(), 1e-300)
