"""Covariance estimators of heracles_amd.covariance against the reference's outputs (tests/golden/reference_covariance.npz), with
the three kernel entry points (_gram, _delete2_q, _shrink_sums) replaced by numpy restatements: keys, shapes, axis, spin, ell
tuples, nd scaling, the l1 = l2 masking of the delete-2 correction, NaN propagation, errors and the target order rule."""

import itertools
import os

import numpy as np
import pytest

import heracles_amd as hx
from heracles_amd import covariance as cv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_covariance.npz")
SPIN = {"POS": 0, "SHE": 2}


def np_gram(X, Y=None, alpha=1.0):
    D = X - X.mean(axis=0)
    E = D if Y is None else Y - Y.mean(axis=0)
    return alpha * (D.T @ E)


def np_delete2_q(njk, c0, c1, c2, pairs, perm, bstart, alpha):
    Q = njk * c0 - (njk - 1) * c1[pairs[:, 0]] - (njk - 1) * c1[pairs[:, 1]] + (njk - 2) * c2
    D = Q[:, perm] - Q[:, perm].mean(axis=0)
    return np.concatenate([(alpha * D[:, s:e].T @ D[:, s:e]).ravel() for s, e in zip(bstart[:-1], bstart[1:])] + [np.zeros(0)])


def np_shrink_sums(X, T):
    n, N = X.shape
    D = X - X.mean(axis=0)
    c, f = (n - 1) ** 2 / n, n / (n - 1) ** 3
    G1, G22, G31 = D.T @ D, (D * D).T @ (D * D), (D**3).T @ D
    Wb, S = c / n * G1, c / (n - 1) * G1
    wd, sd = np.diag(Wb), np.diag(S)
    t = np.asarray(T) / np.sqrt(np.outer(np.diag(T), np.diag(T)))
    cw = f * (c * c * G22 - n * Wb**2)
    ci = f * (c * c * G31 - n * wd[:, None] * Wb)
    cj = f * (c * c * G31.T - n * wd[None, :] * Wb)
    fij = 0.5 * np.sqrt(wd[None, :] / wd[:, None]) * ci + 0.5 * np.sqrt(wd[:, None] / wd[None, :]) * cj
    off = ~np.eye(N, dtype=bool)
    num = np.sum((cw - t * fij)[off])
    den = np.sum(((S - t * np.sqrt(np.outer(sd, sd))) ** 2)[off])
    return num, den


@pytest.fixture
def kernels(monkeypatch):
    monkeypatch.setattr(cv, "_gram", np_gram)
    monkeypatch.setattr(cv, "_delete2_q", np_delete2_q)
    monkeypatch.setattr(cv, "_shrink_sums", np_shrink_sums)
    monkeypatch.setattr(cv, "_hbm_budget", lambda: None)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def parse(s):
    a, b, i, j = s.split("|")
    return (a, b, int(i), int(j))


def ks(key):
    return "|".join(str(k) for k in key)


def spectra(g, case, which, **ell_kw):
    """{key: Result} of the stored spectra; which = cls0, or (cls1 / cls2, sample index)"""
    out = {}
    for s in g[f"{case}/keys"]:
        key = parse(s)
        arr = np.array(g[f"{case}/{which[0]}/{s}"])
        if which[1] is not None:
            arr = np.array(arr[which[1]])
        if which[0] == "cls0":
            hx.update_metadata(arr, nside=8, **({"bias": float(g[f"{case}/bias/{s}"])} if key[0] == key[1] and key[2] == key[3] else {}))
        out[key] = hx.Result(arr, spin=(SPIN[key[0]], SPIN[key[1]]), axis=-1, **ell_kw)
    return out


def case_a(g):
    cls0 = spectra(g, "a", ("cls0", None))
    cls1 = {(int(k),): spectra(g, "a", ("cls1", n)) for n, k in enumerate(g["a/regions1"])}
    cls2 = {tuple(int(x) for x in kk): spectra(g, "a", ("cls2", n)) for n, kk in enumerate(g["a/regions2"])}
    return cls0, cls1, cls2


def check_dict(got, g, tag, rtol=1e-12, ell=False):
    want_keys = sorted(k[len(tag) + 1:] for k in g.files if k.startswith(tag + "/") and k.count("/") == tag.count("/") + 1)
    assert sorted(ks(k) for k in got) == want_keys
    for key, res in got.items():
        want = g[f"{tag}/{ks(key)}"]
        assert res.array.shape == want.shape, key
        scale = np.nanmax(np.abs(want)) if np.any(np.isfinite(want)) else 1.0
        np.testing.assert_array_equal(np.isnan(res.array), np.isnan(want), err_msg=str(key))
        np.testing.assert_allclose(np.nan_to_num(res.array), np.nan_to_num(want), rtol=0, atol=rtol * max(scale, 1e-300), err_msg=str(key))
        assert tuple(res.spin) == tuple(g[f"{tag}/spin/{ks(key)}"]), key
        assert tuple(res.axis) == tuple(g[f"{tag}/axis/{ks(key)}"]), key
        if ell:
            for n, e in enumerate(res.ell):
                np.testing.assert_array_equal(e, g[f"{tag}/ell{n}/{ks(key)}"])


def test_jackknife_covariance_nd1_nd2(kernels, golden):
    cls0, cls1, cls2 = case_a(golden)
    check_dict(hx.jackknife_covariance(cls1, nd=1), golden, "a/jk1", ell=True)
    check_dict(hx.jackknife_covariance(cls2, nd=2), golden, "a/jk2")


def test_delete2_and_debias(kernels, golden):
    cls0, cls1, cls2 = case_a(golden)
    Q = hx.delete2_correction(cls0, cls1, cls2)
    check_dict(Q, golden, "a/q")
    for res in Q.values():  # only the l1 = l2 diagonal survives
        L = res.array.shape[-1]
        assert not np.any(res.array[..., ~np.eye(L, dtype=bool)])
    cov1 = hx.jackknife_covariance(cls1, nd=1)
    check_dict(hx.debias_covariance(cov1, cls0, cls1, cls2), golden, "a/debias")


def test_gaussian_shrinkage_and_shrink(kernels, golden):
    cls0, cls1, cls2 = case_a(golden)
    gauss = hx.gaussian_covariance(cls0)
    check_dict(gauss, golden, "a/gauss", rtol=0, ell=True)
    lam = hx.shrinkage_factor(cls1, gauss)
    assert abs(lam - float(golden["a/lambda"])) <= 1e-10 * abs(float(golden["a/lambda"]))
    # the dense target in data-vector order is the same factor
    dense = hx.flatten(gauss, order=list(next(iter(cls1.values()))))
    assert hx.shrinkage_factor(cls1, dense) == lam
    deb = hx.debias_covariance(hx.jackknife_covariance(cls1, nd=1), cls0, cls1, cls2)
    with np.errstate(invalid="ignore", divide="ignore"):
        shrunk = hx.shrink(deb, gauss, float(golden["a/lambda"]))
    check_dict(shrunk, golden, "a/shrink", rtol=1e-12)
    assert any(np.isnan(r.array).any() for r in shrunk.values())  # negative diagonals of the debiased covariance: NaN as in the reference


def test_binned_results_ell_tuples(kernels, golden):
    g = golden
    ell_kw = {k: g[f"b/{k}"] for k in ("ell", "lower", "upper", "weight")}
    cls0 = spectra(g, "b", ("cls0", None), **ell_kw)
    cls1 = {(n + 1,): spectra(g, "b", ("cls1", n), **ell_kw) for n in range(g[f"b/cls1/{g['b/keys'][0]}"].shape[0])}
    check_dict(hx.jackknife_covariance(cls1, nd=1), g, "b/jk1", ell=True)
    check_dict(hx.gaussian_covariance(cls0), g, "b/gauss", rtol=0, ell=True)
    for res in hx.jackknife_covariance(cls1, nd=1).values():
        assert res.lower is None and res.upper is None and res.weight is None


def test_sample_covariance_and_errors(kernels, golden):
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal((7, 3, 4)), rng.standard_normal((7, 5))
    np.testing.assert_allclose(hx.sample_covariance(x), np.cov(x.reshape(7, -1), rowvar=False).reshape(3, 4, 3, 4), rtol=1e-12)
    np.testing.assert_allclose(hx.sample_covariance(x, y), np.cov(x.reshape(7, -1), y, rowvar=False)[:12, 12:].reshape(3, 4, 5), rtol=1e-12)
    with pytest.raises(ValueError):
        hx.sample_covariance(x, y[:6])
    cls0, cls1, cls2 = case_a(golden)
    with pytest.raises(ValueError):
        hx.jackknife_covariance(cls1, nd=3)
    assert hx.jackknife_covariance({(1,): cls1[(1,)]}) == {}
    broken = dict(cls1)
    broken[(3,)] = {k: v for n, (k, v) in enumerate(cls1[(3,)].items()) if n}
    with pytest.raises(ValueError):
        hx.jackknife_covariance(broken)
    with pytest.raises(ValueError):
        hx.shrinkage_factor(cls1, np.eye(3))


def test_memory_guard(kernels, golden, monkeypatch):
    cls0, cls1, cls2 = case_a(golden)
    monkeypatch.setattr(cv, "_hbm_budget", lambda: 1000)
    called = []
    monkeypatch.setattr(cv, "_gram", lambda *a, **k: called.append(1))
    with pytest.raises(ValueError, match="device memory"):
        hx.jackknife_covariance(cls1)
    assert not called


def test_target_order_is_the_data_order(kernels, golden):
    """A target dict whose keys come in another order gives the same factor: it is flattened in the data vector's order."""
    cls0, cls1, cls2 = case_a(golden)
    gauss = hx.gaussian_covariance(cls0)
    lam = hx.shrinkage_factor(cls1, gauss)
    shuffled = dict(reversed(list(gauss.items())))
    assert hx.shrinkage_factor(cls1, shuffled) == lam
    # and the samples' key order defines it: reordering the samples' keys reorders the target with them
    keys = list(next(iter(cls1.values())))
    perm = keys[::-1]
    cls1r = {r: {k: s[k] for k in perm} for r, s in cls1.items()}
    assert abs(hx.shrinkage_factor(cls1r, gauss) - lam) <= 1e-12 * abs(lam)


def test_impose_correlation_nan():
    a = {("A", "A", "A", "A", 0, 0, 0, 0): hx.Result(np.array([[1.0, 0.5], [0.5, -1.0]]), axis=(0, 1))}
    b = {("A", "A", "A", "A", 0, 0, 0, 0): hx.Result(np.array([[4.0, 1.0], [1.0, 9.0]]), axis=(0, 1))}
    with np.errstate(invalid="ignore"):
        c = hx.impose_correlation(a, b)[("A", "A", "A", "A", 0, 0, 0, 0)].array
    assert c[0, 0] == 4.0 and np.isnan(c[0, 1]) and np.isnan(c[1, 1])


def test_get_cl_symmetric_lookup():
    arr = np.arange(12.0).reshape(2, 2, 3)
    cls = {("SHE", "SHE", 0, 1): hx.Result(arr, spin=(2, 2), axis=-1), ("POS", "SHE", 1, 0): hx.Result(arr[0], spin=(0, 2), axis=-1)}
    r = hx.get_cl(("SHE", "SHE", 1, 0), cls)
    np.testing.assert_array_equal(r.array, arr.transpose(1, 0, 2))
    r = hx.get_cl(("SHE", "POS", 0, 1), cls)
    assert tuple(r.spin) == (2, 0)
    np.testing.assert_array_equal(r.array, arr[0])
    with pytest.raises(KeyError):
        hx.get_cl(("POS", "POS", 0, 0), cls)


def test_flatten_layout():
    cls = {("POS", "POS", 0, 0): hx.Result(np.arange(3.0), spin=(0, 0), axis=-1),
           ("POS", "SHE", 0, 0): hx.Result(np.arange(6.0).reshape(2, 3) + 10, spin=(0, 2), axis=-1)}
    np.testing.assert_array_equal(hx.flatten(cls), np.concatenate([np.arange(3.0), np.arange(6.0) + 10]))
    lay = cv._Layout(cls)
    assert lay.n == 9 and [lay.offset[k] for k in cls] == [0, 3]
    for (k1, k2) in itertools.combinations_with_replacement(cls, 2):
        assert lay.block(np.arange(81.0).reshape(9, 9), k1, k2).shape[-2:] == (3, 3)
