"""HEALPix pixel quadrature weights computed on the GPU (``compute_pixel_weights`` / ``hx_pixel_weights_solve``), pinned from first
principles: with the weights of (nside, lmax <= 3 nside / 2) the round trip ``map2alm(alm2map(a), niter=0)`` returns ``a`` to
rounding, the compressed vector is the minimum-norm solution of the dense constraint system built with the CPU oracle, and the
result has the layout of healpy's weight files (expansion, file round trip, mapper)."""

import types
import warnings

import numpy as np
import pytest


pytestmark = pytest.mark.gpu


def random_alms(rng, lmax, spin, n):
    """n random alms in the library's layout (m-major): real for m = 0, zero below l = spin."""
    nlm = (lmax + 1) * (lmax + 2) // 2
    a = rng.standard_normal((n, nlm)) + 1j * rng.standard_normal((n, nlm))
    a[:, : lmax + 1] = a[:, : lmax + 1].real
    for m in range(min(spin, lmax + 1)):
        i0 = m * (2 * lmax + 1 - m) // 2
        a[:, i0 + m : i0 + min(spin, lmax + 1)] = 0.0
    return a


@pytest.fixture(scope="module")
def solved():
    """(full-sky weights, compressed values, info) of (nside, 3 nside // 2), computed once per size for the whole module."""
    from heracles_amd import weights as hw

    got = {}

    def get(nside):
        if nside not in got:
            w, info = hw.compute_pixel_weights(nside, info=True)
            got[nside] = (w, hw.compute_pixel_weights(nside, compressed=True), info)
        return got[nside]

    return get


@pytest.mark.parametrize("spin", [0, 2, 1])
@pytest.mark.parametrize("nside", [8, 16, 32, 6])
def test_round_trip_is_exact_with_computed_weights(solved, nside, spin):
    """Random alms -> alm2map -> map2alm(niter=0).  With the computed weights the error is at most 1e-10 max|alm| (the suite's 1e-11
    transform parity bound plus a decade; a CPU prototype of the solve gives <= 7e-15 at these sizes); with unit weights it exceeds
    1e-3 (prototype: 3.4e-3 .. 8.8e-3), so the test tells the two apart.  Spin 1 runs the run-time-spin sweeps."""
    import heracles_amd as hx

    lmax = 3 * nside // 2
    w, _, info = solved(nside)
    assert w.shape == (12 * nside**2,) and isinstance(w, np.ndarray)
    rng = np.random.default_rng(100 * nside + spin)
    a = random_alms(rng, lmax, spin, 2 if spin else 1)
    plan = hx.get_plan(nside, lmax)
    maps = plan.alm2map(a, spin)
    scale = np.abs(a).max()
    err_w = np.abs(plan.map2alm(maps, spin, pix_weights=w, niter=0) - a).max() / scale
    err_1 = np.abs(plan.map2alm(maps, spin, niter=0) - a).max() / scale
    print(f"nside {nside} spin {spin}: computed weights {err_w:.3e}, unit weights {err_1:.3e}, {info}")
    assert err_w <= 1e-10
    assert err_1 > 1e-3


@pytest.mark.parametrize("nside", [8, 16])
def test_compressed_vector_is_the_minimum_norm_solution(oracle, solved, nside):
    """The dense system S x = r with the oracle: column j is map2alm_{unit weights, 2 lmax} of the expansion of e_j (without the
    ``1 +``), rows are the real parts of the modes the symmetries leave (L even, M = 0 mod 4), r = sqrt(4 pi) e_00 - (the same
    modes of map2alm(1)).  numpy's minimum-norm least-squares solution against the GPU's conjugate gradients: 1e-9 max|x| (the
    prototype's own CG and lstsq differ by about 1e-12)."""
    lmax = 3 * nside // 2
    L = 2 * lmax
    n = (nside + 1) * (3 * nside + 1) // 4
    cols = np.stack([oracle.expand_full_weights(nside, e) - 1.0 for e in np.eye(n)])
    alm = oracle.map2alm(np.concatenate([cols, np.ones((1, 12 * nside**2))]), nside, L, spin=0)
    rows = np.array([m * (2 * L + 1 - m) // 2 + l for m in range(0, L + 1, 4) for l in range(m, L + 1) if l % 2 == 0])
    S = alm[:n, rows].real.T
    r = -alm[n, rows].real
    r[0] += np.sqrt(4.0 * np.pi)
    assert rows[0] == 0
    ref = np.linalg.lstsq(S, r, rcond=1e-12)[0]
    x = solved(nside)[1]
    err = np.abs(x - ref).max() / np.abs(ref).max()
    print(f"nside {nside}: |x_gpu - x_lstsq| / max|x| = {err:.3e}, lstsq residual {np.abs(S @ ref - r).max():.3e}")
    assert err <= 1e-9


def test_layout_expansion_repeatability_and_file_round_trip(solved, tmp_path):
    import heracles_amd as hx
    from heracles_amd import weights as hw

    nside, lmax = 16, 24
    w, x, _ = solved(nside)
    assert x.shape == (hw.compressed_size(nside),)
    np.testing.assert_array_equal(hw.expand_pixel_weights(nside, x), w)
    dev = hw.compute_pixel_weights(nside, device="cuda")
    assert dev.is_cuda
    np.testing.assert_array_equal(dev.cpu().numpy(), w)
    # a second solve, not the cached result: the same bits
    hx.release_caches()
    x2 = hw.compute_pixel_weights(nside, compressed=True)
    np.testing.assert_array_equal(x2, x)
    # through a file in healpy's layout and a mapper with a data path: the alms of pixel_weights="compute"
    (tmp_path / "full_weights").mkdir()
    hw.write_compressed_weights(tmp_path / "full_weights" / hw.weights_filename(nside), nside, x)
    m = np.random.default_rng(3).standard_normal(12 * nside**2)
    from_file = hx.HipHealpixMapper(nside, lmax, deconvolve=False, niter=0, datapath=tmp_path).transform(m)
    computed = hx.HipHealpixMapper(nside, lmax, deconvolve=False, niter=0, pixel_weights="compute").transform(m)
    np.testing.assert_array_equal(np.asarray(computed), np.asarray(from_file))


def test_mapper_computes_its_weights_without_a_warning(oracle, solved):
    import heracles_amd as hx

    nside, lmax = 16, 24
    w = solved(nside)[0]
    rng = np.random.default_rng(17)
    npix = 12 * nside**2
    a = rng.standard_normal(npix)
    s = rng.standard_normal((2, npix))
    mapper = hx.HipHealpixMapper(nside, lmax, deconvolve=False, niter=0, pixel_weights="compute")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        alm = mapper.transform(a)
        alm2 = mapper.transform(s, spin=2)
    np.testing.assert_array_equal(mapper.pixel_weights.cpu().numpy(), w)  # computed once, kept
    ref = oracle.map2alm(a[None], nside, lmax, spin=0, pix_weights=w)[0]
    np.testing.assert_allclose(alm, ref, atol=1e-11 * np.abs(ref).max())
    ref2 = oracle.map2alm(s, nside, lmax, spin=2, pix_weights=w)
    np.testing.assert_allclose(alm2, ref2, atol=1e-11 * np.abs(ref2).max())
    # region_alms computes them itself (through _load_weights) when it runs before any transform
    fresh = hx.HipHealpixMapper(nside, lmax, deconvolve=False, niter=0, pixel_weights="compute")
    fields = {"A": types.SimpleNamespace(spin=0, mapper_or_error=fresh, mask=None),
              "S": types.SimpleNamespace(spin=2, mapper_or_error=fresh, mask=None)}
    am = a.copy()
    am.dtype = np.dtype(am.dtype, metadata={"spin": 0, "nside": nside})
    sm = s.copy()
    sm.dtype = np.dtype(sm.dtype, metadata={"spin": 2, "nside": nside})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        full = hx.region_alms(fields, {("A", 0): am, ("S", 0): sm}, 1.0 + (np.arange(npix) % 3)).full()
    assert not isinstance(fresh.pixel_weights, str)
    np.testing.assert_array_equal(full["A", 0].numpy(), np.asarray(alm))
    np.testing.assert_array_equal(full["S", 0].numpy(), np.asarray(alm2))
    with pytest.raises(ValueError):
        hx.HipHealpixMapper(nside, lmax, deconvolve=False, pixel_weights="healpy").transform(a)


def test_stopping_rules(solved):
    from heracles_amd import weights as hw

    nside = 32
    converged = solved(nside)[2]
    assert converged["rel_gradient"] <= 1e-12
    with pytest.warns(RuntimeWarning, match="epsilon"):
        w, early = hw.compute_pixel_weights(nside, itmax=5, info=True)
    assert early["iterations"] == 5
    assert early["max_residual"] > converged["max_residual"]
    assert w.shape == (12 * nside**2,)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loose = hw.compute_pixel_weights(nside, epsilon=1e-6, info=True)[1]
    print(f"nside {nside}: converged {converged}, itmax=5 {early}, epsilon=1e-6 {loose}")
    assert loose["iterations"] < converged["iterations"]
    assert loose["rel_gradient"] <= 1e-6


def test_library_refuses_bad_arguments():
    import ctypes

    import heracles_amd as hx

    L = hx._lib.load()
    x = np.empty(hx.weights.compressed_size(8))
    solve = lambda plan, lmax, eps=1e-12, itmax=10, out=x: L.hx_pixel_weights_solve(plan._h if plan else None, lmax, eps, itmax, hx._lib.ptr(out),
                                                                                  None, None, None)
    p24, p26 = hx.get_plan(8, 24), hx.get_plan(8, 26)
    assert solve(None, 12) == hx._lib.HX_ERR_ARG
    assert solve(p24, 13) == hx._lib.HX_ERR_ARG          # the plan is not that of 2 lmax
    assert solve(p26, 13) == hx._lib.HX_ERR_ARG          # lmax > 3 nside / 2
    assert b"3 nside" in L.hx_last_error() or b"lmax" in L.hx_last_error()
    assert solve(p24, 12, eps=-1.0) == hx._lib.HX_ERR_ARG
    assert solve(p24, 12, itmax=-1) == hx._lib.HX_ERR_ARG
    assert solve(p24, 12, out=None) == hx._lib.HX_ERR_ARG
    it = ctypes.c_int(-1)
    assert L.hx_pixel_weights_solve(p24._h, 12, 1e-12, 3, hx._lib.ptr(x), ctypes.byref(it), None, None) == 0 and it.value == 3
    # the plan is left as it was: an ordinary transform on it still covers every order
    m = np.random.default_rng(1).standard_normal(12 * 64)
    alm = p24.map2alm(m)
    assert np.abs(alm[p24.nlm - 1]) > 0 and np.abs(alm[26:50]).max() > 0  # (orders 1 and 24)
