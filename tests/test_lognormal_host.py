"""Host side of the lognormal mocks (no GPU): the shared Jacobi header compiled for the host (plain and with sanitizers), the numpy
restatement (tests/lognormal_reference.py) pinned on closed forms, and the argument checks of the Python layer, which raise before
any library call."""

import os
import subprocess

import numpy as np
import pytest

import lognormal_reference as lr
import synalm_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "csrc", "test_lognormal_host.cpp")


def test_jacobi_header_on_the_host(tmp_path):
    exe = tmp_path / "t_lognormal"
    subprocess.check_call(["g++", "-O2", "-std=c++17", SOURCE, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout


def test_jacobi_header_under_sanitizers(tmp_path):
    exe = tmp_path / "t_lognormal_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SOURCE, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


# ---- the reference, pinned on its own -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam,g0", [(1.0, 0.3), (0.05, 2.0), (2.5, 1e-3)])
def test_reference_constant_correlation_closed_form(lam, g0):
    """xi_G constant (G_0 alone): C_0 = 4 pi lambda^2 expm1(G_0 / 4 pi), nothing else."""
    lmax = 12
    x, w = lr.gl_nodes(2 * lmax + 2)
    G = np.zeros((1, 1, lmax + 1))
    G[0, 0, 0] = g0
    C, _ = lr.convert(G, [lam], x, w, inverse=True)
    want = 4 * np.pi * lam**2 * np.expm1(g0 / (4 * np.pi))
    assert abs(float(C[0, 0, 0]) - want) <= 8 * 2.0**-53 * want
    assert np.abs(C[0, 0, 1:].astype(np.float64)).max() <= 1e-15 * want
    back, _ = lr.convert(C.astype(np.float64), [lam], x, w)
    assert abs(float(back[0, 0, 0]) - g0) <= 1e-14 * g0


def test_reference_round_trip_within_its_bound():
    """realised(gaussian(C)) = C.  The logarithm is not band-limited, so this holds when G keeps every multipole the nodes resolve
    (nl = nodes): the transforms are then exact inverses of each other on the nodes.  Cut at lmax it does not -- which is why
    lognormal_realised_cls exists; the size of that effect is printed."""
    lmax, lam = 40, np.array([1.0, 0.05, 2.5, 0.0, 0.0, 0.0])
    var = np.where(lam > 0, lam**2 * np.expm1([0.5, 0.3, 0.1, 0, 0, 0]), [0, 0, 0, 0.2, 0.3, 0.1])
    C = lr.smooth_spectra(6, lmax, 5, var)
    nodes = 2 * lmax + 2
    x, w = lr.gl_nodes(nodes)
    full = np.zeros((6, 6, nodes))
    full[:, :, : lmax + 1] = C
    G, _ = lr.convert(full, lam, x, w)
    s2 = [lr.sigma2(G[i, i].astype(np.float64)) for i in range(3)]
    assert 0.45 < s2[0] < 0.55 and 0.25 < s2[1] < 0.35 and 0.08 < s2[2] < 0.12, s2
    back, bound = lr.convert(G, lam, x, w, inverse=True)  # (long double all the way)
    err = np.abs((back - full).astype(np.float64))
    ln = np.ix_(lam > 0, lam > 0)
    print("round trip: max error / bound", (err[ln] / bound[ln]).max(), "; max error", err.max(), "of", np.abs(C).max())
    # the nodes and weights themselves are rounded to float64, which moves P_l(x_k) by up to l^2 2^-53: the transforms are inverses
    # of each other to that, on top of the bound of the sums
    assert (err[ln] <= bound[ln] + 4 * nodes**2 * 2.0**-53 * np.abs(C[ln]).max()).all()
    mixed = np.ix_(lam > 0, lam == 0)
    assert (err[mixed] <= 2 * 2.0**-53 * np.abs(full[mixed])).all()
    gg = np.ix_(lam == 0, lam == 0)
    assert (back[gg] == full[gg]).all() and (G[gg] == full[gg]).all()
    cut, _ = lr.convert(G[:, :, : lmax + 1].astype(np.float64), lam, x, w, inverse=True)
    print("cut at lmax: max |realised - C| / max |C| =", float(np.abs(cut - C)[ln].max() / np.abs(C[ln]).max()))


def test_reference_log_argument_error_names_pair_and_node():
    lmax = 6
    x, w = lr.gl_nodes(2 * lmax + 2)
    C = np.zeros((1, 1, lmax + 1))
    C[0, 0, 1] = 4 * np.pi  # xi = 3 cos(theta) / ... reaches -lambda^2 near x = -1 for a small shift
    with pytest.raises(ValueError, match=r"pair \(0, 0\).*node 0"):
        lr.convert(C, [0.5], x, w)


def test_reference_nearest_psd_properties():
    n, nl = 5, 9
    C = sr.conditioned_spectra(n, nl - 1, 3)
    bad = C.copy()
    # push one eigenvalue of l = 4 below zero
    lamb, V = np.linalg.eigh(bad[:, :, 4])
    bad[:, :, 4] -= 1.5 * lamb[0] * np.outer(V[:, 0], V[:, 0])
    bad[:, :, 4] = 0.5 * (bad[:, :, 4] + bad[:, :, 4].T)
    bad[2, :, 6] = bad[:, 2, 6] = 0.0  # a zero row
    out, change, repaired = lr.nearest_psd(bad)
    assert repaired.tolist() == [l == 4 for l in range(nl)]
    keep = np.arange(nl) != 4
    assert (out[:, :, keep] == bad[:, :, keep]).all() and (change[keep] == 0).all() and change[4] > 0
    assert np.linalg.eigvalsh(out[:, :, 4]).min() > 0
    sr.cholesky(sr.pack(out), n)  # passes the factor of 4.15
    with pytest.raises(ValueError, match="l = 4"):
        sr.cholesky(sr.pack(bad), n)
    neg = C.copy()
    neg[1, 1, 7] = -1.0
    neg[0, 3, 3] = np.nan
    with pytest.raises(ValueError, match="l = 3"):
        lr.nearest_psd(neg)


def test_indefinite_set_is_indefinite_after_gaussianisation():
    """The set of the regularize test: every Gaussianised matrix has a negative eigenvalue, the factor of 4.15 refuses it, and the
    repaired set passes."""
    C, lam = lr.indefinite_targets()
    lmax = C.shape[2] - 1
    x, w = lr.gl_nodes(2 * lmax + 2)
    G = lr.convert(C, lam, x, w)[0].astype(np.float64)
    worst = max(np.linalg.eigvalsh(G[:, :, l] / G[0, 0, l]).min() for l in range(lmax + 1))
    assert worst < -0.01
    with pytest.raises(ValueError, match="not positive semi-definite at l = 0"):
        sr.cholesky(sr.pack(G), 3)
    out, change, repaired = lr.nearest_psd(G)
    assert repaired.all() and (change > 0.01).all() and (change < 0.02).all()
    L = sr.unpack(sr.cholesky(sr.pack(out), 3), 3, lower=True)
    assert (np.einsum("iil->il", L) > 0).all()


def test_statistical_experiment_on_the_host(oracle):
    """The experiment of tests/test_gpu_lognormal.py::test_driver_statistics with the oracle's transforms and the numpy restatement, on
    the same Philox draws: the reference alone stays within the conditions (measured: max |z| = 2.64, rms z = 0.976 at n = 200)."""
    nside, lmax, n = lr.STAT_NSIDE, lr.STAT_LMAX, lr.STAT_N
    C, lam = lr.statistical_targets(), lr.STAT_SHIFTS
    x, w = lr.gl_nodes(2 * lmax + 2)
    G = lr.convert(C, lam, x, w)[0].astype(np.float64)
    s2 = [lr.sigma2(G[0, 0]), lr.sigma2(G[1, 1])]
    assert 0.09 < s2[0] < 0.11 and 0.09 < s2[1] < 0.11
    expected = lr.convert(G, lam, x, w, inverse=True)[0].astype(np.float64)
    packed, iu = sr.pack(G), np.triu_indices(4)
    est = np.empty((n, 10, lmax + 1))
    for r in range(n):
        a = sr.synalm(packed, 4, lr.STAT_SEED, r)
        X = lr.maps(oracle.alm2map(a[:2], nside, lmax, 0), s2, lam[:2])
        assert X[0].min() >= -1.0 and X[1].min() >= -0.3
        qu = oracle.alm2map(a[2:], nside, lmax, 2)
        b = np.concatenate([oracle.map2alm(X, nside, lmax, 0, niter=3), oracle.map2alm(qu, nside, lmax, 2, niter=3)])
        est[r] = sr.alm2cl_matrix(b)[iu]
    _, zmax, zrms = lr.z_scores(est[:, :, lr.STAT_ELLS], expected[iu][:, lr.STAT_ELLS])
    print(f"host experiment, n = {n}: max |z| = {zmax:.2f}, rms z = {zrms:.3f}")
    assert zmax <= 6 and 0.8 <= zrms <= 1.2


def test_reference_maps_lower_bound():
    g = np.array([[-800.0, -1.0, 0.0, 1.0, 30.0]])
    out = lr.maps(g, 0.1, 0.3)
    assert out.min() == -0.3 and (out >= -0.3).all() and out[0, 2] == 0.3 * np.expm1(-0.05)


# ---- the Python layer: argument checks before any library call ---------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    from heracles_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "ensure_init", boom)


def _spin2(block):
    block = np.array(block, dtype=float)
    block.dtype = np.dtype(block.dtype.str, metadata={"spin_1": 2, "spin_2": 2})
    return block


def _setup():
    import heracles_amd as hx

    nl = 9
    m = hx.HipHealpixMapper(4, nl - 1, deconvolve=False)
    fields = {"P": hx.Positions(m, "ra", "dec"), "K": hx.ScalarField(m, "ra", "dec", "k"), "G": hx.Shears(m, "ra", "dec", "g1", "g2")}
    ee = np.zeros((2, 2, nl))
    ee[0, 0] = ee[1, 1] = 1.0
    cls = {("P", "P", 0, 0): np.ones(nl), ("K", "K", 0, 0): np.ones(nl), ("G", "G", 0, 0): _spin2(ee)}
    return hx, fields, cls


def test_shift_errors(no_library):
    hx, fields, cls = _setup()
    with pytest.raises(ValueError, match="spin"):
        hx.lognormal_gaussian_cls(cls, {"G": 1.0})
    with pytest.raises(ValueError, match="shift > 0"):
        hx.lognormal_gaussian_cls(cls, {"P": 0.0})
    with pytest.raises(ValueError, match="shift > 0"):
        hx.lognormal_realised_cls(cls, {("P", 0): -1.0})
    with pytest.raises(ValueError, match="names no field"):
        hx.lognormal_gaussian_cls(cls, {"Q": 1.0})
    with pytest.raises(ValueError, match="names no field"):
        hx.lognormal_maps(fields, cls, {("P", 1): 1.0}, seed=1)
    with pytest.raises(ValueError, match="spin"):
        hx.lognormal_maps(fields, cls, {"G": 1.0}, seed=1)
    with pytest.raises(ValueError, match="nodes"):
        hx.lognormal_gaussian_cls(cls, {"P": 1.0}, nodes=5)


def test_driver_errors(no_library):
    hx, fields, cls = _setup()
    with pytest.raises(ValueError, match="regularize"):
        hx.lognormal_maps(fields, cls, {"P": 1.0}, seed=1, regularize="nearest")
    with pytest.raises(ValueError, match="unknown field name"):
        hx.lognormal_maps({"P": fields["P"]}, cls, {"P": 1.0}, seed=1)
    with pytest.raises(ValueError, match="must not appear in cls"):
        hx.lognormal_maps(fields, cls, {"K": 1.0}, seed=1, convergence={"G": "K"})
    scalar = {k: v for k, v in cls.items() if k[0] != "G"}
    with pytest.raises(ValueError, match="lognormal spin-0 field"):
        hx.lognormal_maps(fields, scalar, {"P": 1.0}, seed=1, convergence={"G": "K"})  # K has no shift
    with pytest.raises(ValueError, match="spin-2 field"):
        hx.lognormal_maps(fields, {("K", "K", 0, 0): cls["K", "K", 0, 0]}, {"K": 1.0}, seed=1, convergence={"P": "K"})
    other = dict(fields, G=hx.Shears(hx.HipHealpixMapper(8, 8, deconvolve=False), "ra", "dec", "g1", "g2"))
    with pytest.raises(ValueError, match="differ in nside or lmax"):
        hx.lognormal_maps(other, scalar, {"K": 1.0}, seed=1, convergence={"G": "K"})


def test_nearest_psd_argument_errors(no_library):
    hx, _, _ = _setup()
    with pytest.raises(ValueError, match="packed upper triangle"):
        hx.nearest_psd_cls(np.ones((4, 5)))
    with pytest.raises(ValueError, match="at most 64"):
        hx.nearest_psd_cls(np.ones((65 * 66 // 2, 2)))
    with pytest.raises(ValueError, match="floor"):
        hx.nearest_psd_cls(np.ones((3, 5)), floor=1.5)
    with pytest.raises(ValueError, match="no auto-spectrum"):
        hx.nearest_psd_cls({("A", "B", 0, 0): np.ones(4)})


def test_constants_restated_in_python_match_the_kernel():
    import re

    from heracles_amd import lognormal

    text = open(os.path.join(ROOT, "heracles_amd", "csrc", "hx_lognormal.hip")).read()
    for name, value in (("PSD_MAXN", lognormal.PSD_MAX_COMPONENTS), ("PSD_SWEEPS", lognormal.PSD_SWEEPS)):
        assert re.search(rf"constexpr int {name} = (\d+);", text).group(1) == str(value)
    assert lognormal.default_psd_floor(30) == 64 * 900 * 2.0**-52
    f = lognormal.shear_factor(4)
    assert (f[:2] == 0).all() and f[2] == np.sqrt(4 * 1 / (2 * 3)) and f[4] == np.sqrt(6 * 3 / (4 * 5))
