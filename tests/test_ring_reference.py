"""The ring-stage reference of tests/ring_reference.py against the oracle and against an extended-precision direct DFT: the
GPU ring-stage tests (test_gpu_ring_stage.py) rely on it at bounds of a few 1e-15, so it must be at least ten times tighter."""

import numpy as np
import pytest

from ring_reference import ring_dft_direct_ld, ring_pair_geometry, ring_spectra_ms, ring_spectra_ref


@pytest.mark.parametrize("nside", [1, 2, 3, 12, 64, 4096])
def test_geometry_equals_oracle(oracle, nside):
    geo = ring_pair_geometry(nside)
    rps = range(2 * nside) if nside <= 64 else sorted({0, 1, 2, 63, 64, 1000, nside - 2, nside - 1, nside, nside + 1, nside + 2, 5000,
                                                       2 * nside - 2, 2 * nside - 1})
    for rp in rps:
        i = rp + 1
        sp, nphi, z, sth, phi0 = oracle.ring_info(nside, i)
        assert (geo["startN"][rp], geo["nphi"][rp]) == (sp, nphi), rp
        assert bool(geo["shifted"][rp]) == (phi0 != 0.0), rp
        assert geo["phi0"][rp] == phi0, rp
        if i == 2 * nside:
            assert geo["startS"][rp] == -1
        else:
            spS, nphiS, zS, _, phi0S = oracle.ring_info(nside, 4 * nside - i)
            assert (geo["startS"][rp], nphiS, phi0S) == (spS, nphi, phi0), rp
            assert zS == -z


@pytest.mark.parametrize("n", [4, 12, 28, 4 * 7, 4 * 31, 4 * 255, 3 * 64, 3 * 1024, 4 * 97, 4 * 1021, 16384, 32768])
def test_np_fft_against_direct_dft(n):
    """np.fft against the longdouble direct DFT: error <= 2e-16 log2(n) ||f||_2 (about 1/10 of the tightest GPU bound)."""
    rng = np.random.default_rng(n)
    f = rng.standard_normal(n) * rng.uniform(0.5, 1.5, n)
    ms = sorted({0, 1, 2, 3, n // 4, n // 4 + 1, n // 2, n - 1} | set(rng.integers(0, n, 8).tolist()))
    ref = ring_dft_direct_ld(f, ms)
    got = np.fft.fft(f)[ms]
    err = np.abs(got - ref).max()
    assert err <= 2e-16 * np.log2(n) * np.linalg.norm(f), (n, err / np.linalg.norm(f))


@pytest.mark.parametrize("nside", [1, 2, 4, 12, 48])
@pytest.mark.parametrize("weighted", [False, True])
def test_ring_spectra_equal_oracle_fourier_stage(oracle, nside, weighted):
    """ring_spectra_ref = oracle.fourier_analysis x rw 4 pi / npix, lmax = 4 nside: m >= nphi on the polar rings (aliasing
    X[m mod nphi] and the phase reduced mod 2 nphi)."""
    rng = np.random.default_rng(5 * nside + weighted)
    npix = 12 * nside**2
    lmax = 4 * nside
    maps = rng.standard_normal((2, npix))
    pw = rng.uniform(0.5, 1.5, npix) if weighted else None
    rw = rng.uniform(0.5, 1.5, 2 * nside) if weighted else None
    FN, FS = ring_spectra_ref(maps, nside, lmax, pix_weights=pw, ring_weights=rw)
    F = oracle.fourier_analysis(maps, nside, lmax, pix_weights=pw)  # [comp][ring][m]
    w = (np.ones(2 * nside) if rw is None else rw) * 4 * np.pi / npix
    wantN = np.transpose(F[:, : 2 * nside], (0, 2, 1)) * w
    wantS = np.zeros_like(wantN)
    wantS[:, :, : 2 * nside - 1] = np.transpose(F[:, ::-1][:, : 2 * nside - 1], (0, 2, 1)) * w[:-1]
    scale = np.abs(wantN).max()
    assert np.abs(FN - wantN).max() <= 1e-14 * scale
    assert np.abs(FS - wantS).max() <= 1e-14 * scale
    assert (FS[:, :, -1] == 0).all()
    # a subset of orders in any order gives the same columns
    ms = np.array([lmax, 0, 3, 2 * nside + 1, 1])
    sN, sS = ring_spectra_ms(maps, nside, ms, pix_weights=pw, ring_weights=rw, block=3)
    np.testing.assert_array_equal(sN, FN[:, ms])
    np.testing.assert_array_equal(sS, FS[:, ms])
