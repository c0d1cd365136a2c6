"""Host side of the jackknife regions (no GPU): the shared header hx_jkregions.h compiled for the host and checked piece by piece
against the numpy restatement of the rule (tests/jkregions_reference.py); the restatement pinned on its own -- labels that do not
move when every axis is perturbed by 1e-9, which is what licenses the exact comparison of tests/test_gpu_jkregions.py, and the
invariants of a partition --; and the argument logic of ``hx.jackknife_regions`` with the library call stubbed out."""

import os
import subprocess

import numpy as np
import pytest

import jkregions_reference as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: the two parity inputs of the GPU test: (nside, njk, footprint pixels)
PARITY = ((32, 13, 4398), (64, 50, 17557))


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("jkregions") / "t_jkregions"
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "csrc", "test_jkregions.cpp"), "-o", str(exe)])

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-500:]
        answers = out.stdout.strip().split("\n")
        assert len(answers) == len(lines)
        return answers

    return ask


@pytest.fixture(scope="module")
def parity_cases():
    """{(nside, njk): (weight, labels, region weights, axes)} of the reference, computed once."""
    out = {}
    for nside, njk, _ in PARITY:
        w = jr.parity_weight(nside)
        out[nside, njk] = (w,) + jr.regions(nside, w, njk)
    return out


# ---- the header on the host -------------------------------------------------------------------------------------------------------------

def test_header_quantisation(host_program):
    wmax = 0.8371
    w = np.concatenate([[wmax, 1e-300 * wmax, 2.0**-33 * wmax, 2.0**-34 * wmax, 1.5 * 2.0**-32 * wmax, 2.5 * 2.0**-32 * wmax, 0.5 * wmax],
                        np.random.default_rng(1).uniform(0, wmax, 200)])
    got = np.array([int(a) for a in host_program([f"q {float(x).hex()} {float(wmax).hex()}" for x in w])])
    assert (got == jr.quantise(w, wmax)).all()
    assert got[0] == 2**32 and got[1] == 1 and got[2] == 1 and got[3] == 1
    assert got[4] == 2 and got[5] == 2  # ties to even, as np.rint


def test_header_key_order(host_program):
    tiny = 5e-324
    t = np.array([-np.inf, -1.0, np.nextafter(-1.0, 0), -2.3e-308, -tiny, -0.0, 0.0, tiny, 2.3e-308, np.nextafter(1.0, 0), 1.0, np.nextafter(1.0, 2), np.inf])
    keys = np.array([int(a) for a in host_program([f"k {float(x).hex()}" for x in t])], dtype=np.uint64)
    assert (keys == jr.order_key(t)).all()
    assert keys[5] == keys[6]  # -0 and +0 share a key
    order = np.delete(keys, 5)
    assert (np.diff(order.astype(object)) > 0).all()
    rng = np.random.default_rng(2)
    r = np.concatenate([rng.standard_normal(300), rng.standard_normal(50) * 1e-310])
    k = np.array([int(a) for a in host_program([f"k {float(x).hex()}" for x in r])], dtype=np.uint64)
    assert (np.argsort(k, kind="stable") == np.argsort(r + 0.0, kind="stable")).all()


def test_header_target_and_clamped_count(host_program):
    cases = [(10, 1, 2), (10, 1, 3), (11, 1, 3), (1, 1, 2), (2**62 - 1, 2047, 4095), (2**62 + 12345, 2048, 4096), (2**62 + 7, 1, 3),
             (2**63 - 1, 2047, 4095), (2**63 - 1, 2048, 4096), (3 * 2**32 + 5, 6, 13), (2**32 - 1, 25, 50), (2**32, 3, 7)]
    rng = np.random.default_rng(3)
    for _ in range(200):
        n = int(rng.integers(2, 4097))
        cases.append((int(rng.integers(1, 2**63)), n // 2, n))
    got = [int(a) for a in host_program([f"t {Q} {n1} {n}" for Q, n1, n in cases])]
    assert got == [jr.split_target(*c) for c in cases]
    left = [(0, 1, 0), (0, 1, 1), (5, 3, 6), (5, 2, 6), (5, 1, 5), (2**62, 2**32, 2**62 + 2**31), (2**62, 2**32, 2**62 + 2**31 - 1), (2**62, 1, 2**62)]
    got = [int(a) for a in host_program([f"g {E} {q} {T}" for E, q, T in left])]
    assert got == [1 if 2 * E + q <= 2 * T else 0 for E, q, T in left]
    clamp = [(0, 10, 3, 7), (10, 10, 3, 7), (5, 10, 3, 7), (3, 10, 3, 7), (6, 10, 3, 7), (7, 10, 3, 7), (1, 2, 1, 2), (0, 2, 1, 2), (2, 2, 1, 2), (0, 7, 3, 7), (7, 7, 3, 7)]
    got = [int(a) for a in host_program([f"c {c} {m} {n1} {n}" for c, m, n1, n in clamp])]
    assert got == [min(max(c, n1), m - (n - n1)) for c, m, n1, n in clamp]
    # the whole split count of the reference from the header's pieces, on a segment whose heavy pixel defeats the target
    q = [2**32, 1, 1, 1, 1, 7]
    T = int(host_program([f"t {sum(q)} 3 6"])[0])
    E = np.concatenate([[0], np.cumsum(q)[:-1]])
    c = sum(int(a) for a in host_program([f"g {e} {x} {T}" for e, x in zip(E, q)]))
    assert c == 1 and int(host_program([f"c {c} {len(q)} 3 6"])[0]) == jr.split_count(q, 3, 6) == 3


@pytest.mark.parametrize("nside", [1, 2, 5, 24, 64, 8192])
def test_header_pixel_centres(host_program, nside):
    npix = 12 * nside * nside
    rng = np.random.default_rng(nside)
    ncap = 2 * nside * (nside - 1)
    edges = np.array([0, 3, 4, ncap - 1, ncap, ncap + 4 * nside - 1, ncap + 4 * nside, npix - ncap - 1, npix - ncap, npix - 5, npix - 4, npix - 1])
    pix = np.unique(np.clip(np.concatenate([edges, rng.integers(0, npix, 60)]), 0, npix - 1))
    got = np.array([[float(t) for t in a.split()] for a in host_program([f"v {nside} {p}" for p in pix])])
    want = jr.pix2vec_ring(nside, pix)
    assert np.abs(got - want).max() <= 4e-16
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 4e-16


def test_header_pixel_centres_against_the_oracle(oracle):
    """The reference's own pixel centres return their pixel through the oracle's ang2pix, at a power-of-two and another nside."""
    for nside in (24, 64):
        pix = np.arange(12 * nside * nside)
        v = jr.pix2vec_ring(nside, pix)
        lon, lat = np.degrees(np.arctan2(v[:, 1], v[:, 0])) % 360.0, np.degrees(np.arcsin(v[:, 2]))
        assert (oracle.ang2pix_ring(nside, lon, lat) == pix).all()


def _random_covariances(count, seed):
    """Covariances R diag(s^2 (1, f1, f2)) R^T: spreads s from 1 down to 1e-6 (a region at nside 4096, njk 4096), a leading
    eigenvalue separated from the second by at least a fifth of itself."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        s = 10.0 ** (-6.0 * k / (count - 1))
        f1 = rng.uniform(0.05, 0.8)
        f2 = rng.uniform(1e-4, 1.0) * f1
        R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        out.append((R * (s * s * np.array([1.0, f1, f2]))) @ R.T)
    return [(C + C.T) / 2 for C in out]


def test_header_principal_axis_matches_eigh(host_program):
    covs = _random_covariances(200, 4)
    lines = ["e " + " ".join(float(x).hex() for x in (C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2])) for C in covs]
    got = np.array([[float(t) for t in a.split()] for a in host_program(lines)])
    want = np.array([jr.principal_axis(C) for C in covs])
    err = np.abs(got - want).max(axis=1)
    print(f"largest axis error over {len(covs)} covariances: {err.max():.3g}")
    assert err.max() <= 1e-13
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 1e-15
    assert (got[np.arange(len(got)), np.abs(got).argmax(axis=1)] > 0).all()
    # diagonal, permuted-diagonal and rank-one inputs
    for C, axis in ((np.diag([1.0, 2.0, 3.0]), [0, 0, 1]), (np.diag([5.0, 2.0, 3.0]), [1, 0, 0]), (np.outer([1, -2, 2], [1, -2, 2]) / 9.0, [-1 / 3, 2 / 3, -2 / 3])):
        line = "e " + " ".join(float(x).hex() for x in (C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]))
        assert np.abs(np.array([float(t) for t in host_program([line])[0].split()]) - axis).max() <= 1e-15


def test_header_covariance_from_moments(host_program):
    rng = np.random.default_rng(5)
    v = jr.pix2vec_ring(16, rng.integers(0, 3072, 40))
    q = jr.quantise(rng.uniform(0.2, 1, 40), 1.0)
    w = q.astype(np.float64)
    mom = [w.sum(), *(w[:, None] * v).sum(0)] + [(w * v[:, i] * v[:, j]).sum() for i in range(3) for j in range(i, 3)]
    got = np.array([float(t) for t in host_program(["m " + " ".join(float(x).hex() for x in mom)])[0].split()])
    C = jr.covariance(q, v)
    assert np.abs(got - [C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]]).max() <= 1e-15


def test_constants_restated_in_python_match_the_header():
    import re

    from heracles_amd import regions

    with open(os.path.join(ROOT, "heracles_amd", "csrc", "hx_jkregions.h")) as f:
        header = f.read()
    assert int(re.search(r"\bNJK_MAX = (\d+);", header).group(1)) == regions.NJK_MAX == jr.NJK_MAX


# ---- the reference, pinned on its own ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nside,njk,npix_inside", PARITY)
def test_reference_labels_do_not_depend_on_the_last_digits_of_an_axis(parity_cases, nside, njk, npix_inside):
    """The yardstick: with every split axis perturbed by 1e-9 the reference labels every pixel as before."""
    w, labels, rw, axes = parity_cases[nside, njk]
    assert np.count_nonzero(w > 0) == npix_inside
    again, rw2, axes2 = jr.regions(nside, w, njk, perturb=np.random.default_rng(99))
    assert (again == labels).all()
    assert (axes2 == axes).all()  # (the recorded axes are the unperturbed ones)


@pytest.mark.parametrize("nside,njk,npix_inside", PARITY)
def test_reference_invariants(parity_cases, nside, njk, npix_inside):
    w, labels, rw, axes = parity_cases[nside, njk]
    got = jr.check_invariants(w, labels, njk)
    np.testing.assert_allclose(got, rw, rtol=1e-13)
    spread = (rw.max() - rw.min()) / rw.mean()
    print(f"nside {nside}, njk {njk}: spread of the region weights {100 * spread:.3f} % of the mean")
    assert np.abs(np.linalg.norm(axes, axis=1) - 1).max() <= 1e-14


def test_reference_small_and_clamped_cases():
    for nside, w, njk in ((16, jr.cap_weight(16, 0.97), 37), (24, jr.cap_weight(24, 0.97), 7), (16, jr.clamp_weight(), 7),
                          (16, jr.first_pixels_weight(16, 5), 5), (8, jr.cap_weight(8, 0.5), 1), (8, jr.cap_weight(8, 0.5), 2)):
        labels, rw, axes = jr.regions(nside, w, njk)
        assert ((labels == 0) == (w <= 0)).all()
        assert (np.bincount(labels, minlength=njk + 1)[1:] > 0).all()
        assert axes.shape == (njk - 1, 3)
    assert np.count_nonzero(jr.cap_weight(16, 0.97)) == 45
    with pytest.raises(ValueError, match="fewer"):
        jr.regions(16, jr.first_pixels_weight(16, 5), 6)
    with pytest.raises(ValueError, match="pixel 7"):
        jr.regions(1, np.array([1, 1, 1, 1, 1, 1, 1, np.nan, -1, 1, 1, 1.0]), 2)


# ---- hx.jackknife_regions: argument logic with the library call stubbed out ------------------------------------------------------------------

@pytest.fixture
def stub(monkeypatch):
    from heracles_amd import regions

    calls = []

    def fake(nside, weight, njk, labels, weights, axes):
        calls.append({"nside": nside, "njk": njk, "weight": np.array(weight), "info": weights is not None})
        labels[:] = (np.asarray(weight) > 0) * 1
        if weights is not None:
            weights[:] = 2.0
            axes[:] = 0.5

    monkeypatch.setattr(regions, "_jk_regions", fake)
    return calls


def test_jackknife_regions_arguments(stub):
    import heracles_amd as hx

    w = np.linspace(-1.0, 1.0, 48).astype(np.float32)
    labels = hx.jackknife_regions(w, 3)
    assert labels.dtype == np.int32 and labels.shape == (48,) and (labels == (w > 0)).all()
    assert stub[0]["nside"] == 2 and stub[0]["njk"] == 3 and stub[0]["weight"].dtype == np.float64 and not stub[0]["info"]
    labels, info = hx.jackknife_regions(w, 4, return_info=True)
    assert info["weights"].shape == (4,) and info["axes"].shape == (3, 3) and stub[1]["info"]
    for bad in (np.ones(100), np.ones(0), np.ones((2, 48))):
        with pytest.raises(ValueError, match="HEALPix|1-D"):
            hx.jackknife_regions(bad, 2)
    for njk in (0, 4097, -3):
        with pytest.raises(ValueError, match="njk"):
            hx.jackknife_regions(np.ones(48), njk)
    assert len(stub) == 2


def test_jackknife_fsky_accepts_a_tensor():
    import torch

    from heracles_amd.jackknife import jackknife_fsky

    jk = np.array([0, 1, 1, 2, 3, 3, 3, 0, 2, 1, 0, 0], dtype=np.int32)
    t = torch.from_numpy(jk)
    for args in ((), (1,), (1, 3), (2, 2)):
        for ratio in (True, False):
            assert jackknife_fsky(t, *args, ratio=ratio) == jackknife_fsky(jk, *args, ratio=ratio)
