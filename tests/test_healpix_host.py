"""Host side of the pixel geometry (no GPU): the shared header hx_healpix.h compiled for the host and checked against the references
the tests already have -- ``pixel_reference.ring_starts`` / ``ring2nest_exact`` / ``nest2ring_exact``, ``mockcat_reference.ring2xyf``,
the centres of ``jkregions_reference`` and the rings of ``masktools_reference`` -- over every pixel of the small nsides (3, 5 and 255
take the path that is no power of two; 1 has no cap and 2 a cap of one ring) and, at nside 8192, over
``pixel_reference.sample_pixels``: the first and the last pixel of every ring, the pixels either side of both cap / belt boundaries,
the corners of the faces."""

import math
import os
import subprocess

import numpy as np
import pytest

import jkregions_reference as jr
import masktools_reference as mt
import mockcat_reference as mc
import pixel_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSIDES = (1, 2, 3, 4, 5, 8, 16, 64, 255)
POW2 = tuple(n for n in NSIDES if n & (n - 1) == 0)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("healpix") / "t_healpix"
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "csrc", "test_healpix.cpp"), "-o", str(exe)])

    def ask(line, dtype=np.int64):
        out = subprocess.run([str(exe)], input=line + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-500:]
        return np.array(out.stdout.split(), dtype=dtype)

    return ask


def _pixels(nside):
    """(the pixels, their spelling on a request line): every pixel, or the sample at nside 8192"""
    if nside == 8192:
        pix = pr.sample_pixels(nside, np.random.default_rng(nside), 2000)
        return pix, " ".join(str(p) for p in pix)
    return np.arange(12 * nside * nside), "all"


@pytest.mark.parametrize("nside", NSIDES + (8192,))
def test_rings_and_face_coordinates(host_program, nside):
    pix, text = _pixels(nside)
    ir, j, first, n, face, ix, iy, back = host_program(f"p {nside} {text}").reshape(pix.size, 8).T
    starts = pr.ring_starts(nside)
    assert (ir == np.searchsorted(starts, pix, side="right")).all() and (ir >= 1).all() and (ir <= 4 * nside - 1).all()
    assert (first == starts[ir - 1]).all() and (n == starts[ir] - starts[ir - 1]).all()
    assert (first + j == pix).all() and (j >= 0).all() and (j < n).all()
    for r in np.unique(ir)[:: max(1, nside // 16)]:
        assert mt.ring_start(nside, int(r)) == (first[ir == r][0], n[ir == r][0])
    assert (np.array([face, ix, iy]) == np.array(mc.ring2xyf(nside, pix))).all()
    assert (face >= 0).all() and (face < 12).all() and (np.minimum(ix, iy) >= 0).all() and (np.maximum(ix, iy) < nside).all()
    assert (back == pix).all()  # xyf2ring(ring2xyf(p)) == p


@pytest.mark.parametrize("nside", POW2 + (8192,))
def test_ring_and_nest(host_program, nside):
    pix, text = _pixels(nside)
    order = nside.bit_length() - 1
    nest, ring = host_program(f"n {order} {text}").reshape(pix.size, 2).T
    assert (nest == pr.ring2nest_exact(nside, pix)).all()
    assert (ring == pr.nest2ring_exact(nside, pix)).all()
    # each a permutation, inverse to the other: over every pixel directly, on the sample through a second call
    if text == "all":
        assert (np.sort(nest) == pix).all() and (np.sort(ring) == pix).all()
        assert (ring[nest] == pix).all() and (nest[ring] == pix).all()
    else:
        assert (host_program(f"n {order} " + " ".join(str(q) for q in nest))[1::2] == pix).all()
        assert (host_program(f"n {order} " + " ".join(str(p) for p in ring))[0::2] == pix).all()


@pytest.mark.parametrize("nside", NSIDES + (8192,))
def test_pixel_centres(host_program, nside):
    pix, text = _pixels(nside)
    got = host_program(f"v {nside} {text}", np.float64).reshape(pix.size, 3)
    assert np.abs(got - jr.pix2vec_ring(nside, pix)).max() <= 4e-16
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 4e-16


def test_integer_square_root(host_program):
    k = np.concatenate([np.arange(1, 2**15 + 1), np.unique(np.geomspace(2**15, 2**26 - 1, 4000).astype(np.int64)), [2**26 - 1]])
    v = np.concatenate([k * k - 1, k * k, k * k + 1])
    assert v.max() < 2**52
    got = host_program("q " + " ".join(str(x) for x in v))
    assert (got == np.concatenate([k - 1, k, k])).all()
    assert all(int(g) == math.isqrt(int(x)) for g, x in zip(got[:: 997], v[:: 997]))
