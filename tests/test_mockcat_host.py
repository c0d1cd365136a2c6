"""Host side of the Poisson-sampled mock catalogues (no GPU): the shared header hx_mockcat.h compiled for the host and checked
against the numpy reference of the definition (tests/mockcat_reference.py); the reference pinned on its own -- moments of its two
samplers, every point back in its own pixel through ``oracle.ang2pix_ring`` --; and the argument / key logic of
``hx.poisson_catalog`` and ``hx.mock_catalogs`` with the library calls stubbed out."""

import os
import subprocess

import numpy as np
import pytest

import mockcat_reference as mr
import pixel_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (7 << 32) + 20241


# ---- the header on the host -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mockcat") / "t_mockcat"
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "csrc", "test_mockcat.cpp"), "-o", str(exe)])

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-500:]
        answers = out.stdout.strip().split("\n")
        assert len(answers) == len(lines)
        return answers

    return ask


#: the fixed (lambda, counter) inputs of the exact count comparison
COUNT_LAMBDAS = (0.0, 1e-300, 1e-3, 0.01, 0.7, 3.0, 12.0, 31.9, np.nextafter(32.0, 0.0), 32.0, 32.1, 100.0, 5000.0, 1e6, 2.0**30)
COUNT_PIXELS = (0, 1, 2, 77, 4095, 12 * 8192**2 - 1)
COUNT_REALISATIONS = (0, 3, 2**32 - 1)


def test_header_counts_match_the_reference_exactly(host_program):
    cases = [(lam, p, r) for lam in COUNT_LAMBDAS for p in COUNT_PIXELS for r in COUNT_REALISATIONS]
    got = np.array([int(a) for a in host_program([f"c {float(lam).hex()} {p} {r} {SEED}" for lam, p, r in cases])])
    want = np.array([mr.counts(np.array([lam]), np.array([p]), SEED, r)[0][0] for lam, p, r in cases])
    assert (got == want).all(), [(c, g, w) for c, g, w in zip(cases, got, want) if g != w][:5]
    lam = np.array([c[0] for c in cases])
    assert (got[lam == 0] == 0).all() and (got[lam == 1e-300] == 0).all()
    assert got[lam == 2.0**30].min() > 2**30 - 10 * 2**15 and got[lam == 2.0**30].max() < 2**30 + 10 * 2**15
    assert host_program([f"c {x} 5 0 {SEED}" for x in ("nan", "-1e-300", "inf", float(2.0**30 + 1).hex())]) == ["invalid"] * 4


@pytest.mark.parametrize("nside", [1, 2, 5, 64, 8192])
def test_header_positions_match_the_reference(host_program, nside):
    pix = pr.sample_pixels(nside, np.random.default_rng(nside), 40)
    index = np.arange(pix.size) % 3 + (pix % 2) * 1000
    faces = np.array([[int(t) for t in a.split()] for a in host_program([f"x {nside} {p}" for p in pix])])
    assert (faces.T == np.array(mr.ring2xyf(nside, pix))).all()
    got = np.array([[float(t) for t in a.split()] for a in host_program([f"p {nside} {p} {i} 2 {SEED}" for p, i in zip(pix, index)])])
    lon, lat = mr.positions(nside, pix, index, SEED, 2)
    assert np.abs(got[:, 0] - lon).max() <= 1e-13 and np.abs(got[:, 1] - lat).max() <= 1e-13
    assert (got[:, 0] >= 0).all() and (got[:, 0] < 360).all()


def test_header_noise_matches_the_reference(host_program):
    pix, index = np.arange(50) * 977, np.arange(50) % 7
    got = np.array([float(a) for a in host_program([f"v {p} {i} 1 4 {SEED}" for p, i in zip(pix, index)])])
    assert np.abs(got - mr.noise(pix, index, 1, SEED, 4)).max() <= 1e-13


def test_constants_restated_in_python_match_the_sources():
    import re

    from heracles_amd import mocks

    with open(os.path.join(ROOT, "heracles_amd", "csrc", "hx_mockcat.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "heracles_amd", "csrc", "hx_mockcat.hip")) as f:
        source = f.read()

    def const(text, name):
        value = re.search(rf"\b{name} = (0x[0-9a-f]+|[0-9.]+)u?;", text).group(1)
        return int(value, 16) if value.startswith("0x") else float(value)

    assert const(source, "MC_BLOCK") == mocks.POINTS_PER_GROUP
    assert const(header, "LAMBDA_SWITCH") == mocks.LAMBDA_SWITCH == mr.LAMBDA_SWITCH
    assert const(header, "LAMBDA_MAX") == mocks.LAMBDA_MAX == mr.LAMBDA_MAX
    assert const(header, "INVERSION_KMAX") == mr.INVERSION_KMAX and const(header, "PTRS_MAXIT") == mr.PTRS_MAXIT
    assert const(header, "STREAM_BIT") == mr.STREAM_BIT


# ---- the reference, pinned on its own -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", [0.01, 3.0, 31.9, 32.0, 100.0, 5000.0])
def test_reference_poisson_moments(lam):
    """Fixed seed: mean and variance of 4 10^5 draws within 5 standard errors of lambda (the variance's standard error from the
    fourth central moment of the Poisson law, lambda + 3 lambda^2)."""
    n = 400_000
    k, unsafe = mr.counts(np.full(n, lam), np.arange(n), SEED)
    assert unsafe.mean() <= 1e-3
    mean, var = k.mean(), k.var(ddof=1)
    se_mean = np.sqrt(lam / n)
    se_var = np.sqrt((lam + 3 * lam**2 - lam**2 * (n - 3) / (n - 1)) / n)
    print(f"lambda {lam}: mean {mean:.6g} ({(mean - lam) / se_mean:+.2f} se), variance {var:.6g} ({(var - lam) / se_var:+.2f} se)")
    assert abs(mean - lam) < 5 * se_mean
    assert abs(var - lam) < 5 * se_var


def test_reference_ptrs_iterations_and_streams():
    n = 100_000
    for lam in (32.0, 5000.0, 1e6):
        k, _, iters = mr.poisson_ptrs(np.full(n, lam), np.arange(n), 0, SEED)
        assert 1.1 < iters.mean() < 1.25 and iters.max() < 20
    # another realisation, another seed: other draws; the same inputs: the same
    a = mr.counts(np.full(1000, 3.0), np.arange(1000), SEED, 0)[0]
    assert (a == mr.counts(np.full(1000, 3.0), np.arange(1000), SEED, 0)[0]).all()
    assert (a != mr.counts(np.full(1000, 3.0), np.arange(1000), SEED, 1)[0]).any()
    assert (a != mr.counts(np.full(1000, 3.0), np.arange(1000), SEED + 1, 0)[0]).any()
    with pytest.raises(ValueError, match="pixel 12"):
        mr.counts(np.array([1.0, np.nan, -1.0]), np.array([11, 12, 13]), SEED)


@pytest.mark.parametrize("nside", [1, 2, 5, 64, 8192])
def test_reference_points_return_their_own_pixel(oracle, nside):
    """Corner, edge-midpoint and random offsets of the sampled pixels through the face map, then ``oracle.ang2pix_ring``."""
    pix = pr.sample_pixels(nside, np.random.default_rng(100 + nside), 300)
    face, ix, iy = mr.ring2xyf(nside, pix)
    lo, hi, mid = 0.5 * 2.0**-24, 1.0 - 0.5 * 2.0**-24, 0.5
    rng = np.random.default_rng(nside)
    offs = [(a, b) for a in (lo, hi) for b in (lo, hi)] + [(lo, mid), (hi, mid), (mid, lo), (mid, hi)]
    offs += [tuple(mr.offsets(*rng.integers(0, 2**32, 2, dtype=np.uint64))) for _ in range(8)]
    for u, v in offs:
        lon, lat = mr.xyf2lonlat(nside, face, ix, iy, np.float64(u), np.float64(v))
        assert (lon >= 0).all() and (lon < 360).all()
        back = oracle.ang2pix_ring(nside, lon, lat)
        assert (back == pix).all(), (nside, u, v, pix[back != pix][:5])
    # and the points of the definition itself
    lon, lat = mr.positions(nside, pix, np.arange(pix.size) % 5, SEED)
    assert (oracle.ang2pix_ring(nside, lon, lat) == pix).all()


def test_reference_catalog_layout():
    count = np.array([0, 2, 0, 0, 3, 1])
    maps = np.arange(12.0).reshape(2, 6)
    c = mr.catalog(4, 100, count, SEED, maps=maps, sigma=[0.0, 0.5])
    assert (c["pix"] == [101, 101, 104, 104, 104, 105]).all() and (c["index"] == [0, 1, 0, 1, 2, 0]).all()
    assert (c["values"][0] == maps[0][c["pix"] - 100]).all()
    assert (c["values"][1] == maps[1][c["pix"] - 100] + 0.5 * mr.noise(c["pix"], c["index"], 1, SEED)).all()


# ---- hx.poisson_catalog / hx.mock_catalogs: host logic with the library calls stubbed out ----------------------------------------------------

@pytest.fixture
def stub(monkeypatch):
    """Replace the two library calls: every pixel gets 2 points; point g gets lon = g, lat = -g, value column j = maps[j][pixel] + j."""
    from heracles_amd import mocks

    calls = []

    def fake_counts(nside, pix_begin, pix_end, lam, seed, realisation):
        calls.append({"call": "counts", "nside": nside, "range": (pix_begin, pix_end), "lam": np.array(lam), "seed": seed, "realisation": realisation})
        return np.full(pix_end - pix_begin, 2, dtype=np.int64), 2 * (pix_end - pix_begin)

    def fake_points(nside, pix_begin, pix_end, counts, total, seed, realisation, maps, sigma, like):
        calls.append({"call": "points", "nside": nside, "range": (pix_begin, pix_end), "maps": None if maps is None else np.array(maps),
                      "sigma": None if sigma is None else np.array(sigma), "seed": seed, "realisation": realisation})
        g = np.arange(total, dtype=np.float64)
        nval = 0 if maps is None else len(maps)
        values = np.stack([np.repeat(maps[j], 2) + j for j in range(nval)]) if nval else np.zeros((0, total))
        return g, -g, values

    monkeypatch.setattr(mocks, "_mockcat_counts", fake_counts)
    monkeypatch.setattr(mocks, "_mockcat_points", fake_points)
    return calls


def test_poisson_catalog_columns_metadata_and_range(stub):
    import heracles_amd as hx

    nside = 2
    lam = np.linspace(0.0, 4.7, 48)
    vals = np.arange(96.0).reshape(2, 48)
    cat = hx.poisson_catalog(lam, vals, noise=[0.0, 0.25], seed=9, realisation=4, value_names=("a", "b"), weight="w", page_size=10)
    assert isinstance(cat, hx.ArrayCatalog) and cat.names == ["ra", "dec", "a", "b", "w"] and cat.size == 96 and cat.page_size == 10
    md = cat.metadata
    assert (md["seed"], md["realisation"], md["nside"], md["total"]) == (9, 4, 2, 96)
    page = next(iter(cat))
    assert (page["w"] == 1).all() and (page["b"] == np.repeat(vals[1], 2)[:10] + 1).all()
    counts, points = stub
    assert counts["nside"] == 2 and counts["range"] == (0, 48) and (counts["lam"] == lam).all() and counts["seed"] == 9 and counts["realisation"] == 4
    assert (points["sigma"] == [0.0, 0.25]).all() and (points["maps"] == vals).all()
    # a pixel range: arrays cover the range only and nside must be given
    cat = hx.poisson_catalog(lam[8:20], nside=2, pixel_range=(8, 20), seed=9, names=("lon", "lat"))
    assert cat.names == ["lon", "lat"] and cat.size == 24 and stub[-2]["range"] == (8, 20) and stub[-1]["maps"] is None
    assert cat.metadata["pixel_range"] == (8, 20)
    vis = np.ones(48)
    assert hx.poisson_catalog(lam, seed=1, visibility=vis).visibility is vis


def test_poisson_catalog_rejects_bad_arguments(stub):
    import heracles_amd as hx

    lam = np.ones(48)
    with pytest.raises(ValueError, match="seed"):
        hx.poisson_catalog(lam, seed=-1)
    with pytest.raises(ValueError, match="realisation"):
        hx.poisson_catalog(lam, seed=1, realisation=2**32)
    with pytest.raises(ValueError, match="HEALPix"):
        hx.poisson_catalog(np.ones(47), seed=1)
    with pytest.raises(ValueError, match="nside"):
        hx.poisson_catalog(np.ones(5), seed=1, pixel_range=(0, 5))
    with pytest.raises(ValueError, match="pixel_range"):
        hx.poisson_catalog(np.ones(5), seed=1, nside=2, pixel_range=(0, 6))
    with pytest.raises(ValueError, match="values"):
        hx.poisson_catalog(lam, np.ones((2, 47)), seed=1)
    with pytest.raises(ValueError, match="noise"):
        hx.poisson_catalog(lam, np.ones((2, 48)), noise=[1.0], seed=1)
    with pytest.raises(ValueError, match="value_names"):
        hx.poisson_catalog(lam, np.ones((2, 48)), value_names=("a",), seed=1)
    assert not stub


class _Mapper:
    def __init__(self, nside):
        self.nside, self.lmax, self.deconvolve = nside, 2 * nside, False


def _map(data, **md):
    data = np.array(data, dtype=float)
    data.dtype = np.dtype(data.dtype.str, metadata=md)
    return data


def test_mock_catalogs_builds_lambda_columns_and_seeds(stub):
    import heracles_amd as hx
    from heracles_amd import mocks

    m = _Mapper(2)
    fields = {"POS": hx.Positions(m, "ra", "dec"), "SHE": hx.Shears(m, "ra", "dec", "g1", "g2", "w"), "VIS": hx.Visibility(m),
              "KAP": hx.ScalarField(_Mapper(4), "ra", "dec", "kappa", "w")}
    delta = np.linspace(-1.5, 1.0, 48)
    maps = {("POS", 1): _map(delta, nside=2, spin=0), ("POS", 2): _map(-delta, nside=2, spin=0),
            ("SHE", 1): _map(np.arange(96.0).reshape(2, 48), nside=2, spin=2), ("SHE", 2): _map(np.ones((2, 48)), nside=2, spin=2),
            ("KAP", 1): _map(np.ones(192), nside=4, spin=0)}
    vis = {1: np.linspace(0.0, 1.0, 48), 2: None}
    cats = hx.mock_catalogs(fields, maps, {1: 3.0, 2: 0.5}, visibility=vis, noise={"SHE": (0.3, 0.3)}, seed=100, realisation=6)
    assert list(cats) == [1, 2]
    assert cats[1].names == ["ra", "dec", "g1", "g2", "w"]  # (KAP lives on another nside: not a column of this catalogue)
    c1, p1, c2, p2 = stub
    assert (c1["lam"] == 3.0 * vis[1] * np.maximum(0.0, 1.0 + delta)).all() and (c2["lam"] == 0.5 * np.maximum(0.0, 1.0 - delta)).all()
    assert (p1["maps"] == maps["SHE", 1]).all() and (p1["sigma"] == [0.3, 0.3]).all()
    assert c1["seed"] == mocks.bin_seed(100, 1) == p1["seed"] and c2["seed"] == mocks.bin_seed(100, 2) and c1["seed"] != c2["seed"]
    assert c1["realisation"] == 6 and cats[1].visibility is vis[1] and cats[2].visibility is None
    assert mocks.bin_seed(100, 1) == (100 + 0x9E3779B97F4A7C15 * 2) % 2**64
    # one scalar for all bins
    cats = hx.mock_catalogs({"POS": fields["POS"]}, {("POS", 1): maps["POS", 1]}, 2.0, seed=1)
    assert cats[1].names == ["ra", "dec"] and (stub[-2]["lam"] == 2.0 * np.maximum(0.0, 1.0 + delta)).all()


def test_mock_catalogs_rejects_inconsistent_input(stub):
    import heracles_amd as hx

    m = _Mapper(2)
    pos, she = hx.Positions(m, "ra", "dec"), hx.Shears(m, "ra", "dec", "g1", "g2")
    d = _map(np.zeros(48), nside=2, spin=0)
    with pytest.raises(ValueError, match="Positions"):
        hx.mock_catalogs({"SHE": she}, {("SHE", 1): _map(np.zeros((2, 48)), nside=2, spin=2)}, 1.0, seed=1)
    with pytest.raises(ValueError, match="no map"):
        hx.mock_catalogs({"POS": pos, "SHE": she}, {("SHE", 1): _map(np.zeros((2, 48)), nside=2, spin=2)}, 1.0, seed=1)
    with pytest.raises(ValueError, match="nside"):
        hx.mock_catalogs({"POS": pos}, {("POS", 1): _map(np.zeros(192), nside=4, spin=0)}, 1.0, seed=1)
    with pytest.raises(ValueError, match="rows"):
        hx.mock_catalogs({"POS": pos, "SHE": she}, {("POS", 1): d, ("SHE", 1): _map(np.zeros(48), nside=2, spin=0)}, 1.0, seed=1)
    with pytest.raises(ValueError, match="nbar"):
        hx.mock_catalogs({"POS": pos}, {("POS", 1): d}, {2: 1.0}, seed=1)
    assert not stub
