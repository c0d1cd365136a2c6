"""Host side of ``hx.mask_polygons`` (no GPU): the polygon part of the shared header hx_masktools.h compiled for the host
(tests/csrc/test_maskpoly.cpp) and checked against the brute-force restatement of the rule (tests/maskpoly_reference.py) -- validity and
orientation, the inside test on every pixel, the rings and clipped phi windows, the pruning they achieve at nside 1024 --; the same
program once more under the address and undefined-behaviour sanitizers; the new symbol in the bindings and the C header; and the
argument logic of ``hx.mask_polygons`` / ``hx.rectangle_polygons`` with the library call stubbed out.

Every comparison of pixels is exact: the reference asserts for its inputs that no pixel / edge pair has |d| / |n_e| < 1e-9, while the
host's and numpy's sin and cos differ by a few 2^-53."""

import os
import re
import subprocess

import numpy as np
import pytest

import maskpoly_reference as mp
from masktools_reference import ring_start

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "csrc", "test_maskpoly.cpp")
NSIDES = (1, 2, 3, 8, 12, 16, 32)


def _asker(exe):
    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
        answers = out.stdout.split("\n")[:-1]  # (an answer may be empty: no pixel)
        assert len(answers) == len(lines)
        return answers

    return ask


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("maskpoly") / "t_maskpoly"
    subprocess.check_call(["g++", "-O2", "-std=c++17", SOURCE, "-o", str(exe)])
    return _asker(exe)


@pytest.fixture(scope="module")
def shapes():
    """[(name, (lon, lat))]: the ten named shapes, the long triangle, 40 random rectangles -- each also in the other winding."""
    out = []
    for name, p in mp.test_shapes():
        out += [(name, p), (name + ", reversed", mp.reverse(p))]
    return out


def _polygon(p):
    lon, lat = p
    return f"{len(lon)} " + " ".join(f"{float(a).hex()} {float(b).hex()}" for a, b in zip(lon, lat))


def _pixels(answer):
    return np.array(answer.split(), dtype=np.int64)


# ---- validity ----------------------------------------------------------------------------------------------------------------------------

def test_header_validity_accepts_both_windings_and_rejects_what_is_not_a_convex_polygon(host_program, shapes):
    answers = host_program(["v " + _polygon(p) for _, p in shapes])
    for k in range(0, len(shapes), 2):
        a, b = answers[k].split(), answers[k + 1].split()
        assert a[0] == b[0] == "1" and {a[1], b[1]} == {"1", "-1"}, shapes[k][0]  # valid, and the two windings have opposite sigma
        assert mp.is_valid(*shapes[k][1]) and mp.is_valid(*shapes[k + 1][1])
    square = (np.array([10.0, 20.0, 20.0, 10.0]), np.array([-5.0, -5.0, 5.0, 5.0]))
    ngon65 = mp.regular_ngon(40.0, 30.0, 20.0, 65)
    bad = {
        "a repeated vertex": ((np.array([10.0, 20.0, 20.0, 10.0]), np.array([-5.0, -5.0, -5.0, 5.0])), 2),
        "a repeated vertex, not adjacent": ((np.array([10.0, 20.0, 10.0, 15.0]), np.array([-5.0, -5.0, -5.0, 5.0])), 2),
        "a reflex quadrilateral": ((np.array([10.0, 20.0, 13.0, 10.0]), np.array([-5.0, -5.0, -2.0, 5.0])), 2),
        "a collinear triple": ((np.array([10.0, 15.0, 20.0, 15.0]), np.array([0.0, 0.0, 0.0, 9.0])), 2),
        "a bow tie": ((square[0][[0, 2, 1, 3]], square[1][[0, 2, 1, 3]]), 2),
        "a degenerate triangle": ((np.array([10.0, 10.0, 50.0]), np.array([3.0, 3.0, 7.0])), 2),
        "2 vertices": ((square[0][:2], square[1][:2]), 0),
        "65 vertices": (ngon65, 0),
        "a NaN longitude": ((np.array([10.0, np.nan, 20.0, 10.0]), square[1]), 1),
        "a NaN latitude": ((square[0], np.array([-5.0, -5.0, np.nan, 5.0])), 1),
        "an infinite longitude": ((np.array([10.0, 20.0, np.inf, 10.0]), square[1]), 1),
        "a latitude beyond the pole": ((square[0], np.array([-5.0, -5.0, 90.5, 5.0])), 1),
    }
    assert host_program(["v " + _polygon(square)]) == ["1 1"] and mp.is_valid(*square)
    assert host_program(["v " + _polygon(mp.regular_ngon(40.0, 30.0, 20.0, 64))])[0].startswith("1")
    for name, (p, reason) in bad.items():
        assert host_program(["v " + _polygon(p)]) == [f"0 {reason}"], name
        assert not mp.is_valid(*p), name


# ---- the inside test and the windows -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nside", NSIDES)
def test_header_inside_test_agrees_with_the_restatement_on_every_pixel(host_program, shapes, nside):
    every = host_program([f"i {nside} " + _polygon(p) for _, p in shapes])
    pruned = host_program([f"p {nside} " + _polygon(p) for _, p in shapes])
    total = 0
    for (name, p), a, b in zip(shapes, every, pruned):
        want = np.flatnonzero(mp.inside(nside, *p))  # (asserts the gap of its inputs)
        assert np.array_equal(_pixels(a), want), name  # the rule, asked of every pixel
        assert np.array_equal(_pixels(b), want), name  # rings, clipped windows, then the rule: what the kernels do
        total += want.size
    print(f"nside {nside}: {len(shapes)} polygons, {total} pixels inside, smallest gap {mp.gap(nside, [p for _, p in shapes]):.3g}")
    assert total > 0 or nside == 1


@pytest.mark.parametrize("nside", NSIDES)
def test_header_windows_hold_every_inside_pixel_and_no_ring_outside_the_range_holds_one(host_program, shapes, nside):
    answers = host_program([f"w {nside} " + _polygon(p) for _, p in shapes])
    for (name, p), answer in zip(shapes, answers):
        t = [int(s) for s in answer.split()]
        capped, lo, hi, windows = t[0], t[1], t[2], np.array(t[3:]).reshape(-1, 2)
        assert 1 <= lo <= hi <= 4 * nside - 1 and len(windows) == hi - lo + 1
        if name.startswith("long triangle"):
            assert capped == 0 and (lo, hi) == (1, 4 * nside - 1)  # the whole-sphere fallback
        elif name.startswith(("thin trail", "tiny", "on the", "across")):
            assert capped == 1
        hit = mp.inside(nside, *p)
        for ir in range(1, 4 * nside):
            first, n = ring_start(nside, ir)
            js = np.flatnonzero(hit[first:first + n])
            if not lo <= ir <= hi:
                assert js.size == 0, (name, ir)
                continue
            k0, count = windows[ir - lo]
            assert 0 <= count <= n
            assert (((js - k0) % n) < count).all(), (name, ir)


def test_header_clipping_prunes_long_thin_shapes_at_nside_1024(host_program):
    """The pixels tested with the clipped windows, the pixels of the bounding cap's windows, and the pixels inside (found among the
    clipped windows' pixels and among all pixels of the map: no pixel is lost).  Measured: thin trail 145380 / 9345024 / 88540; sliver
    1121336 / 9431040 / 163708 (it crosses most of its rings twice, and the hull of the two crossings is kept); 20 x 0.05 degree
    rectangle 1676 / 97237 / 303."""
    named = mp.named_shapes()
    cases = {"thin trail": named["thin trail"], "sliver": named["sliver"], "20 x 0.05 degree rectangle": mp.rectangle(200.3, -47.1, 20.0, 0.05, 33.0)}
    for name, p in cases.items():
        assert mp.is_valid(*p)
        clipped, cap, inside, inside_all = (int(s) for s in host_program(["c 1024 " + _polygon(p)])[0].split())
        print(f"{name}: {clipped} pixels tested with the clipped windows, {cap} in the bounding cap's windows, {inside} inside")
        assert inside == inside_all > 0
        assert inside <= clipped < cap


# ---- the stand-alone program under the sanitizers (host code only) -----------------------------------------------------------------------

def test_host_program_is_clean_under_the_sanitizers(tmp_path, shapes):
    exe = tmp_path / "t_maskpoly_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SOURCE, "-o", str(exe)])
    ask = _asker(exe)
    subset = shapes[:24]  # the named shapes and the long triangle in both windings, one random rectangle
    lines = ["v " + _polygon(p) for _, p in subset]
    lines += ["v " + _polygon((np.array([1.0, 2.0]), np.array([1.0, 2.0]))), "v " + _polygon(mp.regular_ngon(40.0, 30.0, 20.0, 65))]
    lines += ["v " + _polygon((np.array([1.0, np.nan, 3.0]), np.array([1.0, 2.0, 5.0])))]
    for nside in (1, 2, 12):
        for cmd in "ipwc":
            lines += [f"{cmd} {nside} " + _polygon(p) for _, p in subset]
    ask(lines)


# ---- constants and bindings --------------------------------------------------------------------------------------------------------------

def test_symbol_and_limits_match_the_headers():
    from heracles_amd import _lib

    with open(os.path.join(ROOT, "include", "hxsht.h")) as f:
        api = f.read()
    assert "hx_mask_polygons" in _lib.SYMBOLS
    m = re.search(r"\bint hx_mask_polygons\(([^)]*)\);", api)
    assert m and [a.strip() for a in m.group(1).split(",")] == [
        "int nside", "double *mask", "int64_t npoly", "const int64_t *offsets", "const double *lon", "const double *lat", "double value"]
    with open(os.path.join(ROOT, "heracles_amd", "csrc", "hx_masktools.h")) as f:
        header = f.read()
    assert re.search(r"POLY_MIN = 3, POLY_MAX = 64;", header)  # the 3 .. 64 of the documents and the messages
    for name in ("mask_polygons", "rectangle_polygons"):
        import heracles_amd as hx

        assert name in hx.__all__ and callable(getattr(hx, name))


# ---- hx.mask_polygons / hx.rectangle_polygons: argument logic with the library call stubbed out ------------------------------------------

@pytest.fixture
def stub(monkeypatch):
    from heracles_amd import masks

    calls = []

    def polygons(nside, mask, npoly, offsets, lon, lat, value):
        calls.append({"nside": nside, "npoly": npoly, "offsets": np.array(offsets), "lon": np.array(lon), "lat": np.array(lat), "value": value,
                      "start": np.array(mask)})
        mask[:npoly] = value

    monkeypatch.setattr(masks, "_mask_polygons", polygons)
    return calls


def test_mask_polygons_arguments(stub):
    import heracles_amd as hx

    lon, lat = np.arange(8.0).reshape(2, 4), np.arange(8.0).reshape(2, 4) + 10
    given = np.ones(48, dtype=np.float32)
    out = hx.mask_polygons(given, lon, lat)  # the 2-D form
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out is not given and (given == 1).all()
    assert (out[:2] == 0).all() and (out[2:] == 1).all()
    c = stub[0]
    assert (c["nside"], c["npoly"], c["value"]) == (2, 2, 0.0) and c["offsets"].dtype == np.int64 and c["offsets"].tolist() == [0, 4, 8]
    assert c["lon"].tolist() == list(range(8)) and c["lat"].tolist() == [v + 10 for v in range(8)]
    out = hx.mask_polygons(np.ones(48), np.arange(7.0), np.arange(7.0), [0, 3, 7], value=0.25)  # the offsets form
    c = stub[1]
    assert (c["npoly"], c["value"]) == (2, 0.25) and c["offsets"].dtype == np.int64 and c["offsets"].tolist() == [0, 3, 7] and (out[:2] == 0.25).all()
    # an int nside starts from ones when value == 0 and from zeros otherwise
    out = hx.mask_polygons(3, lon, lat)
    assert out.shape == (108,) and (stub[2]["start"] == 1).all() and stub[2]["nside"] == 3
    out = hx.mask_polygons(3, lon, lat, value=1.0)
    assert out.shape == (108,) and (stub[3]["start"] == 0).all() and (out[:2] == 1).all() and (out[2:] == 0).all()
    out = hx.mask_polygons(1, np.zeros((0, 4)), np.zeros((0, 4)))  # no polygon
    assert out.shape == (12,) and stub[4]["npoly"] == 0 and stub[4]["offsets"].tolist() == [0]
    assert hx.mask_polygons(1, np.zeros(0), np.zeros(0), [0]).shape == (12,) and stub[5]["npoly"] == 0
    n = len(stub)
    for bad in (np.ones(100), np.ones(0), np.ones((2, 48)), 0, 8193):
        with pytest.raises(ValueError, match="HEALPix|1-D|nside"):
            hx.mask_polygons(bad, lon, lat)
    with pytest.raises(ValueError, match="shape"):
        hx.mask_polygons(np.ones(48), lon, lat[:, :3])
    with pytest.raises(ValueError, match="shape"):
        hx.mask_polygons(np.ones(48), np.arange(7.0), np.arange(6.0), [0, 3, 7])
    with pytest.raises(ValueError, match="offsets"):
        hx.mask_polygons(np.ones(48), np.arange(7.0), np.arange(7.0))  # 1-D without offsets
    with pytest.raises(ValueError, match="offsets"):
        hx.mask_polygons(np.ones(48), lon, lat, [0, 4, 8])  # offsets with the 2-D form
    with pytest.raises(ValueError, match="offsets end"):
        hx.mask_polygons(np.ones(48), np.arange(7.0), np.arange(7.0), [0, 3, 6])
    with pytest.raises(ValueError, match="offsets"):
        hx.mask_polygons(np.ones(48), np.arange(7.0), np.arange(7.0), [])
    with pytest.raises(ValueError, match="1-D or 2-D"):
        hx.mask_polygons(np.ones(48), np.zeros((1, 2, 4)), np.zeros((1, 2, 4)))
    assert len(stub) == n


def _separation(lon, lat, want):
    """The angle in degrees between (lon, lat) in degrees and the unit vector want, all in long double."""
    ld = np.longdouble
    rad = np.arctan(ld(1.0)) * ld(4.0) / ld(180.0)
    lo, la = ld(lon) * rad, ld(lat) * rad
    got = np.array([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], dtype=ld)
    return float(np.sqrt(((got - want) ** 2).sum()) / rad)


def test_rectangle_polygons_against_a_long_double_restatement():
    """Every corner lies within 8 ulp of 360 degrees (8 x 2^-44 degrees, 7.9e-15 rad) of the corner computed in long double from the same
    float64 inputs -- the unit in which a longitude is returned: lon pi / 180 alone is rounded at 2 pi (2^-51 rad), so is the returned
    longitude (2^-52 rad), and the sines, cosines, tangents, the three sums and the normalisation add some 2^-53 each."""
    import heracles_amd as hx

    assert np.finfo(np.longdouble).eps < 2.0**-60  # (the restatement is the finer one)
    rng = np.random.default_rng(21)
    n = 60
    lon, lat = rng.uniform(0, 360, n), np.degrees(np.arcsin(rng.uniform(-1, 1, n)))
    length, width, angle = 10.0 ** rng.uniform(-3, np.log10(175.0), n), 10.0 ** rng.uniform(-3, np.log10(175.0), n), rng.uniform(-360, 360, n)
    lon[:4], lat[:4], length[:4], width[:4], angle[:4] = [359.2, 123.4, 0.0, 250.1], [23.7, 41.8103, 90.0, -90.0], [31.3, 17.9, 5.0, 170.3], [9.1, 6.3, 3.0, 4.7], [63.0, -20.0, 0.0, 12.0]
    glon, glat = hx.rectangle_polygons(lon, lat, length, width, angle)
    assert isinstance(glon, np.ndarray) and glon.shape == glat.shape == (n, 4) and glon.dtype == glat.dtype == np.float64
    assert (glon >= 0).all() and (glon < 360).all() and (np.abs(glat) <= 90).all()
    worst = 0.0
    for k in range(n):
        want = mp.rectangle_vectors(lon[k], lat[k], length[k], width[k], angle[k], dtype=np.longdouble)
        for c in range(4):
            worst = max(worst, _separation(glon[k, c], glat[k, c], want[c]))
        assert mp.is_valid(glon[k], glat[k]), k  # convex for a length and a width below 180 degrees
    print(f"worst corner separation: {worst / 2.0**-44:.3g} ulp of 360 degrees")
    assert worst <= 8 * 2.0**-44
    # through the centre the rectangle is exactly length by width: the midpoints of opposite edges are that far apart
    v = mp.vertices(glon[0], glat[0])
    mid = [v[0] + v[1], v[2] + v[3], v[1] + v[2], v[3] + v[0]]
    mid = [m / np.linalg.norm(m) for m in mid]
    assert abs(np.degrees(np.arccos(mid[0] @ mid[1])) - length[0]) < 1e-12 and abs(np.degrees(np.arccos(mid[2] @ mid[3])) - width[0]) < 1e-12
    # numbers broadcast against arrays; one rectangle from numbers alone
    a, b = hx.rectangle_polygons(lon, lat, 2.0, 1.0, 30.0)
    c, d = hx.rectangle_polygons(lon, lat, np.full(n, 2.0), np.full(n, 1.0), np.full(n, 30.0))
    assert a.tobytes() == c.tobytes() and b.tobytes() == d.tobytes()
    one = hx.rectangle_polygons(10.0, 20.0, 2.0, 1.0, 0.0)
    assert one[0].shape == one[1].shape == (1, 4) and one[1][0, 0] > 20.0 > one[1][0, 2]  # the long axis points north at angle 0
    for bad in (0.0, -1.0, 180.0, float("nan")):
        with pytest.raises(ValueError, match="length"):
            hx.rectangle_polygons(lon, lat, bad, 1.0, 0.0)
        with pytest.raises(ValueError, match="width"):
            hx.rectangle_polygons(lon, lat, 1.0, bad, 0.0)
    with pytest.raises(ValueError, match="1-D"):
        hx.rectangle_polygons(np.zeros((2, 2)), np.zeros((2, 2)), 1.0, 1.0, 0.0)
