"""Host side of the mask tools (no GPU): the shared header hx_masktools.h compiled for the host and checked piece by piece against
the brute-force restatement of the rule (tests/masktools_reference.py) -- ring geometry, the rings and phi windows of a disc, the
discs themselves, the pruned search with its evaluation counter, the tapers --; the same program once more under the address and
undefined-behaviour sanitizers; and the argument logic of ``hx.mask_discs`` / ``hx.mask_distance`` / ``hx.apodize_mask`` with the
library calls stubbed out."""

import os
import re
import subprocess

import numpy as np
import pytest

import masktools_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "csrc", "test_masktools.cpp")
NSIDES = (1, 2, 3, 8, 12, 16, 32)


def _asker(exe):
    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
        answers = out.stdout.rstrip("\n").split("\n")
        assert len(answers) == len(lines)
        return answers

    return ask


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("masktools") / "t_masktools"
    subprocess.check_call(["g++", "-O2", "-std=c++17", SOURCE, "-o", str(exe)])
    return _asker(exe)


def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _floats(text):
    return np.array([float.fromhex(t) for t in text.split()])


def _discs(nside, seed):
    lon, lat, radius = mr.named_discs(nside)
    rlon, rlat, rrad = mr.random_discs(12, seed)
    return np.concatenate([lon, rlon]), np.concatenate([lat, rlat]), np.concatenate([radius, rrad])


def _search(host_program, nside, mask, max_distance):
    masked = np.flatnonzero(mask <= 0)
    line = f"s {nside} {float(max_distance).hex()} {masked.size} " + " ".join(str(p) for p in masked)
    H, evals = host_program([line])[0].split(";")
    return _floats(H), np.array([int(t) for t in evals.split()])


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nside", NSIDES + (64, 255))
def test_header_rings_reproduce_the_pixel_centres_bit_for_bit(host_program, nside):
    assert host_program([f"B {nside}"]) == ["0"]


def test_header_chord_and_angle(host_program):
    rng = np.random.default_rng(1)
    u = rng.standard_normal((200, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    v = u + 10.0 ** rng.uniform(-9, 0, 200)[:, None] * rng.standard_normal((200, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    got = np.array([float.fromhex(a) for a in host_program(["h " + _hex(np.concatenate([a, b])) for a, b in zip(u, v)])])
    assert (got == mr.chord_h(u, v)).all()  # (the same operations in the same order)
    deg = np.concatenate([[0.0, 1e-4, 0.5 / 60, 0.5, 20.0, 90.0, 180.0], rng.uniform(0, 180, 50)])
    got = np.array([float.fromhex(a) for a in host_program([f"a {float(d).hex()}" for d in deg])])
    want = mr.angle_h(deg)
    assert np.abs(got - want).max() <= 8 * mr.EPS * 2.0 and (np.abs(got - want) <= 8 * mr.EPS * want + 1e-300).all()
    assert got[0] == 0.0 and abs(got[6] - 2.0) <= 4 * mr.EPS  # h(0) = 0, h(180) = 2


@pytest.mark.parametrize("nside", NSIDES)
def test_header_windows_hold_every_pixel_of_the_disc_and_little_else(host_program, nside):
    lon, lat, radius = _discs(nside, 100 + nside)
    table = mr.disc_table(nside, lon, lat)
    z = np.array([mr.centres(nside)[mr.ring_start(nside, ir)[0], 2] for ir in range(1, 4 * nside)])
    theta_ring = np.arccos(z)
    answers = host_program([f"w {nside} {float(a).hex()} {float(b).hex()} {float(c).hex()}" for a, b, c in zip(lon, lat, radius)])
    for k, answer in enumerate(answers):
        t = [int(s) for s in answer.split()]
        lo, hi, windows = t[0], t[1], np.array(t[2:]).reshape(-1, 2)
        assert 1 <= lo <= hi <= 4 * nside - 1 and len(windows) == hi - lo + 1
        theta_c, r = np.radians(90.0 - lat[k]), np.radians(radius[k])
        has_pole = theta_c - r <= 0 or theta_c + r >= np.pi
        assert hi - lo + 1 <= np.count_nonzero(np.abs(theta_ring - theta_c) <= r) + 4
        hit = table[:, k] <= mr.angle_h(radius[k])
        for ir in range(1, 4 * nside):
            first, n = mr.ring_start(nside, ir)
            js = np.flatnonzero(hit[first:first + n])
            if not lo <= ir <= hi:
                assert js.size == 0, (k, ir)
                continue
            k0, count = windows[ir - lo]
            assert 1 <= count <= n
            assert (((js - k0) % n) < count).all(), (k, ir)  # the window holds every pixel of the disc
            if count == n:
                assert has_pole or js.size + 6 >= n, (k, ir)
            else:
                assert count <= js.size + 6, (k, ir, count, js.size)  # one pixel each side, the roundings of floor and ceil


@pytest.mark.parametrize("nside", NSIDES)
def test_header_discs_match_the_table_exactly(host_program, nside):
    lon, lat, radius = _discs(nside, 200 + nside)
    gap = mr.disc_gap(nside, lon, lat, radius)
    assert gap >= 1e-9, gap  # no pixel sits on an edge: the comparison below may be exact
    want = np.flatnonzero(mr.mask_discs(np.ones(12 * nside * nside), lon, lat, radius) == 0)
    line = f"d {nside} {lon.size} " + " ".join(_hex(t) for t in zip(lon, lat, radius))
    got = np.array([int(s) for s in host_program([line])[0].split()])
    assert got.size == want.size and (got == want).all()
    # every disc on its own as well (the union can hide a pixel one disc lost and another one covered)
    for k in range(lon.size):
        one = np.flatnonzero(mr.mask_discs(np.ones(12 * nside * nside), lon[k:k + 1], lat[k:k + 1], radius[k:k + 1]) == 0)
        got = np.array([int(s) for s in host_program([f"d {nside} 1 " + _hex((lon[k], lat[k], radius[k]))])[0].split()], dtype=np.int64)
        assert got.size == one.size and (got == one).all(), k


# ---- the search --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nside", NSIDES)
def test_header_search_matches_the_full_minimum(host_program, nside):
    worst = 0.0
    for name, mask in mr.hole_masks(nside).items():
        for max_distance in (25.0, 180.0):
            H, evals = _search(host_program, nside, mask, max_distance)
            want = mr.mask_h(mask, max_distance)
            err, bound = np.abs(H - want), mr.distance_bound(want)
            assert (err <= bound).all(), (name, max_distance, np.argmax(err - bound))
            assert (H[mask <= 0] == 0).all() and (evals[mask <= 0] == 0).all()
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    print(f"nside {nside}: worst |H - H_ref| / bound = {worst:.3g}")


def test_header_search_cost_does_not_scale_with_the_disc_area(host_program):
    """One masked pixel at nside 64, max_distance 20 degrees: every unmasked pixel evaluates h at most 4 times per ring whose colatitude
    lies within 20 degrees of its own -- and H is h to that one pixel, or the cap."""
    nside, q, deg = 64, 20000, 20.0
    mask = np.ones(12 * nside * nside)
    mask[q] = 0.0
    H, evals = _search(host_program, nside, mask, deg)
    v = mr.centres(nside)
    theta = np.arccos(v[:, 2])
    theta_ring = np.unique(theta)
    assert theta_ring.size == 4 * nside - 1
    rings_within = np.array([np.count_nonzero(np.abs(theta_ring - t) <= np.radians(deg)) for t in theta_ring])[np.searchsorted(theta_ring, theta)]
    assert (evals <= 4 * rings_within).all()
    print(f"largest number of h evaluations of one pixel: {evals.max()}, rings within {deg} degrees: {rings_within.min()} .. {rings_within.max()}")
    want = np.minimum(mr.angle_h(deg), mr.chord_h(v, v[q]))
    assert (np.abs(H - want) <= mr.distance_bound(want)).all()
    assert H[q] == 0 and np.count_nonzero(H < mr.angle_h(deg)) > 1000


# ---- tapers ------------------------------------------------------------------------------------------------------------------------------

def test_header_tapers(host_program):
    import heracles_amd.masks as masks

    x = np.concatenate([[0.0, 1.0], np.linspace(0, 1, 401)[1:-1], 10.0 ** np.linspace(-8, -1, 30)])
    for kind, number in masks.KINDS.items():
        got = np.array([float.fromhex(a) for a in host_program([f"t {number} {float(t).hex()}" for t in x])])
        assert got[0] == 0.0 and got[1] == 1.0
        assert np.abs(got - mr.taper(kind, x)).max() <= 8 * mr.EPS
        order = np.argsort(x, kind="stable")
        assert (np.diff(got[order]) >= 0).all()  # monotone
        H = np.random.default_rng(3).uniform(0, 1, 50) * mr.angle_h(10.0)
        got = np.array([float.fromhex(a) for a in host_program([f"T {number} {float(h).hex()} {float(mr.angle_h(10.0)).hex()}" for h in H])])
        assert np.abs(got - mr.taper(kind, np.sqrt(H / mr.angle_h(10.0)))).max() <= 8 * mr.EPS
    assert float.fromhex(host_program(["T 1 " + _hex((2.5, 2.0))])[0]) == 1.0  # (x > 1 cannot arise from a capped H; it gives 1)


def test_reference_tapers_known_answers():
    for kind in ("C1", "C2"):
        assert mr.taper(kind, 0.0) == 0.0 and abs(mr.taper(kind, 1.0) - 1.0) <= mr.EPS and abs(mr.taper(kind, 0.5) - 0.5) <= mr.EPS
    with pytest.raises(ValueError):
        mr.taper("Smooth", 0.5)


# ---- the stand-alone program under the sanitizers (host code only) -----------------------------------------------------------------------

def test_host_program_is_clean_under_the_sanitizers(tmp_path):
    exe = tmp_path / "t_masktools_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SOURCE, "-o", str(exe)])
    ask = _asker(exe)
    nside = 12
    lon, lat, radius = _discs(nside, 200 + nside)
    lines = [f"B {nside}", "B 1", f"d {nside} {lon.size} " + " ".join(_hex(t) for t in zip(lon, lat, radius)), "d 1 1 " + _hex((10.0, 80.0, 50.0))]
    lines += [f"w {n} " + _hex((359.9, 89.9, 0.3)) for n in (1, 2, 12)]
    for mask in mr.hole_masks(nside).values():
        masked = np.flatnonzero(mask <= 0)
        lines.append(f"s {nside} {float(180.0).hex()} {masked.size} " + " ".join(str(p) for p in masked))
    lines.append("s 1 " + float(30.0).hex() + " 1 11")
    ask(lines)


# ---- constants and bindings --------------------------------------------------------------------------------------------------------------

def test_constants_and_symbols_match_the_headers():
    from heracles_amd import _lib, masks

    with open(os.path.join(ROOT, "heracles_amd", "csrc", "hx_masktools.h")) as f:
        header = f.read()
    m = re.search(r"KIND_C1 = (\d+), KIND_C2 = (\d+);", header)
    assert masks.KINDS == {"C1": int(m.group(1)), "C2": int(m.group(2))}
    with open(os.path.join(ROOT, "include", "hxsht.h")) as f:
        api = f.read()
    for name in ("hx_mask_discs", "hx_mask_distance", "hx_mask_taper"):
        assert name in _lib.SYMBOLS and re.search(rf"\bint {name}\(", api)


# ---- hx.mask_discs / mask_distance / apodize_mask: argument logic with the library calls stubbed out --------------------------------------

@pytest.fixture
def stub(monkeypatch):
    from heracles_amd import masks

    calls = []

    def discs(nside, mask, ndisc, lon, lat, radius, radius_all):
        calls.append(("discs", nside, ndisc, None if radius is None else np.array(radius), radius_all))
        mask[:ndisc] = 0.0

    def distance(nside, mask, max_distance, H):
        calls.append(("distance", nside, max_distance))
        H[:] = mr.angle_h(max_distance)

    def taper(nside, mask, aposize, kind, out):
        calls.append(("taper", nside, aposize, kind))
        out[:] = np.asarray(mask) * 0.5

    monkeypatch.setattr(masks, "_mask_discs", discs)
    monkeypatch.setattr(masks, "_mask_distance", distance)
    monkeypatch.setattr(masks, "_mask_taper", taper)
    return calls


def test_mask_discs_arguments(stub):
    import heracles_amd as hx

    given = np.ones(48, dtype=np.float32)
    out = hx.mask_discs(given, [1.0, 2.0, 3.0], [0.0, 1.0, 2.0], 2.5)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and (given == 1).all() and (out[:3] == 0).all() and (out[3:] == 1).all()
    assert stub[0][1:3] == (2, 3) and stub[0][3] is None and stub[0][4] == 2.5
    out = hx.mask_discs(3, np.array([1.0, 2.0]), np.array([0.0, 1.0]), np.array([2.5, 1.0]))
    assert out.shape == (108,) and stub[1][1:3] == (3, 2) and (stub[1][3] == [2.5, 1.0]).all()
    assert hx.mask_discs(1, [], [], 1.0).shape == (12,) and stub[2][2] == 0
    for bad in (np.ones(100), np.ones(0), np.ones((2, 48)), 0, 8193):
        with pytest.raises(ValueError, match="HEALPix|1-D|nside"):
            hx.mask_discs(bad, [1.0], [1.0], 1.0)
    with pytest.raises(ValueError, match="entries"):
        hx.mask_discs(np.ones(48), [1.0, 2.0], [1.0], 1.0)
    with pytest.raises(ValueError, match="entries"):
        hx.mask_discs(np.ones(48), [1.0, 2.0], [1.0, 2.0], [1.0])
    assert len(stub) == 3


def test_distance_and_apodize_arguments(stub):
    import heracles_amd as hx

    mask = np.ones(48)
    d = hx.mask_distance(mask, 30.0)
    assert isinstance(d, np.ndarray) and np.abs(d - 30.0).max() <= 1e-12 and stub[0] == ("distance", 2, 30.0)
    out = hx.apodize_mask(mask, 2.0)
    assert (out == 0.5).all() and (mask == 1).all() and stub[1] == ("taper", 2, 2.0, 1)
    hx.apodize_mask(mask, 180, kind="C2")
    assert stub[2] == ("taper", 2, 180.0, 2)
    for kind in ("Smooth", "c1", 1, None):
        with pytest.raises(ValueError, match="kind"):
            hx.apodize_mask(mask, 2.0, kind=kind)
    for bad in (0.0, -1.0, 180.5, float("nan")):
        with pytest.raises(ValueError, match="aposize"):
            hx.apodize_mask(mask, bad)
        with pytest.raises(ValueError, match="max_distance"):
            hx.mask_distance(mask, bad)
    for bad in (np.ones(100), np.ones((2, 48))):
        with pytest.raises(ValueError, match="HEALPix|1-D"):
            hx.apodize_mask(bad, 2.0)
    assert len(stub) == 3
