"""The rule of ``hx.mask_polygons`` restated in numpy by brute force, independent of the library's code: the full
(npix x edges) table of d for every polygon, orientation, validity and the inside test from it; ``rectangle_polygons`` restated in
float64 and in long double; the shapes the tests share.  numpy multiplies and adds one rounding at a time (no fused multiply-adds),
which is the arithmetic the rule prescribes."""

import functools

import numpy as np

from jkregions_reference import pix2vec_ring

GAP_MIN = 1e-9  # no pixel / edge pair of a test's inputs may have |d| / |n_e| below this: the comparisons may then be exact


@functools.lru_cache(maxsize=None)
def centres(nside):
    """The pixel centres (npix, 3); computed once per nside and shared: not to be written to."""
    return pix2vec_ring(nside, np.arange(12 * nside * nside))


def vertices(lon, lat):
    """v_k = (cos lat cos lon, cos lat sin lon, sin lat), (n, 3)."""
    lon, lat = np.radians(np.asarray(lon, dtype=np.float64)), np.radians(np.asarray(lat, dtype=np.float64))
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=-1)


def normals(v):
    """n_e = v_e x v_(e+1), unnormalised, each component the difference of two products in the written order: (n, 3)."""
    w = np.roll(v, -1, axis=0)
    return np.stack([v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1], v[:, 2] * w[:, 0] - v[:, 0] * w[:, 2], v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0]], axis=-1)


def d_table(u, n):
    """d(u, e) = (n_x u_x + n_y u_y) + n_z u_z for every u (m, 3) and edge (k, 3): (m, k)."""
    return (u[:, None, 0] * n[None, :, 0] + u[:, None, 1] * n[None, :, 1]) + u[:, None, 2] * n[None, :, 2]


def orientation(v):
    return 1.0 if d_table(v[2:3], normals(v)[0:1])[0, 0] > 0 else -1.0


def is_valid(lon, lat):
    """Finite coordinates, |lat| <= 90, 3 .. 64 vertices, and sigma d(v_k, e) > 0 for every edge e and every vertex k that is not one of
    its endpoints."""
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    n = lon.size
    if not 3 <= n <= 64 or lat.size != n or not (np.isfinite(lon).all() and np.isfinite(lat).all() and (np.abs(lat) <= 90).all()):
        return False
    v = vertices(lon, lat)
    t = orientation(v) * d_table(v, normals(v))  # [vertex, edge]
    k, e = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    other = (k != e) & (k != (e + 1) % n)
    return bool((t[other] > 0).all())


def signed_table(nside, lon, lat):
    """(sigma d(v_p, e) for every pixel and edge: (npix, n), |n_e|: (n,))."""
    v = vertices(lon, lat)
    n = normals(v)
    return orientation(v) * d_table(centres(nside), n), np.sqrt((n * n).sum(axis=1))


def inside(nside, lon, lat):
    """The pixels whose centres are inside the polygon: sigma d(v_p, e) >= 0 for every edge; asserts that no pixel / edge pair lies
    within GAP_MIN of an edge's great circle, so that no pixel is left out of a comparison."""
    t, norm = signed_table(nside, lon, lat)
    gap = float((np.abs(t) / norm).min())
    assert gap >= GAP_MIN, (nside, gap)
    return (t >= 0).all(axis=1)


def gap(nside, polygons):
    """The smallest |d| / |n_e| over all pixels and all edges of all polygons [(lon, lat), ...]."""
    best = np.inf
    for lon, lat in polygons:
        t, norm = signed_table(nside, lon, lat)
        best = min(best, float((np.abs(t) / norm).min()))
    return best


def mask_polygons(mask, polygons, value=0.0):
    """mask with ``value`` on every pixel inside at least one of the polygons [(lon, lat), ...], every one of them valid."""
    mask = np.array(mask, dtype=np.float64)
    nside = int(round((mask.size / 12) ** 0.5))
    for lon, lat in polygons:
        assert is_valid(lon, lat)
        mask[inside(nside, lon, lat)] = value
    return mask


def flatten(polygons):
    """(lon, lat, offsets) of a list of polygons, for the 1-D form of the call."""
    offsets = np.concatenate([[0], np.cumsum([len(lon) for lon, _ in polygons])]).astype(np.int64)
    if not polygons:
        return np.zeros(0), np.zeros(0), offsets
    return np.concatenate([np.asarray(lon, dtype=np.float64) for lon, _ in polygons]), np.concatenate([np.asarray(lat, dtype=np.float64) for _, lat in polygons]), offsets


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------

def _rad(dtype):
    """pi / 180 in dtype (np.pi itself is a float64)."""
    return np.arctan(dtype(1.0)) * dtype(4.0) / dtype(180.0)


def _frame(lon, lat, dtype=np.float64):
    """The centre c, east = (-sin lon, cos lon, 0) and north = (-sin lat cos lon, -sin lat sin lon, cos lat) in dtype."""
    lo, la = dtype(lon) * _rad(dtype), dtype(lat) * _rad(dtype)
    c = np.array([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], dtype=dtype)
    east = np.array([-np.sin(lo), np.cos(lo), dtype(0.0)], dtype=dtype)
    north = np.array([-np.sin(la) * np.cos(lo), -np.sin(la) * np.sin(lo), np.cos(la)], dtype=dtype)
    return c, east, north


def _lonlat(p):
    lon = np.degrees(np.arctan2(p[..., 1], p[..., 0])) % 360.0
    return lon, np.degrees(np.arctan2(p[..., 2], np.hypot(p[..., 0], p[..., 1])))


def regular_ngon(lon, lat, r, n):
    """Vertices at cos r c + sin r (cos t north + sin t east), t = 0.3 + 2 pi k / n, all angles in degrees: (lon [n], lat [n])."""
    c, east, north = _frame(lon, lat)
    t = 0.3 + 2.0 * np.pi * np.arange(n) / n
    r = np.radians(r)
    return _lonlat(np.cos(r) * c[None, :] + np.sin(r) * (np.cos(t)[:, None] * north[None, :] + np.sin(t)[:, None] * east[None, :]))


def rectangle_vectors(lon, lat, length, width, angle, dtype=np.float64):
    """The four corners of the gnomonic rectangle as unit vectors (4, 3) in ``dtype`` (np.longdouble for the restatement the library's
    ``rectangle_polygons`` is held against): normalise(c +- tan(length / 2) a +- tan(width / 2) b), a = cos(angle) north + sin(angle)
    east, b = -sin(angle) north + cos(angle) east, in the order (+, +), (+, -), (-, -), (-, +)."""
    c, east, north = _frame(lon, lat, dtype=dtype)
    rad = _rad(dtype)
    an = dtype(angle) * rad
    a = np.cos(an) * north + np.sin(an) * east
    b = -np.sin(an) * north + np.cos(an) * east
    tl, tw = np.tan(dtype(length) * rad / dtype(2.0)), np.tan(dtype(width) * rad / dtype(2.0))
    p = np.stack([c + sa * tl * a + sb * tw * b for sa, sb in ((1, 1), (1, -1), (-1, -1), (-1, 1))])
    return p / np.sqrt((p * p).sum(axis=1))[:, None]


def rectangle(lon, lat, length, width, angle):
    """(lon [4], lat [4]) of the gnomonic rectangle, in float64."""
    return _lonlat(rectangle_vectors(lon, lat, length, width, angle))


def named_shapes():
    """{name: (lon, lat)}: the shapes at the places the kernels can go wrong."""
    return {
        "pentagon over the north pole": regular_ngon(37.0, 88.3, 7.3, 5),
        "triangle over the south pole": regular_ngon(211.0, -89.1, 11.7, 3),
        "across phi = 0": rectangle(359.2, 23.7, 31.3, 9.1, 63.0),
        "on the cap / belt transition": rectangle(123.4, 41.8103, 17.9, 6.3, -20.0),
        "on the equator": rectangle(181.7, 0.37, 44.1, 5.7, 81.0),
        "thin trail": rectangle(77.3, -31.9, 121.7, 2.9, 37.0),
        "64-gon": regular_ngon(301.3, -12.9, 23.1, 64),
        "large 7-gon": regular_ngon(141.9, 17.3, 85.1, 7),
        "sliver": rectangle(250.1, 55.3, 170.3, 4.7, 12.0),
        "tiny rectangle holding no pixel centre": rectangle(10.1, 10.3, 0.011, 0.007, 5.0),
    }


def long_triangle():
    """Two vertices 4 degrees apart and the third 175 degrees away: valid, and its bounding cap is wider than a hemisphere."""
    return np.array([3.1, 2.3, 177.9]), np.array([-1.3, 2.9, 0.7])


def random_rectangles(count, seed, length=(2.0, 40.0), width=(1.0, 15.0)):
    """[(lon, lat), ...] of rectangles at random places and angles, sizes in degrees."""
    rng = np.random.default_rng(seed)
    lon, lat = rng.uniform(0, 360, count), np.degrees(np.arcsin(rng.uniform(-1, 1, count)))
    ln, wd, an = rng.uniform(*length, count), rng.uniform(*width, count), rng.uniform(0, 360, count)
    return [rectangle(*t) for t in zip(lon, lat, ln, wd, an)]


def reverse(polygon):
    """The same polygon in the other winding."""
    lon, lat = polygon
    return np.asarray(lon)[::-1].copy(), np.asarray(lat)[::-1].copy()


def test_shapes(seed=7):
    """The named shapes, the long triangle and 40 random rectangles: [(name, (lon, lat)), ...]."""
    out = list(named_shapes().items()) + [("long triangle", long_triangle())]
    return out + [(f"random rectangle {k}", p) for k, p in enumerate(random_rectangles(40, seed))]


test_shapes.__test__ = False  # (a helper, not a test)
