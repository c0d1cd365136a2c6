"""Exact references for the HEALPix pixelisation, host only (numpy integers and mpmath): the pixel of a point with the set of pixels a
correct double-precision evaluation may return (``admissible``), points aimed at pixel edges (``edge_points``), and RING <-> NEST from
the projection of the pixel centre (``ring2nest_exact`` / ``nest2ring_exact``).

The point rule
--------------
healpy's ``ang2pix(nside, lon, lat, lonlat=True)`` has a front end that IEEE arithmetic defines completely,

    theta_d = pi/2 - radians(lat),   phi_d = radians(lon),   tt_d = fmodulo(phi_d * (2/pi), 4)

(every operation rounds on its own, fmod is exact, no libm), so ``front_end`` evaluates it in numpy as ``oracle.ang2pix_ring`` does and
the reference takes (theta_d, tt_d) as its inputs: near a pole the cancellation in theta_d belongs to the definition.  From there the
rule (healpix_cxx loc2pix, RING) is, with z = cos(theta_d), za = |z|:

    belt (za <= 2/3):  jp = floor(nside (0.5 + tt - 0.75 z)),  jm = floor(nside (0.5 + tt + 0.75 z))
    caps (za >  2/3):  tmp = nside sqrt(3 (1 - za)),  tp = tt - floor(tt),
                       jp = floor(tp tmp),  jm = floor((1 - tp) tmp),  ir = jp + jm + 1,  ip = floor(tt ir)

and integer arithmetic from there on.  ``analyse`` evaluates z and the floor arguments in mpmath at 200 bits; ``exact_pixel`` takes
plain floors.  The admissible set holds every pixel reached when each floor argument a is replaced by any value in [a - delta, a + delta]
(never below 0: the double expressions are sums and products of non-negative terms under monotone rounding); within the window of
za = 2/3 both branches contribute.  Candidates outside a branch's rings (belt ring index outside 1..2 nside + 1, cap ring above nside)
are no pixel of that branch and are dropped.

delta: forward error of the double algorithm
--------------------------------------------
U = 2^-52.  A double operation that is correctly rounded (+, *, /, sqrt, as assumed here) has relative error <= U/2; cos and sin are
assumed within K = 4 ulp (OpenCL's bound for double), i.e. relative error <= K U.  tt, and tp = tt - floor(tt) (exact: tt < 4), carry no
error.  Second-order terms are covered by rounding each sum of first-order terms up.

belt.  The double code forms temp1 = nside * (0.5 + tt), temp2 = nside * z * 0.75, then temp1 -+ temp2.
    0.5 + tt <= 4.5: rounding <= ulp(4.5)/2 = 2 U, times nside                         2      nside U
    nside * (.) <= 4.5 nside: rounding <= 4.5 nside U/2                                 2.25   nside U
    z: K U |z|, |z| <= 2/3 (1 + K U), times 0.75 nside                                  0.5 K  nside U
    nside * z (<= 2/3 nside), then * 0.75 (<= nside/2): two roundings, scaled to temp2  0.5    nside U
    temp1 -+ temp2 <= 5 nside: rounding                                                 2.5    nside U
  sum 0.5 K + 7.25; used: delta_belt = nside (0.5 K + 8) U.

caps, first form tmp = nside * sqrt(3 * (1 - za)) (taken when za < 0.99 or theta is not within 0.01 of a pole).
    za: K U za absolute; 1 - za is exact for za >= 1/2 (Sterbenz): relative K U za / (1 - za)
    3 * (.): U/2;  sqrt halves what it is given and rounds: 0.5 K U za / (1 - za) + U/4 + U/2;  nside * (.): U/2
  tmp: relative 0.5 K U za / (1 - za) + 1.25 U.  tp * tmp adds U/2; (1 - tp) * tmp adds U/2 for 1 - tp (absolute 2^-53, times tmp) and
  U/2 for the product.  Sum 0.5 K za / (1 - za) + 2.25; used: delta_cap = tmp (0.5 K za / (1 - za) + 3) U, which carries the
  1 / (1 - za) amplification of the cosine's error (at theta = 0.01, the last point of this form, it is 2 10^4).

caps, second form tmp = nside * sth / sqrt((1 + za) / 3), sth = sin(theta_d) (theta within 0.01 of a pole and za >= 0.99; in exact
arithmetic the same number, since 1 - za^2 = sth^2).
    sth: K U;  nside * sth: U/2;  1 + za (about 2, za off by K U): 0.5 K U + U/2;  / 3: U/2;  sqrt: 0.25 K U + U/2 + U/2;  the division: U/2
  tmp: relative (1.25 K + 2) U; the products add at most U as above.  Used: delta_sth = tmp (1.25 K + 4) U.

ip = floor(tt * ir): ir is an exact integer, the product rounds once: delta_ip = tt ir U (twice the bound).  The double code caps ip
at 4 ir - 1; so does the reference.

Where za is within K U of 0.99 either form may be taken and the larger delta is used.  The window of za = 2/3 is (K + 1) U (K U za of
the cosine, and the distance of the double constant 2/3 from 2/3).  These constants are below the (0.75 K + 27, 0.5 K /(1 - za) + 6,
2 K + 8) of the first prototype: every term is listed above.
"""

import functools

import mpmath as mp
import numpy as np

K_ULP = 4
U = 2.0**-52
_PREC = 200


# ---- the IEEE front end ----------------------------------------------------------------------------------------------------------------
def front_end(lon, lat):
    """(theta_d, tt_d) of (lon, lat) in degrees, in numpy, operation for operation as ``oracle.ang2pix_ring`` forms them."""
    lon = np.asarray(lon, dtype=np.float64)
    lat = np.asarray(lat, dtype=np.float64)
    theta = np.pi / 2.0 - np.radians(lat)
    phi = np.radians(lon)
    v = phi * 0.6366197723675813430755350534900574
    with np.errstate(invalid="ignore"):
        neg = np.fmod(v, 4.0) + 4.0
        tt = np.where(v >= 0, np.where(v < 4.0, v, np.fmod(v, 4.0)), np.where(neg == 4.0, 0.0, neg))
    return theta, tt


def theta_valid(theta_d):
    """healpy's check_theta_valid on theta_d: 0 <= theta <= pi + 1e-5 (a NaN fails)."""
    theta_d = np.asarray(theta_d, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (theta_d >= 0.0) & (theta_d <= np.pi + 1e-5)


# ---- exact pixel and admissible set ----------------------------------------------------------------------------------------------------
def _belt_pixel(nside, jp, jm):
    ir = nside + 1 + jp - jm
    if not 1 <= ir <= 2 * nside + 1:
        return None
    nl4 = 4 * nside
    kshift = 1 - (ir & 1)
    ip = ((jp + jm - nside + kshift + 1 + 2 * nl4) >> 1) % nl4
    return 2 * nside * (nside - 1) + (ir - 1) * nl4 + ip


def _cap_ring(nside, jp, jm):
    ir = jp + jm + 1
    return ir if 1 <= ir <= nside else None


def _cap_pixel(nside, ir, ip, north):
    ip = min(ip, 4 * ir - 1)
    return 2 * ir * (ir - 1) + ip if north else 12 * nside * nside - 2 * ir * (ir + 1) + ip


def _floors(a, delta):
    """(plain floor, the floors reached within +-delta, distance to the nearest integer in units of delta)."""
    f = int(mp.floor(a))
    lo = int(mp.floor(a - delta)) if a - delta > 0 else 0
    hi = int(mp.floor(a + delta))
    dist = min(a - f, f + 1 - a)
    return f, sorted({lo, hi}), (dist / delta if delta > 0 else mp.inf)


def analyse(nside, theta_d, tt_d):
    """(exact_pixel, admissible set, margin) of a point given by the doubles (theta_d, tt_d), 0 <= theta_d <= pi.  margin is the
    distance of the nearest floor argument from an integer (or of za from 2/3), in units of its delta: the set has one pixel iff > 1."""
    theta_d, tt_d, nside = float(theta_d), float(tt_d), int(nside)
    if not (0.0 <= theta_d <= np.pi) or not (0.0 <= tt_d < 4.0):
        raise ValueError(f"analyse: theta_d={theta_d!r} tt_d={tt_d!r} outside 0 <= theta <= pi, 0 <= tt < 4")
    with mp.workprec(_PREC):
        theta, tt = mp.mpf(theta_d), mp.mpf(abs(tt_d))
        z = mp.cos(theta)
        za = abs(z)
        third2 = mp.mpf(2) / 3
        window = (K_ULP + 1) * U
        margin = abs(za - third2) / window
        both = margin <= 1
        in_belt = za <= third2
        pixels = set()
        exact = None
        if in_belt or both:
            delta = nside * (0.5 * K_ULP + 8) * U
            fp, cp, mp_ = _floors(nside * (mp.mpf(0.5) + tt - mp.mpf(0.75) * z), delta)
            fm, cm, mm = _floors(nside * (mp.mpf(0.5) + tt + mp.mpf(0.75) * z), delta)
            if in_belt:
                exact = _belt_pixel(nside, fp, fm)
                margin = min(margin, mp_, mm)
            for jp in cp:
                for jm in cm:
                    p = _belt_pixel(nside, jp, jm)
                    if p is not None:
                        pixels.add(p)
        if not in_belt or both:
            have_sth = theta_d < 0.01 or theta_d > 3.14159 - 0.01
            sth = abs(mp.sin(theta))
            # the two forms are the same number; the second keeps its digits next to a pole
            tmp = nside * sth / mp.sqrt((1 + za) / 3) if za > 0.9 else nside * mp.sqrt(3 * (1 - za))
            d_first = tmp * (0.5 * K_ULP * za / (1 - za) + 3) * U if za < 1 else mp.mpf(0)
            d_sth = tmp * (1.25 * K_ULP + 4) * U
            if not have_sth or za < mp.mpf(0.99) - K_ULP * U:
                delta = d_first
            elif za > mp.mpf(0.99) + K_ULP * U:
                delta = d_sth
            else:
                delta = max(d_first, d_sth)
            tp = tt - mp.floor(tt)
            fp, cp, mp_ = _floors(tp * tmp, delta)
            fm, cm, mm = _floors((1 - tp) * tmp, delta)
            north = z > 0
            if not in_belt:
                ir = _cap_ring(nside, fp, fm)
                fi, _, mi = _floors(tt * ir, tt * ir * U)
                exact = _cap_pixel(nside, ir, fi, north)
                margin = min(margin, mp_, mm, mi)
            for jp in cp:
                for jm in cm:
                    ir = _cap_ring(nside, jp, jm)
                    if ir is None:
                        continue
                    _, ci, _ = _floors(tt * ir, tt * ir * U)
                    for ip in ci:
                        pixels.add(_cap_pixel(nside, ir, ip, north))
        return exact, pixels, float(margin)


def admissible(nside, theta_d, tt_d):
    """(exact_pixel, set_of_pixels) of the point (theta_d, tt_d): see the module docstring."""
    exact, pixels, _ = analyse(nside, theta_d, tt_d)
    return exact, pixels


# ---- points aimed at edges -------------------------------------------------------------------------------------------------------------
def ulp_step(x, n):
    """x moved by n units in the last place (n an integer or an array of integers), through zero where needed."""
    i = np.array(x, dtype=np.float64).view(np.int64)
    low = np.int64(-(2**63))
    i = np.where(i < 0, low - i, i) + np.asarray(n, dtype=np.int64)
    return np.where(i < 0, low - i, i).view(np.float64)


_NUDGES = [0] + [s * k for k in (1, 3, *(2**e for e in range(3, 11))) for s in (1, -1)]


def _nudged(lon, lat):
    """The point as drawn, and moved in lat and in lon by +-1, +-3 and +-2^k ulp (k = 3..10): 41 points."""
    n = np.array(_NUDGES[1:])
    return (np.concatenate([[lon], np.full(n.size, lon), ulp_step(lon, n)]),
            np.concatenate([[lat], ulp_step(lat, n), np.full(n.size, lat)]))


def _belt_edge(nside, rng, which, ring=None):
    """(lon, lat) on the edge nside (0.5 + tt -+ 0.75 z) = k of the belt, near the given ring (nside .. 3 nside) if one is named."""
    while True:
        tt = rng.uniform(0.0, 4.0)
        if ring is None:
            z0 = rng.uniform(-2.0 / 3.0, 2.0 / 3.0)
        else:
            z0 = (2 * nside - ring) * 2.0 / (3.0 * nside) + rng.uniform(-1.0, 1.0) / (3.0 * nside)
        sign = -1.0 if which == "jp" else 1.0
        k = np.rint(nside * (0.5 + tt + sign * 0.75 * z0))
        z = sign * (k / nside - 0.5 - tt) / 0.75
        if abs(z) < 2.0 / 3.0:
            return 90.0 * tt, np.degrees(np.arcsin(z))


def _cap_edge(nside, rng, which, north):
    """(lon, lat) on the edge tp tmp = k (jp) or (1 - tp) tmp = k (jm) of a cap; nside = 1 has no such edge inside a cap."""
    while True:
        tp = rng.uniform(0.02, 0.98)
        k = max(1.0, np.rint(tp * rng.uniform(0.0, nside)))
        tmp = k / tp
        if tmp < nside:
            break
    tt = rng.integers(0, 4) + (tp if which == "jp" else 1.0 - tp)
    theta = 2.0 * np.arcsin(tmp / (nside * np.sqrt(6.0)))  # 1 - cos(theta) = tmp^2 / (3 nside^2)
    lat = 90.0 - np.degrees(theta)
    return 90.0 * tt, lat if north else -lat


def _random_lat(rng, where):
    if where == "belt":
        return np.degrees(np.arcsin(rng.uniform(-0.6, 0.6)))
    lat = np.degrees(np.arcsin(rng.uniform(0.7, 0.9999)))
    return lat if where == "north" else -lat


def edge_points(nside, rng, n=1500):
    """About n points (lon, lat in degrees), every one valid (0 <= theta_d <= pi), aimed at the edges of the rule above.

    As drawn and moved by +-1 ulp in lat: lat = +-90 and +-(90 - 2^-k), k = 1..40.  As drawn: theta_d to either side of 0.01 and of
    3.14159 - 0.01 (the switch between the two cap forms).  As drawn and moved by +-1 ulp in lat and in lon: lon = 360 - eps, -0.0 and
    -1e-300 in a cap and in the belt.  As drawn and moved by +-1, +-3, +-8 ulp in lon: tt at the integers, lon = 90 k and shifted by
    +-360 and +-720, in both caps and in the belt.  As drawn and with all 40 nudges of ``_nudged``: |z| = 2/3 in both hemispheres (the
    nudges of +-1 and +-3 ulp reach the double 2/3 and either side of it) and, filling up to n, points solved for an edge: belt jp and
    jm edges anywhere and next to the rings nside, 2 nside and 3 nside, and the jp and jm edges of both caps."""
    lons, lats = [], []

    def emit(lo, la):
        lons.append(np.atleast_1d(np.asarray(lo, dtype=np.float64)))
        lats.append(np.atleast_1d(np.asarray(la, dtype=np.float64)))

    for sign in (1.0, -1.0):
        for lat in [90.0] + [90.0 - 2.0**-k for k in range(1, 41)]:
            lon = rng.uniform(0.0, 360.0)
            emit(np.full(3, lon), ulp_step(sign * lat, np.array([0, 1, -1])))
    for th in (0.01, 3.14159 - 0.01):
        emit(np.full(9, rng.uniform(0.0, 360.0)), ulp_step(90.0 - np.degrees(th), np.arange(-4, 5)))
    for lon in (np.nextafter(360.0, 0.0), -0.0, -1e-300):
        for where in ("north", "belt"):
            lat = _random_lat(rng, where)
            emit(ulp_step(lon, np.array([0, 0, 0, 1, -1])), ulp_step(lat, np.array([0, 1, -1, 0, 0])))
    for i, lon in enumerate(90.0 * k + s for k in range(4) for s in (0.0, 360.0, -360.0, 720.0, -720.0)):
        lat = _random_lat(rng, ("north", "south", "belt")[i % 3])
        emit(ulp_step(lon, np.array([0, 1, -1, 3, -3, 8, -8])), np.full(7, lat))
    for sign in (1.0, -1.0):
        emit(*_nudged(rng.uniform(0.0, 360.0), sign * np.degrees(np.arcsin(2.0 / 3.0))))
    makers = [lambda: _belt_edge(nside, rng, "jp"), lambda: _belt_edge(nside, rng, "jm"),
              lambda: _belt_edge(nside, rng, "jp", nside), lambda: _belt_edge(nside, rng, "jm", 2 * nside),
              lambda: _belt_edge(nside, rng, "jp", 3 * nside), lambda: _belt_edge(nside, rng, "jm", nside),
              lambda: _belt_edge(nside, rng, "jp", 2 * nside), lambda: _belt_edge(nside, rng, "jm", 3 * nside)]
    if nside > 1:
        makers += [lambda: _cap_edge(nside, rng, "jp", True), lambda: _cap_edge(nside, rng, "jm", True),
                   lambda: _cap_edge(nside, rng, "jp", False), lambda: _cap_edge(nside, rng, "jm", False)]
    have = sum(a.size for a in lons)
    for i in range(max(len(makers), (n - have) // (2 * len(_NUDGES) - 1))):
        emit(*_nudged(*makers[i % len(makers)]()))
    lon, lat = np.concatenate(lons), np.concatenate(lats)
    theta, _ = front_end(lon, lat)
    keep = (theta >= 0.0) & (theta <= np.pi)
    return lon[keep], lat[keep]


def random_points(rng, n=600):
    """n points uniform on the sphere, lon over three turns."""
    return rng.uniform(-360.0, 720.0, n), np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n)))


NSIDES = (1, 2, 3, 64, 4096, 8192, 2**24)


@functools.lru_cache(maxsize=None)
def cases(nside):
    """The points every test of one nside shares, analysed once: dict of read-only arrays lon, lat, theta, tt, targeted (bool), exact,
    margin, and the list ``sets`` of admissible sets."""
    rng = np.random.default_rng(1000 + nside)
    tlon, tlat = edge_points(nside, rng)
    rlon, rlat = random_points(rng)
    lon, lat = np.concatenate([tlon, rlon]), np.concatenate([tlat, rlat])
    theta, tt = front_end(lon, lat)
    res = [analyse(nside, t, x) for t, x in zip(theta, tt)]
    out = {"lon": lon, "lat": lat, "theta": theta, "tt": tt, "targeted": np.arange(lon.size) < tlon.size,
           "exact": np.array([r[0] for r in res], dtype=np.int64), "margin": np.array([r[2] for r in res]),
           "nset": np.array([len(r[1]) for r in res])}
    for a in out.values():
        a.setflags(write=False)
    out["sets"] = [frozenset(r[1]) for r in res]
    return out


def check_inputs(c):
    """The conditions on the inputs that keep a test from passing by calling everything ambiguous."""
    amb, tg = c["nset"] > 1, c["targeted"]
    assert all(e in s for e, s in zip(c["exact"], c["sets"])), "exact pixel outside its own admissible set"
    assert c["nset"].max() <= 6, f"an admissible set of {c['nset'].max()} pixels"
    assert not amb[~tg].any(), f"{amb[~tg].sum()} random points are ambiguous"
    share = amb[tg].mean()
    assert 0.2 <= share <= 0.8, f"{100 * share:.1f} % of the targeted points are ambiguous"
    return share


def in_sets(pix, c):
    return np.array([int(p) in s for p, s in zip(pix, c["sets"])])


# ---- RING <-> NEST from the projection of the pixel centre, integers only ---------------------------------------------------------------
def _spread(v):
    v = (v | (v << 16)) & 0x0000FFFF0000FFFF
    v = (v | (v << 8)) & 0x00FF00FF00FF00FF
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0F
    v = (v | (v << 2)) & 0x3333333333333333
    return (v | (v << 1)) & 0x5555555555555555


def _squeeze(v):
    v = v & 0x5555555555555555
    v = (v | (v >> 1)) & 0x3333333333333333
    v = (v | (v >> 2)) & 0x0F0F0F0F0F0F0F0F
    v = (v | (v >> 4)) & 0x00FF00FF00FF00FF
    v = (v | (v >> 8)) & 0x0000FFFF0000FFFF
    return (v | (v >> 16)) & 0x00000000FFFFFFFF


@functools.lru_cache(maxsize=None)
def ring_starts(nside):
    """First pixel of ring i = 1 .. 4 nside - 1 at index i - 1, and npix at the end: cumulative ring lengths."""
    i = np.arange(1, 4 * nside, dtype=np.int64)
    length = 4 * np.minimum(np.minimum(i, nside), 4 * nside - i)
    s = np.concatenate([[0], np.cumsum(length)])
    s.setflags(write=False)
    return s


def ring2nest_exact(nside, p):
    """NEST index of the RING pixels p (nside a power of two).  The centre of pixel j = 1.. of ring i lies at tt = (j - fodd) / nr
    (nr pixels per quadrant of the ring; fodd = 1/2 in the caps and on the belt rings with i - nside even, else 1) and
    z = (2 nside - i) 2 / (3 nside) in the belt, tmp = i (from its own pole) in the caps.  Put into the rule of the module docstring the
    floors become integer divisions: belt 2 jp = 2 j - 2 fodd + i - nside, 2 jm = 2 j - 2 fodd + 3 nside - i (both odd: a centre
    lies on no edge); caps jp = j - 1 - ntt i, jm = i - j + ntt i with ntt = (j - 1) div i the quadrant."""
    p = np.asarray(p, dtype=np.int64)
    nside = int(nside)
    starts = ring_starts(nside)
    i = np.searchsorted(starts, p, side="right")
    j = p - starts[i - 1] + 1
    # belt
    fodd2 = np.where((i - nside) % 2 == 0, 1, 2)
    jp = (2 * j - fodd2 + i - nside) // 2
    jm = (2 * j - fodd2 + 3 * nside - i) // 2
    ifp, ifm = jp // nside, jm // nside
    face_b = np.where(ifp == ifm, (ifp & 3) + 4, np.where(ifp < ifm, ifp, ifm + 8))
    ix_b, iy_b = jm % nside, nside - 1 - jp % nside
    # caps, ring counted from the pole of its hemisphere
    north = i < nside
    south = i > 3 * nside
    ic = np.where(south, 4 * nside - i, np.maximum(i, 1))
    ntt = np.minimum(3, (j - 1) // ic)
    jpc, jmc = j - 1 - ntt * ic, ic - j + ntt * ic
    face = np.where(north, ntt, np.where(south, ntt + 8, face_b))
    ix = np.where(north, nside - 1 - jmc, np.where(south, jpc, ix_b))
    iy = np.where(north, nside - 1 - jpc, np.where(south, jmc, iy_b))
    return face * nside * nside + _spread(ix) + (_spread(iy) << 1)


def nest2ring_exact(nside, q):
    """RING index of the NEST pixels q: the relations of ``ring2nest_exact`` solved for (i, j).  A face fixes (ifp, ifm) -- polar north
    (f, f + 1), equatorial (f - 4, f - 4), polar south (f - 7, f - 8) -- so jp = ifp nside + nside - 1 - iy, jm = ifm nside + ix, and
    the two odd numerators 2 jp + 1, 2 jm + 1 give i = 2 nside - (jm - jp) and 2 j = jp + jm + 1 - nside + 2 fodd (mod 8 nside).  A
    pixel of a polar face whose cap ring jp + jm + 1 (from the face's own corner) is below nside lies in the cap."""
    q = np.asarray(q, dtype=np.int64)
    nside = int(nside)
    npface = nside * nside
    face, pf = q // npface, q % npface
    ix, iy = _squeeze(pf), _squeeze(pf >> 1)
    starts = ring_starts(nside)
    # belt
    ifp = np.where(face < 4, face, np.where(face < 8, face - 4, face - 7))
    ifm = np.where(face < 4, face + 1, np.where(face < 8, face - 4, face - 8))
    jp, jm = ifp * nside + nside - 1 - iy, ifm * nside + ix
    i_b = 2 * nside - (jm - jp)
    fodd2 = np.where((i_b - nside) % 2 == 0, 1, 2)
    j_b = (jp + jm + 1 - nside + fodd2) // 2
    j_b = (j_b - 1) % (4 * nside) + 1
    # caps
    jpn, jmn = nside - 1 - iy, nside - 1 - ix
    i_n = jpn + jmn + 1
    j_n = jpn + 1 + face * i_n
    i_s = ix + iy + 1
    j_s = ix + 1 + (face - 8) * i_s
    north = (face < 4) & (i_n < nside)
    south = (face >= 8) & (i_s < nside)
    i = np.where(north, i_n, np.where(south, 4 * nside - i_s, i_b))
    j = np.where(north, j_n, np.where(south, j_s, j_b))
    return starts[i - 1] + j - 1


def sample_pixels(nside, rng, nrandom):
    """Every ring's first and last pixel, the pixels either side of ncap and of npix - ncap, the twelve face corners (the four corner
    pixels of every face, given as NEST indices turned to RING), and nrandom random pixels: sorted unique RING indices."""
    starts = ring_starts(nside)
    npix, ncap, npface = 12 * nside * nside, 2 * nside * (nside - 1), nside * nside
    corners = np.array([f * npface + c for f in range(12) for c in (0, (npface - 1) // 3, 2 * ((npface - 1) // 3), npface - 1)])
    sel = np.concatenate([starts[:-1], starts[1:] - 1, [max(ncap - 1, 0), ncap, npix - ncap - 1, min(npix - ncap, npix - 1)],
                          nest2ring_exact(nside, corners), rng.integers(0, npix, nrandom)])
    return np.unique(sel)
