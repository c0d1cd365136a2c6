"""The exact pixel references (tests/pixel_reference.py) against the numpy restatements of the oracle, on the host: the oracle's
ang2pix inside the admissible set of every edge-targeted and random point, the inputs' shares, RING <-> NEST as a bijection equal to the
oracle's index formulas, and planted errors that must be caught."""

import numpy as np
import pytest

import pixel_reference as pr

RING_NEST_FULL = (1, 2, 4, 8, 32, 256)


@pytest.mark.parametrize("nside", pr.NSIDES)
def test_oracle_ang2pix_is_admissible_everywhere(oracle, nside):
    c = pr.cases(nside)
    share = pr.check_inputs(c)
    got = oracle.ang2pix_ring(nside, c["lon"], c["lat"])
    inside = pr.in_sets(got, c)
    differ = got != c["exact"]
    print(f"nside {nside}: {c['lon'].size} points, {100 * share:.1f} % of the targeted ones ambiguous, oracle != exact at {differ.sum()}"
          f" (largest margin {c['margin'][differ].max() if differ.any() else 0:.3f} delta)")
    assert inside.all(), f"oracle outside the admissible set at (lon, lat) = {c['lon'][~inside][:3]}, {c['lat'][~inside][:3]}"


def test_edge_points_hit_what_they_aim_at():
    """Both sides of each switch of the rule occur among the targeted points, and the double 2/3 itself."""
    for nside in (3, 4096):
        c = pr.cases(nside)
        th, tt = c["theta"][c["targeted"]], c["tt"][c["targeted"]]
        za = np.abs(np.cos(th))
        assert (th == 0.0).any() and (th == np.pi).any()
        for edge in (0.01, 3.14159 - 0.01):
            assert (th < edge).any() and (th > edge).any() and (np.abs(th - edge) < 1e-15).any()
        assert (za == 2.0 / 3.0).any() and (za < 2.0 / 3.0).any() and (za > 2.0 / 3.0).any()
        assert all((tt == k).any() for k in range(4)) and (tt > 3.9999999999999).any()
        assert (np.signbit(c["lon"]) & (c["lon"] > -1e-299)).sum() >= 2  # -0.0 and -1e-300
        assert c["margin"][c["targeted"]].min() < 0.05 and (c["margin"][c["targeted"]] > 20).any()


def _restated(nside, lon, lat, zscale=1.0, strict=False, wrong_cap=False):
    """``oracle.ang2pix_ring`` once more, with switches for the planted errors: z scaled, ``<`` for ``<=`` at 2/3, a cap ring off by one."""
    theta, tt = pr.front_end(lon, lat)
    z = np.cos(theta) * zscale
    have_sth = (theta < 0.01) | (theta > 3.14159 - 0.01)
    sth = np.where(have_sth, np.sin(theta), 0.0)
    za = np.abs(z)
    nl4, npix, ncap = 4 * nside, 12 * nside * nside, 2 * nside * (nside - 1)
    temp1, temp2 = nside * (0.5 + tt), nside * z * 0.75
    jp, jm = (temp1 - temp2).astype(np.int64), (temp1 + temp2).astype(np.int64)
    ir = nside + 1 + jp - jm
    ip = ((jp + jm - nside + (1 - (ir & 1)) + 1 + nl4 + nl4) >> 1) % nl4
    pe = ncap + (ir - 1) * nl4 + ip
    tp = tt - tt.astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        tmp = np.where((za < 0.99) | ~have_sth, nside * np.sqrt(3.0 * (1.0 - za)), nside * sth / np.sqrt((1.0 + za) / 3.0))
    ir2 = (tp * tmp).astype(np.int64) + ((1.0 - tp) * tmp).astype(np.int64) + (2 if wrong_cap else 1)
    ip2 = np.minimum((tt * ir2).astype(np.int64), 4 * ir2 - 1)
    belt = (za < 2.0 / 3.0) if strict else (za <= 2.0 / 3.0)
    return np.where(belt, pe, np.where(z > 0, 2 * ir2 * (ir2 - 1) + ip2, npix - 2 * ir2 * (ir2 + 1) + ip2))


@pytest.mark.parametrize("nside", [64, 4096, 2**24])
def test_planted_errors_are_caught(oracle, nside):
    c = pr.cases(nside)
    tg = c["targeted"]
    lon, lat = c["lon"], c["lat"]
    np.testing.assert_array_equal(_restated(nside, lon, lat), oracle.ang2pix_ring(nside, lon, lat))
    # a cosine off by 32 ulp, eight times the bound the admissible sets are built for
    off = _restated(nside, lon, lat, zscale=1.0 + 32 * 2.0**-52)
    assert (~pr.in_sets(off, c))[tg].any()
    assert pr.in_sets(off, c)[~tg].all()  # ... which random points do not see
    # za == 2/3 sent to the caps: harmless alone (ring nside is numbered alike by both branches), caught once the cap formula is wrong
    at = tg & (np.abs(np.cos(c["theta"])) == 2.0 / 3.0)
    assert at.any()
    assert pr.in_sets(_restated(nside, lon, lat, strict=True), c).all()
    wrong = _restated(nside, lon, lat, strict=True, wrong_cap=True)
    assert (~pr.in_sets(wrong, c))[at].any()


@pytest.mark.parametrize("nside", RING_NEST_FULL)
def test_ring_nest_exact_is_a_bijection_equal_to_the_oracle(oracle, nside):
    npix = 12 * nside**2
    p = np.arange(npix)
    q = pr.ring2nest_exact(nside, p)
    assert q.min() == 0 and q.max() == npix - 1 and np.unique(q).size == npix
    np.testing.assert_array_equal(pr.nest2ring_exact(nside, q), p)
    np.testing.assert_array_equal(pr.ring2nest_exact(nside, pr.nest2ring_exact(nside, p)), p)
    np.testing.assert_array_equal(q, oracle.ring2nest(nside, p))
    np.testing.assert_array_equal(pr.nest2ring_exact(nside, p), oracle.nest2ring(nside, p))


@pytest.mark.parametrize("nside", [4096, 8192])
def test_ring_nest_exact_equals_the_oracle_at_production_size(oracle, nside):
    npix = 12 * nside**2
    p = pr.sample_pixels(nside, np.random.default_rng(nside), 1_000_000)
    starts = pr.ring_starts(nside)
    assert np.isin(starts[:-1], p).all() and np.isin(starts[1:] - 1, p).all() and p[0] == 0 and p[-1] == npix - 1
    q = pr.ring2nest_exact(nside, p)
    assert q.min() >= 0 and q.max() < npix and np.unique(q).size == p.size
    np.testing.assert_array_equal(pr.nest2ring_exact(nside, q), p)
    np.testing.assert_array_equal(q, oracle.ring2nest(nside, p))
    np.testing.assert_array_equal(pr.nest2ring_exact(nside, p), oracle.nest2ring(nside, p))
    np.testing.assert_array_equal(pr.ring2nest_exact(nside, pr.nest2ring_exact(nside, p)), p)
