"""hx_ang2pix_ring and every path that places a catalogue row in a pixel, at pixel edges and up to the largest nside, against the exact
reference of tests/pixel_reference.py: where the reference leaves one pixel the kernel must give it; within delta of an edge it must
give one of the admissible pixels; map_values, map_catalogs, the one-pass views and FootprintFilter must place each row in the pixel
ang2pix_ring gave; and the accept/raise decision at the poles follows healpy's rule on theta_d."""

import warnings

import numpy as np
import pytest

import pixel_reference as pr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nside", pr.NSIDES)
def test_ang2pix_exact_off_the_edges_admissible_on_them(oracle, nside):
    """Measured on the MI355X (points, kernel != oracle, kernel != exact pixel, largest margin of such a point in delta):
    see DESIGN.md, "Pixelisation: what is pinned"."""
    from heracles_amd.mapper import ang2pix_ring

    c = pr.cases(nside)
    share = pr.check_inputs(c)
    got = ang2pix_ring(nside, c["lon"], c["lat"])
    vs_oracle = got != oracle.ang2pix_ring(nside, c["lon"], c["lat"])
    vs_exact = got != c["exact"]
    print(f"\nnside {nside}: {got.size} points ({100 * share:.1f} % of the targeted ones ambiguous): kernel != oracle at {vs_oracle.sum()}, "
          f"kernel != exact at {vs_exact.sum()}, largest margin of those {c['margin'][vs_oracle | vs_exact].max(initial=0.0):.3f} delta")
    one = c["nset"] == 1
    bad = one & vs_exact
    assert not bad.any(), (f"{bad.sum()} unambiguous points in another pixel, first (lon, lat) = ({c['lon'][bad][0]!r}, {c['lat'][bad][0]!r}): "
                           f"kernel {got[bad][0]}, exact {c['exact'][bad][0]}, margin {c['margin'][bad][0]:.2f} delta")
    inside = pr.in_sets(got, c)
    assert inside.all(), (f"{(~inside).sum()} points outside their admissible set, first (lon, lat) = ({c['lon'][~inside][0]!r}, "
                          f"{c['lat'][~inside][0]!r}): kernel {got[~inside][0]}, set {sorted(c['sets'][np.flatnonzero(~inside)[0]])}")


def _counts(ipix, weights, npix):
    import torch

    ip = torch.as_tensor(ipix, device="cuda")
    return torch.stack([torch.bincount(ip, minlength=npix).to(torch.float64),
                        torch.bincount(ip, weights=torch.as_tensor(weights, device="cuda"), minlength=npix)])


@pytest.mark.parametrize("nside", [64, 4096])
def test_one_pixel_per_point_on_every_path(nside):
    """The targeted points through map_values, map_catalogs (k_cat_prepare), two views in one pass (k_sel_prepare) and FootprintFilter:
    hit counts and the sums of the weights j + 1 (integers: exact in any order) equal those of ang2pix_ring's pixels, bit for bit."""
    import torch

    import heracles_amd as hx
    from heracles_amd.mapper import ang2pix_ring, map_values

    c = pr.cases(nside)
    lon, lat = c["lon"][c["targeted"]], c["lat"][c["targeted"]]
    n, npix = lon.size, 12 * nside**2
    w = np.arange(1.0, n + 1.0)
    ipix = ang2pix_ring(nside, lon, lat)
    want = _counts(ipix, w, npix)
    assert len(np.unique(ipix)) > 64  # groups of neighbours across an edge all over the sphere, not a few crowded pixels

    maps = torch.zeros((2, npix), dtype=torch.float64, device="cuda")
    map_values(nside, lon, lat, maps, np.stack([np.ones(n), w]))
    assert torch.equal(maps, want), "map_values"
    del maps

    m = hx.HipHealpixMapper(nside, 2 * min(nside, 64), deconvolve=False)
    fields = {"CNT": hx.Positions(m, "lon", "lat", overdensity=False, nbar=1.0),
              "POS": hx.Positions(m, "lon", "lat", "w", overdensity=False, nbar=1.0)}
    sel = (np.arange(n) * 7 % 5 < 2).astype(np.int64)
    cols = {"lon": lon, "lat": lat, "w": w, "SEL": sel}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = hx.map_catalogs(fields, {0: hx.ArrayCatalog(cols, page_size=701)}, device="cuda")
        assert torch.equal(got["CNT", 0].tensor, want[0]) and torch.equal(got["POS", 0].tensor, want[1]), "map_catalogs"
        del got

        base = hx.ArrayCatalog(cols, page_size=701)
        got = hx.map_catalogs(fields, {k: base[f"SEL=={k}"] for k in (0, 1)}, device="cuda")
        for k in (0, 1):
            part = _counts(ipix[sel == k], w[sel == k], npix)
            assert torch.equal(got["CNT", k].tensor, part[0]) and torch.equal(got["POS", k].tensor, part[1]), f"view {k}"
        del got, part

        # FootprintFilter: the footprint of ang2pix_ring's own pixels keeps every row (the filter's pixel is one of them); footprints
        # holding the pixels whose rank among them has bit b set keep exactly the rows of those pixels, for every bit: the same pixel
        upix, rank = np.unique(ipix, return_inverse=True)
        dpix = torch.as_tensor(upix, device="cuda")
        keeps = [np.ones(n, dtype=bool)] + [(rank >> b) & 1 == 1 for b in range(int(upix.size - 1).bit_length())]
        for b, keep in enumerate(keeps):
            fp = torch.zeros(npix, dtype=torch.float64, device="cuda")
            fp[dpix[torch.as_tensor(np.unique(rank[keep]), device="cuda")]] = 1.0
            cat = hx.ArrayCatalog(cols, page_size=701)
            cat.add_filter(hx.FootprintFilter(fp, "lon", "lat"))
            got = hx.map_catalogs(fields, {0: cat}, device="cuda")
            part = _counts(ipix[keep], w[keep], npix)
            assert torch.equal(got["CNT", 0].tensor, part[0]) and torch.equal(got["POS", 0].tensor, part[1]), f"FootprintFilter, footprint {b}"
            del got, part, fp


def _frontier_lats():
    """Latitudes whose theta_d is 0, the smallest positive double step 2^-52, pi, and values in (pi, pi + 1e-5] up to either side of the
    bound; one to four ulp beyond +-90."""
    beyond = -90.0 - np.degrees(np.array([1e-12, 1e-9, 1e-7, 1e-6, 5e-6, 9.9e-6]))
    lat = -90.0 - np.degrees(1e-5)
    bound = pr.ulp_step(lat, np.arange(-600, 601, 40))  # theta_d moves by 2^-51 per 1.5 ulp of lat: both sides of pi + 1e-5
    return np.concatenate([pr.ulp_step(90.0, np.arange(-4, 5)), pr.ulp_step(-90.0, np.arange(-4, 5)), beyond, bound])


@pytest.mark.parametrize("nside", [3, 4096, 2**24])
def test_validity_frontier(nside):
    """Accepted iff lon is finite and 0 <= theta_d <= pi + 1e-5 (healpy's check_theta_valid, evaluated in numpy on theta_d).  An
    accepted point with theta_d <= pi gets an admissible pixel; one with theta_d in (pi, pi + 1e-5] a pixel of the last ring.  A
    rejected point raises ValueError and map_values leaves the maps as they were."""
    from heracles_amd.mapper import ang2pix_ring, map_values

    lat = _frontier_lats()
    lon = np.linspace(1.0, 359.0, lat.size)
    theta, tt = pr.front_end(lon, lat)
    valid = pr.theta_valid(theta)
    past = valid & (theta > np.pi)
    assert (theta == 0.0).any() and (theta == 2.0**-52).any() and (theta == np.pi).any() and (theta < 0).any()
    assert past.sum() >= 8 and (~valid & (theta > np.pi)).sum() >= 2 and theta[past].max() > np.pi + 0.99e-5
    npix = 12 * nside**2
    for lo, la, th, t, ok in zip(lon, lat, theta, tt, valid):
        one = (np.array([lo]), np.array([la]))
        if not ok:
            with pytest.raises(ValueError):
                ang2pix_ring(nside, *one)
            continue
        p = int(ang2pix_ring(nside, *one)[0])
        if th <= np.pi:
            assert p in pr.admissible(nside, th, t)[1], (lo, la, p)
        else:
            assert npix - 4 <= p < npix, f"theta_d - pi = {th - np.pi:.3e} (lon, lat) = ({lo!r}, {la!r}): pixel npix - {npix - p}"
    # a page with one rejected row raises as a whole, before anything is scattered
    ns = min(nside, 64)
    maps = np.full((2, 12 * ns**2), 7.0)
    for bad in np.flatnonzero(~valid)[[0, -1]]:
        rows = np.r_[np.flatnonzero(valid)[:5], bad]
        with pytest.raises(ValueError):
            ang2pix_ring(ns, lon[rows], lat[rows])
        with pytest.raises(ValueError):
            map_values(ns, lon[rows], lat[rows], maps, np.ones((2, rows.size)))
        assert (maps == 7.0).all()
    map_values(ns, lon[valid], lat[valid], maps, np.ones((2, int(valid.sum()))))
    assert maps.sum() == 7.0 * maps.size + 2 * valid.sum()
