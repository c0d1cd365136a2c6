"""The numpy restatement of the coupled Gaussian covariance (tests/gauss_cov_reference.py) pinned on its own, and the pure-Python
request list of heracles_amd.gausscov.  No GPU.

The Monte Carlo check is the one the formula was validated with: nside 16, two spin-0 fields with white spectra [[1, 0.7], [0.7, 2]]
up to lmax 32, two different smooth positive masks of band limit 3, pseudo-Cl to L = 24 with niter = 3, data vector (aa, ab, bb), 600
realisations with a fixed seed, entries with l >= 4.  z_ij = (sample - analytic) / sigma_ij, sigma_ij^2 = (C_ii C_jj + C_ij^2) / (n - 1);
the conditions are max |z| <= 6 and 0.8 <= rms z <= 1.2."""

import itertools

import numpy as np
import pytest

import gauss_cov_reference as gr
import heracles_amd as hx
from heracles_amd.gausscov import covariance_requests, table_key


class _F:
    def __init__(self, spin, mask):
        self.spin, self.mask = spin, mask


def _white_cls(L):
    one = np.ones(L + 1)
    (caa, cab), (_, cbb) = gr.MC["spectra"]
    return {("A", "A", 1, 1): hx.Result(caa * one, spin=(0, 0)), ("A", "B", 1, 1): hx.Result(cab * one, spin=(0, 0)),
            ("B", "B", 1, 1): hx.Result(cbb * one, spin=(0, 0))}


def test_full_sky_is_gaussian_covariance_over_2l_plus_1(oracle):
    L = 12
    rng = np.random.default_rng(3)
    cls = {}
    for (a, i), (b, j) in itertools.combinations_with_replacement([("P", 1), ("G", 1)], 2):
        da, db = (1 if a == "P" else 2), (1 if b == "P" else 2)
        arr = rng.standard_normal((da, db, L + 1))
        if (a, i) == (b, j):
            arr = arr + arr.transpose(1, 0, 2)
        shape = tuple(d for d, n in ((da, a), (db, b)) if n != "P") + (L + 1,)
        spin = (0 if a == "P" else 2, 0 if b == "P" else 2)
        cls[a, b, i, j] = hx.Result(arr.reshape(shape), spin=spin)
    hx.update_metadata(cls["P", "P", 1, 1].array, bias=0.25)
    fields = {"P": _F(0, "V"), "G": _F(2, "W")}
    full = np.zeros(2 * L + 1)
    full[0] = 4 * np.pi
    xi = gr.xi_table(oracle, full, L)
    assert np.abs(xi - np.diag(1.0 / (2 * np.arange(L + 1) + 1))).max() <= 1e-14
    cov, _ = gr.covariance(oracle, cls, lambda *k: full, fields)
    want = hx.flatten(hx.gaussian_covariance(cls), order=list(cls))
    nunits = cov.shape[0] // (L + 1)
    want = want / np.tile(2 * np.arange(L + 1) + 1, nunits)[None, :]
    assert np.abs(cov - want).max() <= 1e-13 * np.abs(want).max()


def test_reference_is_symmetric(oracle):
    L = 10
    rng = np.random.default_rng(4)
    cls = _white_cls(L)
    for res in cls.values():
        res.array[:] *= 1 + 0.3 * rng.standard_normal(L + 1)
    fields = {"A": _F(0, "VA"), "B": _F(0, "VB")}
    spectra = {}

    def mask_cls(*k):
        key = table_key(((k[0], k[1]), (k[2], k[3])))
        if key not in spectra:
            spectra[key] = rng.uniform(0.5, 1.5, 2 * L + 1) / (1 + np.arange(2 * L + 1)) ** 2
        return spectra[key]

    plan = hx.BinPlan(np.arange(L + 1), np.array([2, 3, 6, L + 1]), "2l+1")
    for p in (None, plan):
        cov, A = gr.covariance(oracle, cls, mask_cls, fields, p)
        assert np.abs(cov - cov.T).max() <= 64 * 2.0**-53 * A.max()
        assert np.all(A >= np.abs(cov) * (1 - 1e-12))


def test_reference_passes_the_monte_carlo_check(oracle):
    c = gr.MC
    nside, lf, L, n = c["nside"], c["lmax_field"], c["L"], c["nreal"]
    ma, mb = gr.smooth_masks(oracle, nside, 2, c["mask_lmax"], c["seed"])
    assert ma.min() > 0 and mb.min() > 0 and np.abs(ma - mb).max() > 0.05
    rng = np.random.default_rng(c["seed"] + 1)
    samples = np.empty((n, 3 * (L + 1)))
    masks = np.stack([ma, mb])
    for r in range(n):
        maps = oracle.alm2map(gr.white_alms(rng, lf, c["spectra"]), nside, lf) * masks
        alm = oracle.map2alm(maps, nside, L, niter=c["niter"])
        samples[r] = np.concatenate([oracle.alm2cl(alm[0]), oracle.alm2cl(alm[0], alm[1]), oracle.alm2cl(alm[1])])
    # the spectra of the mask products, band limit 6: taken to 12, zero beyond
    mk = {("VA", 1): ma, ("VB", 1): mb}
    cache = {}

    def mask_cls(k1, k2, k3, k4):
        key = table_key(((k1, k2), (k3, k4)))
        if key not in cache:
            prod = np.stack([mk[k1] * mk[k2], mk[k3] * mk[k4]])
            alm = oracle.map2alm(prod, nside, 12, niter=c["niter"])
            cache[key] = oracle.alm2cl(alm[0], alm[1])
        return cache[key]

    fields = {"A": _F(0, "VA"), "B": _F(0, "VB")}
    cov, _ = gr.covariance(oracle, _white_cls(L), mask_cls, fields)
    keep = np.flatnonzero(np.tile(np.arange(L + 1), 3) >= c["lmin"])
    zmax, zrms, diag = gr.z_statistic(samples, cov, keep)
    print(f"Monte Carlo, oracle, n = {n}: max |z| = {zmax:.2f}, rms z = {zrms:.3f}, mean diagonal ratio {diag:.4f}")
    assert zmax <= 6, zmax
    assert 0.8 <= zrms <= 1.2, zrms


# ---- covariance_requests ------------------------------------------------------------------------------------------------------------
def _cls_2x2(L=5):
    units = [("P", 1), ("P", 2), ("G", 1), ("G", 2)]
    cls = {}
    for (a, i), (b, j) in itertools.combinations_with_replacement(units, 2):
        shape = tuple(2 for n in (a, b) if n == "G") + (L + 1,)
        cls[a, b, i, j] = hx.Result(np.zeros(shape), spin=(0 if a == "P" else 2, 0 if b == "P" else 2))
    return cls


def test_requests_every_block_has_two_terms():
    cls = _cls_2x2()
    req = covariance_requests(cls, {"P": _F(0, "V"), "G": _F(2, "W")})
    assert req.nl == 6
    assert len(req.units) == 3 * 1 + 4 * 2 + 3 * 4 and req.layout.n == len(req.units) * req.nl
    # the units are the layout's blocks, dof-major
    for u, (key, x, y) in enumerate(req.units):
        ndof = req.layout.size[key] // req.nl
        assert req.layout.offset[key] <= u * req.nl < req.layout.offset[key] + ndof * req.nl
    terms = {}
    for t, blocks in req.tables.items():
        assert t == table_key(t)
        for u1, u2, s in blocks:
            assert u1 <= u2
            assert all(0 <= v < len(req.spectra) for v in s[:2])
            terms[u1, u2] = terms.get((u1, u2), 0) + (2 if s[2] >= 0 else 1)
            if s[2] < 0:
                assert s[3] < 0
    nu = len(req.units)
    assert set(terms) == set(itertools.combinations_with_replacement(range(nu), 2))
    assert set(terms.values()) == {2}
    assert list(req.tables) == sorted(req.tables)


def test_requests_terms_and_spectra_follow_the_formula():
    cls = _cls_2x2()
    fields = {"P": _F(0, "V"), "G": _F(2, "W")}
    req = covariance_requests(cls, fields)
    comps = []
    for key, x, y in req.units:
        a, b, i, j = key
        comps.append(((a, i, x), (b, j, y)))
    mask = lambda p: (fields[p[0]].mask, p[1])  # noqa: E731
    seen = {}
    for t, blocks in req.tables.items():
        for u1, u2, s in blocks:
            seen.setdefault((u1, u2), []).extend((t, tuple(sorted(req.spectra[v] for v in s[2 * k:2 * k + 2]))) for k in range(2) if s[2 * k] >= 0)
    for (u1, u2), got in seen.items():
        (a, b), (c, d) = comps[u1], comps[u2]
        want = [(table_key(((mask(a), mask(c)), (mask(b), mask(d)))), tuple(sorted((tuple(sorted((a, c))), tuple(sorted((b, d))))))),
                (table_key(((mask(a), mask(d)), (mask(b), mask(c)))), tuple(sorted((tuple(sorted((a, d))), tuple(sorted((b, c)))))))]
        assert sorted(got) == sorted(want), (u1, u2)


def test_table_keys_are_invariant_under_the_swaps():
    a, b, c, d = ("V", 1), ("W", 2), ("V", 2), ("W", 1)
    canon = table_key(((a, b), (c, d)))
    for p, q in (((a, b), (c, d)), ((c, d), (a, b))):
        for pp in (p, p[::-1]):
            for qq in (q, q[::-1]):
                assert table_key((pp, qq)) == canon
                assert table_key(((a, b), (c, d)), {(pp, qq): 7}) == 7
    assert table_key(((a, c), (b, d))) != canon
    with pytest.raises(KeyError, match="W"):
        table_key(((a, b), (c, d)), {})


def test_requests_merge_terms_when_masks_coincide():
    cls = _cls_2x2()
    shared = covariance_requests(cls, {"P": _F(0, "V"), "G": _F(2, "V")})
    apart = covariance_requests(cls, {"P": _F(0, "V"), "G": _F(2, "W")})
    nblocks = len(shared.units) * (len(shared.units) + 1) // 2
    # one mask per bin: tables are keyed by bins alone, and a block's terms share a table exactly when the table keys coincide
    merged = sum(1 for blocks in shared.tables.values() for _, _, s in blocks if s[2] >= 0)
    single = sum(1 for blocks in shared.tables.values() for _, _, s in blocks if s[2] < 0)
    assert merged + single // 2 == nblocks and merged > 0
    assert len(shared.tables) < len(apart.tables)
    for t, blocks in shared.tables.items():
        assert len({(u1, u2) for u1, u2, _ in blocks}) == len(blocks)  # one item per block and table
    # the auto block of one field and bin: both terms read (m m, m m)
    u = next(k for k, (key, x, y) in enumerate(shared.units) if key == ("P", "P", 1, 1))
    t = table_key(((("V", 1), ("V", 1)), (("V", 1), ("V", 1))))
    assert any(u1 == u and u2 == u and s[2] >= 0 for u1, u2, s in shared.tables[t])


def test_requests_order_is_stable():
    fields = {"P": _F(0, "V"), "G": _F(2, "W")}
    one = covariance_requests(_cls_2x2(), fields)
    two = covariance_requests(_cls_2x2(), dict(reversed(list(fields.items()))))
    assert list(one.tables) == list(two.tables)
    assert one.tables == two.tables and one.spectra == two.spectra and one.units == two.units


def test_item_record_is_the_c_struct():
    import ctypes

    from heracles_amd.gausscov import ITEM, pack_items

    assert ITEM.itemsize == ctypes.sizeof(hx._lib.CovItem) == 32
    assert [ITEM.fields[n][1] for n in ("row", "col", "s")] == [hx._lib.CovItem.row.offset, hx._lib.CovItem.col.offset, hx._lib.CovItem.s.offset]
    arr = pack_items([(1, 2, (3, 4, -1, -1)), (5, 6, (7, 8, 9, 10))], scale=3)
    assert arr["row"].tolist() == [3, 15] and arr["col"].tolist() == [6, 18] and arr["s"].tolist() == [[3, 4, -1, -1], [7, 8, 9, 10]]
    assert pack_items(arr) is arr and len(pack_items([])) == 0


def test_requests_errors():
    cls = _cls_2x2()
    with pytest.raises(ValueError, match="no mask"):
        covariance_requests(cls, {"P": _F(0, "V"), "G": _F(2, None)})
    cls["P", "P", 1, 1] = hx.Result(np.zeros(4), spin=(0, 0))
    with pytest.raises(ValueError, match="multipoles"):
        covariance_requests(cls, {"P": _F(0, "V"), "G": _F(2, "W")})
