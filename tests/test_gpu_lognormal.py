"""The lognormal mocks on the GPU against the numpy restatement (tests/lognormal_reference.py): the element-wise
pass between the correlation functions, the Gaussianised spectra, the repair of indefinite matrices of spectra, the map pass, and the
driver -- statistically, with a convergence-derived shear, and with the repair switched on."""

import numpy as np
import pytest

import lognormal_reference as lr
import synalm_reference as sr

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def hx():
    import heracles_amd

    heracles_amd.init()
    return heracles_amd


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- hx_lognormal_xi ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ncol", [1, 3, 70])
def test_lognormal_xi_against_numpy(hx, torch, ncol):
    from heracles_amd.lognormal import lognormal_xi

    rng = np.random.default_rng(ncol)
    worst = {}
    for nnodes in (1, 63, 64, 143):
        fac = 10.0 ** rng.uniform(-3, 3, ncol)
        arg = np.concatenate([rng.uniform(-0.95, 3.0, (ncol, nnodes - nnodes // 2)), rng.uniform(-1, 1, (ncol, nnodes // 2)) * 1e-9], axis=1)
        for inverse in (False, True):
            xi = arg if inverse else arg / fac[:, None]
            ref = lr.xi_inverse(xi, fac) if inverse else lr.xi_forward(xi, fac)
            for in_place in (False, True):
                dev = torch.from_numpy(xi.copy()).cuda()
                got = lognormal_xi(dev, fac, inverse=inverse, out=dev if in_place else None)
                assert (got is dev) == in_place
                if not in_place:
                    assert (bits(dev.cpu().numpy()) == bits(xi)).all()
                got = got.cpu().numpy()
                ulps = np.abs(got - ref) / np.spacing(np.abs(ref))
                worst[inverse] = max(worst.get(inverse, 0.0), float(ulps.max()))
                assert (ulps <= 2).all(), (nnodes, inverse, in_place, float(ulps.max()))
            host = lognormal_xi(xi.copy(), fac, inverse=inverse)  # host arrays in, host array out
            assert (np.abs(host - ref) <= 2 * np.spacing(np.abs(ref))).all()
    print(f"lognormal_xi ncol {ncol}: worst error {worst[False]:.2f} ulp (log1p), {worst[True]:.2f} ulp (expm1)")


def test_lognormal_xi_bad_argument_reports_first_and_writes_nothing(hx, torch):
    from heracles_amd.lognormal import lognormal_xi

    ncol, nnodes = 3, 16
    rng = np.random.default_rng(8)
    xi = rng.uniform(-0.5, 0.5, (ncol, nnodes))
    fac = np.array([2.0, 1.0, 4.0])
    xi[2, 5] = -0.25  # * 4 = -1
    xi[0, 9] = -0.75  # * 2 = -1.5
    buf = torch.full((ncol * nnodes + 16,), float("nan"), dtype=torch.float64, device="cuda")
    buf[8 : 8 + ncol * nnodes] = 7.0
    before = bits(buf.cpu().numpy()).copy()
    out = buf[8 : 8 + ncol * nnodes].view(ncol, nnodes)
    with pytest.raises(hx.HxError, match="column 0, node 9") as err:
        lognormal_xi(torch.from_numpy(xi).cuda(), fac, out=out)
    assert err.value.code == -1
    assert (bits(buf.cpu().numpy()) == before).all()
    src = torch.from_numpy(xi).cuda()
    with pytest.raises(hx.HxError, match="column 0, node 9"):
        lognormal_xi(src, fac, out=src)  # in place: the input survives
    assert (bits(src.cpu().numpy()) == bits(xi)).all()
    xi[0, 9] = np.nan
    with pytest.raises(hx.HxError, match="column 0, node 9"):
        lognormal_xi(xi, fac)
    lognormal_xi(xi, fac, inverse=True)  # the way back has no forbidden argument


# ---- lognormal_gaussian_cls ------------------------------------------------------------------------------------------------------------------

GAUSS_FIELDS = (("D", 0, 0), ("D", 1, 0), ("D", 2, 0), ("T", 0, 0), ("G", 0, 2))
GAUSS_SHIFTS = np.array([1.0, 0.05, 2.5, 0.0, 0.0, 0.0])


@pytest.fixture(scope="module")
def gauss_case():
    lmax = 40
    var = np.where(GAUSS_SHIFTS > 0, GAUSS_SHIFTS**2 * np.expm1([0.5, 0.3, 0.1, 0, 0, 0]), [0, 0, 0, 0.2, 0.3, 0.1])
    Cm = lr.smooth_spectra(6, lmax, 5, var)
    Cm[4:, :, :2] = 0.0
    Cm[:, 4:, :2] = 0.0
    return lmax, Cm, sr.matrix_to_cls(Cm, GAUSS_FIELDS)


@pytest.mark.parametrize("extra", [None, 7])
def test_gaussian_cls_against_long_double(hx, gauss_case, extra):
    lmax, Cm, cls = gauss_case
    nodes = None if extra is None else lmax + extra + 1
    shifts = {("D", 0): 1.0, ("D", 1): 0.05, ("D", 2): 2.5}
    got = hx.lognormal_gaussian_cls(cls, shifts, nodes=nodes)
    assert list(got) == list(cls)
    for key in cls:
        assert got[key].shape == cls[key].shape and got[key].dtype.metadata == cls[key].dtype.metadata
    G = sr.cls_to_matrix(got, GAUSS_FIELDS)
    x, w = hx.gauss_legendre(2 * lmax + 2 if nodes is None else nodes)
    ref, bound = lr.convert(Cm, GAUSS_SHIFTS, x, w)
    ln = np.ix_(GAUSS_SHIFTS > 0, GAUSS_SHIFTS > 0)
    err = np.abs((G - ref).astype(np.float64))[ln]
    print(f"gaussian cls (nodes {len(x)}): max error {err.max():.3e}, worst error / bound {(err / bound[ln]).max():.3f}, "
          f"sigma^2 = {[round(lr.sigma2(G[i, i]), 3) for i in range(3)]}")
    assert (err <= bound[ln]).all()
    lam = GAUSS_SHIFTS[:3]
    assert (G[:3, 3:] == Cm[:3, 3:] / lam[:, None, None]).all() and (G[3:, :3] == Cm[3:, :3] / lam[None, :, None]).all()
    assert (G[3:, 3:] == Cm[3:, 3:]).all()
    # a name alone shifts every bin of the field
    same = hx.lognormal_gaussian_cls({k: v for k, v in cls.items() if k[0] == k[1] == "D"}, {"D": 1.0}, nodes=nodes)
    assert same["D", "D", 0, 0].shape == (lmax + 1,)


def test_realised_cls_inverts_gaussian_cls_up_to_the_cut(hx, gauss_case):
    lmax, Cm, cls = gauss_case
    shifts = {("D", 0): 1.0, ("D", 1): 0.05, ("D", 2): 2.5}
    back = sr.cls_to_matrix(hx.lognormal_realised_cls(hx.lognormal_gaussian_cls(cls, shifts), shifts), GAUSS_FIELDS)
    x, w = hx.gauss_legendre(2 * lmax + 2)
    G, _ = lr.convert(Cm, GAUSS_SHIFTS, x, w)
    ref, bound = lr.convert(G.astype(np.float64), GAUSS_SHIFTS, x, w, inverse=True)
    # against the restatement of the same cut chain.  The way back starts from the GPU's own G, which differs from the restatement's
    # by the forward chain's error (within its bound, test above: below 1e-13 of the peak); carried through expm1 and the second
    # transform that stays below 1e-11 of each spectrum's peak, which is added to the bound of the way back
    err = np.abs((back - ref).astype(np.float64))
    scale = np.abs(Cm).max(axis=2, keepdims=True)
    print(f"realised cls: worst error / (bound + 1e-11 peak) = {float((err / (bound + 1e-11 * scale + 1e-300)).max()):.3f}")
    assert (err <= bound + 1e-11 * scale).all()
    assert np.abs(back - Cm).max() <= 1e-3 * np.abs(Cm).max()  # the cut itself: 1.5e-4 at sigma^2 = 0.5 (test_lognormal_host.py)


def test_gaussian_cls_names_the_pair_of_a_forbidden_correlation(hx):
    lmax = 6
    c = np.zeros(lmax + 1)
    c[1] = 4 * np.pi
    with pytest.raises(ValueError, match=r"\('D', 0\) x \('D', 0\).*node 0 of 14"):
        hx.lognormal_gaussian_cls({("D", "D", 0, 0): c}, {"D": 0.5})


# ---- hx_cl_nearest_psd -------------------------------------------------------------------------------------------------------------------

PSD_LMAX = 70


def psd_case(n):
    """(C (n, n, nl), kinds): per l one of  a: strictly positive definite;  b: PSD of rank n - 1;  c: one to three eigenvalues of the
    scaled matrix at -1e-3 .. -1e-9 of the largest;  then  +d: component scales 1e4, 1e-4 alternating;  +e: a zero row and column.
    n = 9: components 7, 8 are a spin-2 field's and vanish below l = 2 (f)."""
    rng = np.random.default_rng(100 + n)
    nl = PSD_LMAX + 1
    Cm = np.zeros((n, n, nl))
    kinds = []
    for l in range(nl):
        kind = "abcacac"[l % 7]
        if n == 1 and kind in "bc":
            kind = "a"
        if kind == "a":
            B = rng.standard_normal((n, 2 * n + 2))
            M = B @ B.T
        elif kind == "b":
            B = rng.standard_normal((n, n - 1))
            M = B @ B.T
        else:
            B = rng.standard_normal((n, 2 * n + 2))
            M = B @ B.T
            d = np.sqrt(np.diagonal(M))
            lamb, V = np.linalg.eigh(M / np.outer(d, d))
            k = min(3 if l % 7 == 6 else 1 + l % 3, n - 1)  # (with a zero row to come: enough of them that one survives it)
            lamb[:k] = -lamb[-1] * 10.0 ** -rng.uniform(3, 9, k)
            M = (V * lamb) @ V.T * np.outer(d, d)
            M = 0.5 * (M + M.T)
            assert (np.diagonal(M) > 0).all()
        extra = ""
        if l % 7 in (3, 4):
            s = np.where(np.arange(n) % 2 == 0, 1e4, 1e-4)
            M = M * np.outer(s, s)
            extra += "d"
        if l % 7 in (5, 6) and n > 1:
            j = (l // 7) % n
            M[j, :] = M[:, j] = 0.0
            extra += "e"
        if n == 9 and l < 2:
            M[7:, :] = M[:, 7:] = 0.0
            extra += "f"
        Cm[:, :, l] = M / (l + 1.0) ** 2
        kinds.append(kind + extra)
    return Cm, kinds


@pytest.mark.parametrize("n", [1, 2, 3, 9, 33, 64])
def test_nearest_psd_against_eigh(hx, torch, n):
    from heracles_amd.mocks import cl_cholesky

    Cm, kinds = psd_case(n)
    packed = sr.pack(Cm)
    want, want_change, repaired = lr.nearest_psd(Cm)
    # the case is what its labels say: (a) needs no repair, (b) and (c) do -- a zero row on top may leave what is left definite
    assert not any(r for r, k in zip(repaired, kinds) if k[0] == "a")
    assert all(r for r, k in zip(repaired, kinds) if k[0] != "a" and len(k) == 1 or k[1:] == "d" and k[0] != "a")
    assert n < 3 or any(r for r, k in zip(repaired, kinds) if "e" in k)
    got, change = hx.nearest_psd_cls(packed, return_change=True)
    assert got.shape == packed.shape and change.shape == (PSD_LMAX + 1,)
    keep = ~repaired
    assert (bits(got[:, keep]) == bits(packed[:, keep])).all() and (change[keep] == 0).all()  # valid input is never perturbed
    full = sr.unpack(got, n)
    scale = np.sqrt(np.einsum("iil,jjl->ijl", Cm, Cm))
    err = np.abs(full - want)
    live = scale > 0
    print(f"nearest_psd N = {n}: worst |gpu - eigh| / sqrt(C_ii C_jj) = {(err[live] / scale[live]).max():.3e}, largest change {change.max():.3e}, "
          f"worst |change - ref| = {np.abs(change - want_change).max():.3e}")
    assert (err <= 1e-12 * scale).all()  # (exactly zero where a diagonal is zero)
    assert (np.abs(change - want_change) <= 1e-12).all()
    # every output passes the factor of 4.15 with no zeroed column among the components that have power
    L = sr.unpack(cl_cholesky(got, n), n, lower=True)
    diag = np.einsum("iil->il", L)
    power = np.einsum("iil->il", Cm) > 0
    assert (diag[power] > 0).all() and (diag[~power] == 0).all()
    alms = hx.synalm_components(got, n, seed=5)
    assert np.isfinite(alms).all()
    # the same bits in a second run, from a device tensor, and on a sub-range of l
    again = hx.nearest_psd_cls(torch.from_numpy(packed).cuda()).cpu().numpy()
    assert (bits(again) == bits(got)).all()
    part, part_change = hx.nearest_psd_cls(np.ascontiguousarray(packed[:, 10:37]), return_change=True)
    assert (bits(part) == bits(got[:, 10:37])).all() and (bits(part_change) == bits(change[10:37])).all()


def test_nearest_psd_dict_form(hx):
    Cm, lam = lr.indefinite_targets()
    fields = (("D", 0, 0), ("D", 1, 0), ("D", 2, 0))
    x, w = hx.gauss_legendre(2 * 16 + 2)
    G = lr.convert(Cm, lam, x, w)[0].astype(np.float64)
    cls = sr.matrix_to_cls(G, fields)
    out, change = hx.nearest_psd_cls(cls, return_change=True)
    assert list(out) == list(cls) and (change > 0).all()
    want, want_change, _ = lr.nearest_psd(G)
    assert np.abs(sr.cls_to_matrix(out, fields) - want).max() <= 1e-12 * np.abs(G).max()
    assert out["D", "D", 0, 1].dtype.metadata == cls["D", "D", 0, 1].dtype.metadata


def test_nearest_psd_rejects_bad_input_and_writes_nothing(hx):
    from heracles_amd import _lib

    n = 3
    Cm, _ = psd_case(n)
    Cm[1, 1, 7] = -1.0
    Cm[0, 2, 3] = Cm[2, 0, 3] = np.nan
    packed = sr.pack(Cm)
    with pytest.raises(hx.HxError, match="l = 3") as err:
        hx.nearest_psd_cls(packed)
    assert err.value.code == _lib.HX_ERR_ARG
    lib = _lib.load()
    out, change = np.full(packed.shape, 3.0), np.full(PSD_LMAX + 1, 4.0)
    assert lib.hx_cl_nearest_psd(n, PSD_LMAX, _lib.ptr(packed), -1.0, _lib.ptr(out), _lib.ptr(change)) == _lib.HX_ERR_ARG
    assert b"l = 3" in lib.hx_last_error() and (out == 3.0).all() and (change == 4.0).all()
    packed[sr.pair_list(n).index((0, 2)), 3] = 0.5
    with pytest.raises(hx.HxError, match=r"negative auto-spectrum at l = 7 \(component 1\)"):
        hx.nearest_psd_cls(packed)
    for bad in (0, 65):
        assert lib.hx_cl_nearest_psd(bad, 4, _lib.ptr(packed), -1.0, _lib.ptr(out), _lib.ptr(change)) == _lib.HX_ERR_ARG
    assert (out == 3.0).all()


# ---- hx_lognormal_maps -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrow", [1, 5])
def test_lognormal_maps_against_numpy(hx, torch, nrow):
    from heracles_amd.lognormal import lognormal_transform_maps

    rng = np.random.default_rng(nrow)
    worst = 0.0
    for npix in (1, 12, 49, 1027, 12 * 16**2):
        s2 = rng.uniform(0.0, 1.0, nrow)
        lam = 10.0 ** rng.uniform(-2, 1, nrow)
        g = rng.standard_normal((nrow, npix)) * 2.0
        g.flat[0] = -800.0  # expm1 = -1 exactly
        ref = lr.maps(g, s2, lam)
        tol = 4 * np.spacing(lam[:, None] * np.maximum(1.0, np.exp(g - 0.5 * s2[:, None])))
        # offsets of the two buffers in doubles: aligned, both off by one (a head element per row), different (no vectors)
        for off_in, off_out in ((0, None), (0, 0), (1, 1), (1, 0)):
            src = torch.full((nrow * npix + 4,), float("nan"), dtype=torch.float64, device="cuda")
            a = src[off_in : off_in + nrow * npix].view(nrow, npix)
            a.copy_(torch.from_numpy(g))
            if off_out is None:
                got = lognormal_transform_maps(a, s2, lam)
                assert got is a
                whole = src
            else:
                dst = torch.full((nrow * npix + 4,), float("nan"), dtype=torch.float64, device="cuda")
                got = lognormal_transform_maps(a, s2, lam, out=dst[off_out : off_out + nrow * npix].view(nrow, npix))
                assert (bits(a.cpu().numpy()) == bits(g)).all()
                whole, off_in = dst, off_out
            whole = whole.cpu().numpy()
            assert np.isnan(whole[:off_in]).all() and np.isnan(whole[off_in + nrow * npix :]).all()  # the sentinels keep their bits
            got = got.cpu().numpy()
            err = np.abs(got - ref)
            worst = max(worst, float((err / (tol / 4)).max()))
            assert (err <= tol).all(), (npix, off_in, off_out)
            assert got.flat[0] == -lam[0] and (got >= -lam[:, None]).all()
        host = lognormal_transform_maps(g.copy() if nrow > 1 else g[0].copy(), s2, lam)
        assert (np.abs(host.reshape(nrow, npix) - ref) <= tol).all()
    print(f"lognormal_maps nrow {nrow}: worst error {worst:.2f} ulp of lambda max(1, e^x)")


def test_lognormal_maps_partial_overlap_is_refused(hx, torch):
    from heracles_amd import _lib
    from heracles_amd.lognormal import lognormal_transform_maps

    buf = torch.arange(40, dtype=torch.float64, device="cuda") / 40
    before = bits(buf.cpu().numpy()).copy()
    with pytest.raises(hx.HxError, match="overlaps") as err:
        lognormal_transform_maps(buf[0:24].view(2, 12), 0.1, 1.0, out=buf[6:30].view(2, 12))
    assert err.value.code == _lib.HX_ERR_ARG and (bits(buf.cpu().numpy()) == before).all()
    host = np.arange(40.0) / 40
    with pytest.raises(hx.HxError, match="overlaps"):
        lognormal_transform_maps(host[0:24], 0.1, 1.0, out=host[1:25])
    assert (host == np.arange(40.0) / 40).all()
    with pytest.raises(hx.HxError, match="shift"):
        lognormal_transform_maps(host[0:24], 0.1, 0.0)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------

STAT_FIELDS = (("P", 0, 0), ("P", 1, 0), ("G", 0, 2))


def test_driver_statistics(hx, torch):
    """n realisations of one seed at nside 32, lmax 32: the spectra of the maps (map2alm with niter = 3, alm2cl_pairs, 2 <= l <= 16)
    against lognormal_realised_cls of the factored spectra.  The conditions are those of DESIGN.md 4.19: max |z| <= 6, 0.8 <= rms z <= 1.2.
    The same experiment on the host with the oracle's transforms and the numpy restatement (the same Philox draws) gave max |z| = 2.64,
    rms z = 0.976 at n = 200."""
    nside, lmax, n = lr.STAT_NSIDE, lr.STAT_LMAX, lr.STAT_N
    mapper = hx.HipHealpixMapper(nside, lmax, deconvolve=False)
    fields = {"P": hx.Positions(mapper, "ra", "dec"), "G": hx.Shears(mapper, "ra", "dec", "g1", "g2")}
    cls = sr.matrix_to_cls(lr.statistical_targets(), STAT_FIELDS)
    shifts = {("P", 0): 1.0, ("P", 1): 0.3}
    gcls = hx.lognormal_gaussian_cls(cls, shifts, lmax=lmax)
    expected = sr.cls_to_matrix(hx.lognormal_realised_cls(gcls, shifts), STAT_FIELDS)
    pairs = sr.pair_list(4)
    plan = hx.get_plan(nside, lmax)
    est = np.empty((n, len(pairs), lmax + 1))
    for r in range(n):
        maps = hx.lognormal_maps(fields, cls, shifts, seed=lr.STAT_SEED, realisation=r, device="cuda")
        assert list(maps) == [("P", 0), ("P", 1), ("G", 0)]
        a0 = plan.map2alm(torch.stack([maps["P", 0].tensor, maps["P", 1].tensor]), 0, niter=3)
        a2 = plan.map2alm(maps["G", 0].tensor, 2, niter=3)
        est[r] = hx.alm2cl_pairs([a0[0], a0[1], a2[0], a2[1]], pairs, lmax)
        if r == 0:
            first = {k: v.tensor.cpu().numpy() for k, v in maps.items()}
            assert first["P", 0].min() >= -1.0 and first["P", 1].min() >= -0.3
            assert maps["P", 0].dtype.metadata["spin"] == 0 and maps["G", 0].dtype.metadata["nside"] == nside
    want = np.stack([expected[a, b] for a, b in pairs])
    z, zmax, zrms = lr.z_scores(est[:, :, lr.STAT_ELLS], want[:, lr.STAT_ELLS])
    print(f"driver statistics, n = {n}: max |z| = {zmax:.2f}, rms z = {zrms:.3f}")
    assert zmax <= 6 and 0.8 <= zrms <= 1.2
    again = hx.lognormal_maps(fields, cls, shifts, seed=lr.STAT_SEED, realisation=0, device="cuda")
    for k, v in again.items():
        assert (bits(v.tensor.cpu().numpy()) == bits(first[k])).all()
    host = hx.lognormal_maps(fields, cls, shifts, seed=lr.STAT_SEED, realisation=0)  # numpy maps: the same mock
    assert np.abs(host["P", 1] - first["P", 1]).max() <= 1e-12 and host["P", 1].dtype.metadata["spin"] == 0


def test_driver_convergence_gives_the_shear_of_the_map(hx):
    """E of the derived shear maps is f_l times the alm of the convergence map, B is zero, to the round-trip level 1e-10.  At nside 16
    and lmax 24 the transform reaches that level with computed pixel weights only (unit weights and niter = 3 leave 7e-7), so the
    mapper uses pixel_weights="compute"."""
    from heracles_amd.lognormal import shear_factor

    nside, lmax = 16, 24
    mapper = hx.HipHealpixMapper(nside, lmax, deconvolve=False, pixel_weights="compute")
    fields = {"K": hx.ScalarField(mapper, "ra", "dec", "kappa"), "G": hx.Shears(mapper, "ra", "dec", "g1", "g2")}
    l = np.arange(lmax + 1)
    c = 0.1 * 4 * np.pi / ((l + 3.0) ** 2.2)
    cls = {("K", "K", 0, 0): c, ("K", "K", 1, 1): 0.5 * c, ("K", "K", 0, 1): 0.3 * c}
    maps = hx.lognormal_maps(fields, cls, {"K": 1.0}, seed=3, convergence={"G": "K"})
    assert list(maps) == [("K", 0), ("K", 1), ("G", 0), ("G", 1)]
    assert maps["G", 1].shape == (2, 12 * nside**2) and maps["G", 1].dtype.metadata["spin"] == 2
    alms = hx.transform(fields, maps)
    ll, _ = sr.lm_index(lmax)
    for i in (0, 1):
        want = shear_factor(lmax)[ll] * alms["K", i]
        top = np.abs(want).max()
        e, b = np.abs(alms["G", i][0] - want).max() / top, np.abs(alms["G", i][1]).max() / top
        print(f"convergence bin {i}: |E - f kappa| / max = {e:.2e}, |B| / max = {b:.2e}")
        assert e <= 1e-10 and b <= 1e-10
    # a positive peak of kappa has tangential shear around it: Q cos 2 psi + U sin 2 psi < 0, psi from south through east
    from oracle import hxoracle as ho

    th, ph = ho.pix2ang(nside)
    k = maps["K", 0]
    p = int(np.argmax(np.where(np.abs(th - np.pi / 2) < 0.6, k, -np.inf)))
    u, v = th - th[p], np.angle(np.exp(1j * (ph - ph[p]))) * np.sin(th[p])
    ring = (u * u + v * v > 0.05**2) & (u * u + v * v < 0.13**2)
    psi = np.arctan2(v[ring], u[ring])
    q, uu = maps["G", 0][0][ring], maps["G", 0][1][ring]
    assert np.mean(-(q * np.cos(2 * psi) + uu * np.sin(2 * psi))) > 0


def test_driver_regularize(hx):
    """Three fields with target correlations 0.99, 0.99, 0.90: the Gaussianised matrices have an eigenvalue of -0.02 (scaled) at every
    l.  Without repair the driver fails as synalm does and says how to go on; with it, it runs."""
    from heracles_amd import _lib

    Cm, lam = lr.indefinite_targets()
    cls = sr.matrix_to_cls(Cm, (("D", 0, 0), ("D", 1, 0), ("D", 2, 0)))
    mapper = hx.HipHealpixMapper(8, 16, deconvolve=False)
    fields = {"D": hx.Positions(mapper, "ra", "dec")}
    shifts = {("D", i): lam[i] for i in range(3)}
    with pytest.raises(hx.HxError, match='not positive semi-definite at l = 0.*regularize="clip"') as err:
        hx.lognormal_maps(fields, cls, shifts, seed=1)
    assert err.value.code == _lib.HX_ERR_ARG
    maps = hx.lognormal_maps(fields, cls, shifts, seed=1, regularize="clip")
    for i in range(3):
        assert np.isfinite(maps["D", i]).all() and maps["D", i].min() >= -lam[i] and maps["D", i].std() > 0
