"""Template deprojection on the host: the numpy restatement (tests/deprojection_reference.py) pinned on its own with the CPU oracle,
the host-side parts of heracles_amd.deprojection, and the Monte Carlo check of the deprojection bias.  No GPU.

Bounds.  With u = 2^-53, k templates, kappa = cond of the unit-diagonal Gram matrix and alpha = G^+ r formed in double from a Gram
matrix that is exact to a few u: the relative error of alpha in the norm of G is at most c k u kappa for a modest constant c (eigh is
backward stable), so |f_i^T d_c| = |sum_j G_ij dalpha_j| <= sqrt(G_ii) |F dalpha| <= c k u kappa sqrt(G_ii d^T d), and a map that
should not change moves by at most c k u kappa |d| in the 2-norm.  c = 64 covers the constants of eigh and of the products.

The Monte Carlo check: nside 16, lmax 24, 600 Gaussian realisations of one spin-0 and one spin-2 field with a non-zero
cross-spectrum, two different smooth masks, 8 band-limited templates (l <= 6) per field, pseudo-Cl with niter = 3.  Per realisation
Delta_l = PCL(cleaned) - PCL(uncleaned) for (PP, PE, PB, EE, EB, BE, BB); z_l = (mean Delta_l - bias_l) / (std Delta_l / sqrt(n)); the
conditions are max |z| <= 6 and 0.8 <= rms z <= 1.2 over l >= 2.  With the bias set to zero the same statistic must violate
max |z| <= 6.  Measured on the oracle: max |z| = 2.70, rms z = 0.990; with the bias set to zero max |z| = 23.5, rms z = 5.63."""

import math

import numpy as np
import pytest

import deprojection_reference as dr
import heracles_amd as hx
from heracles_amd import deprojection as dp

U = 2.0**-53
C_EIGH = 64


class _F:
    def __init__(self, spin, mask):
        self.spin, self.mask = spin, mask


def _case(oracle, nside, ncomp, k, seed, nmap=1):
    rng = np.random.default_rng(seed)
    spin = 0 if ncomp == 1 else 2
    t = dr._band_limited(oracle, rng, nside, 4, k, spin) + 0.05 * rng.standard_normal((k, ncomp, 12 * nside**2))
    v = 0.5 + 0.5 * rng.random(12 * nside**2)
    d = v * rng.standard_normal((nmap, ncomp, 12 * nside**2))
    return d, t, v


def test_long_double_sums_agree_with_fsum(oracle):
    d, t, v = _case(oracle, 8, 2, 3, 1)
    G, A = dr.gram(t, d, v)
    f = (v * t).reshape(3, -1)  # (the double products; fsum of their exact pair products differs from the long-double rule by the mask rounding)
    X = np.concatenate([f, d.reshape(1, -1)])
    for i, j in ((0, 0), (0, 2), (1, 3), (3, 3)):
        exact = math.fsum((X[i].astype(np.longdouble) * X[j].astype(np.longdouble)).astype(float))
        assert abs(G[i, j] - exact) <= 4 * U * A[i, j], (i, j)
    assert np.array_equal(G, G.T) and np.all(A >= np.abs(G))


@pytest.mark.parametrize("nside,ncomp", [(8, 1), (8, 2), (16, 1), (16, 2)])
def test_projector(oracle, nside, ncomp):
    d, t, v = _case(oracle, nside, ncomp, 6, 10 + nside + ncomp)
    ref = dr.deproject(d, t, v)
    assert ref["rank"] == 6 and ref["dropped"] == ()
    k, kappa = 6, ref["cond"]
    dc = ref["cleaned"]
    Gc, _ = dr.gram(t, dc, v)
    dd = float((d.astype(np.longdouble) ** 2).sum())
    bound = C_EIGH * k * U * kappa * np.sqrt(np.diag(ref["gram"]) * dd)
    assert np.all(np.abs(Gc[:k, k]) <= bound), np.abs(Gc[:k, k]) / bound
    again = dr.deproject(dc, t, v)["cleaned"]
    assert np.linalg.norm(again - dc) <= C_EIGH * k * U * kappa * np.sqrt(dd)
    # what is removed: alpha^T r = d^T d - d_c^T d_c
    assert abs(float(ref["alpha"][0] @ ref["r"][:, 0]) - (dd - Gc[k, k])) <= C_EIGH * k * U * kappa * dd


@pytest.mark.parametrize("nside,ncomp", [(8, 1), (16, 2)])
def test_contamination_is_removed(oracle, nside, ncomp):
    d, t, v = _case(oracle, nside, ncomp, 5, 30 + nside)
    beta = np.array([3.0, -1.5, 0.25, 10.0, -7.0])
    dirty = d + v * np.einsum("i,icp->cp", beta, t)[None]
    a, b = dr.deproject(d, t, v), dr.deproject(dirty, t, v)
    scale = np.sqrt(float((dirty.astype(np.longdouble) ** 2).sum()))
    assert np.linalg.norm(a["cleaned"] - b["cleaned"]) <= C_EIGH * 5 * U * a["cond"] * scale
    assert np.abs(b["alpha"] - a["alpha"] - beta).max() <= 1e-9


def test_duplicate_and_zero_templates_are_dropped(oracle):
    d, t, v = _case(oracle, 8, 1, 4, 77)
    more = np.concatenate([t, t[1:2], np.zeros_like(t[:1])])  # template 4 repeats template 1, template 5 is all zero
    a, b = dr.deproject(d, t, v), dr.deproject(d, more, v)
    assert (a["rank"], a["dropped"]) == (4, ()) and (b["rank"], b["dropped"]) == (4, (5,))
    scale = np.sqrt(float((d.astype(np.longdouble) ** 2).sum()))
    assert np.linalg.norm(a["cleaned"] - b["cleaned"]) <= C_EIGH * 6 * U * a["cond"] * scale
    # the package's host rule is the reference's
    inv, rank, dropped = dp.scaled_pinv(b["gram"])
    assert (rank, dropped) == (4, (5,))
    assert np.abs(inv - b["inverse"]).max() <= 1e-12 * np.abs(b["inverse"]).max()
    inv0, rank0, dropped0 = dp.scaled_pinv(np.zeros((2, 2)))
    assert rank0 == 0 and dropped0 == (0, 1) and not inv0.any()


def test_debias_cls_subtracts_a_block_shaped_result():
    rng = np.random.default_rng(5)
    cls = {("P", "G", 1, 1): rng.standard_normal((2, 9)), ("P", "P", 1, 1): rng.standard_normal(9)}
    bias = {("P", "G", 1, 1): hx.Result(rng.standard_normal((2, 9)), spin=(0, 2), axis=-1)}
    out = hx.debias_cls(cls, bias)
    assert np.array_equal(out["P", "G", 1, 1], cls["P", "G", 1, 1] - bias["P", "G", 1, 1].array)
    assert np.array_equal(out["P", "P", 1, 1], cls["P", "P", 1, 1])


def test_deproject_maps_checks_its_keys_before_computing():
    npix = 12
    fields = {"P": _F(0, "V"), "G": _F(2, "W"), "N": _F(0, None)}
    maps = {("P", 1): np.zeros(npix), ("G", 1): np.zeros((2, npix))}
    masks = {("V", 1): np.ones(npix), ("W", 1): np.ones(npix)}
    with pytest.raises(KeyError, match=r"\('W', 1\)"):
        hx.deproject_maps(fields, maps, {"G": np.ones((1, 2, npix))}, {("V", 1): np.ones(npix)})
    with pytest.raises(KeyError, match="Q"):
        hx.deproject_maps(fields, maps, {"Q": np.ones((1, npix))}, masks)
    with pytest.raises(KeyError, match=r"\('P', 2\)"):
        hx.deproject_maps(fields, maps, {("P", 2): np.ones((1, npix))}, masks)
    with pytest.raises(ValueError, match=r"\('G', 1\)"):
        hx.deproject_maps(fields, maps, {"G": np.ones((1, npix))}, masks)  # one component for a spin-2 field
    with pytest.raises(ValueError, match=r"\('P', 1\)"):
        hx.deproject_maps(fields, maps, {"P": np.ones((3, npix + 1))}, masks)
    with pytest.raises(ValueError, match="no mask"):
        hx.deproject_maps(fields, {("N", 1): np.zeros(npix)}, {"N": np.ones((1, npix))}, masks)
    with pytest.raises(ValueError, match="unknown field"):
        hx.deproject_maps(fields, {("X", 1): np.zeros(npix)}, {"X": np.ones((1, npix))}, masks)
    # nothing to clean: the maps pass through untouched, no library call is made
    same, infos = hx.deproject_maps(fields, maps, {}, masks)
    assert infos == {} and all(same[k] is maps[k] for k in maps)


def mc_units(oracle, s):
    """The two fields of the Monte Carlo setup as the reference's bias takes them."""
    vp, vg = s["masks"]
    units = {}
    for name, spin, v in (("P", 0, vp), ("G", 2, vg)):
        f = s["templates"][name] * v
        G, _ = dr.gram(s["templates"][name], np.zeros((0,) + f.shape[1:]), v)
        M, rank, _, cond = dr.pinv(G)
        assert rank == dr.MC["ntemp"] and cond <= 100, (name, rank, cond)
        units[name] = dict(spin=spin, v=v, f=f, M=M)
    return units


def mc_bias_vector(oracle, s, units):
    c = dr.MC
    b = s["blocks"]
    L = c["lmax"]
    pp = dr.bias(oracle, c["nside"], L, c["niter"], units["P"], units["P"], b["P", "P", 1, 1].reshape(1, 1, -1))
    pg = dr.bias(oracle, c["nside"], L, c["niter"], units["P"], units["G"], b["P", "G", 1, 1].reshape(1, 2, -1))
    gg = dr.bias(oracle, c["nside"], L, c["niter"], units["G"], units["G"], b["G", "G", 1, 1])
    return dr.mc_vector(pp, pg, gg)


def test_bias_passes_the_monte_carlo_check(oracle):
    c = dr.MC
    nside, L, n = c["nside"], c["lmax"], c["nreal"]
    s = dr.mc_setup(oracle)
    assert np.abs(s["masks"][0] - s["masks"][1]).max() > 0.05 and s["masks"].min() > 0
    units = mc_units(oracle, s)
    bias = mc_bias_vector(oracle, s, units)
    rng = np.random.default_rng(c["seed"] + 1)
    delta = np.empty((n, 7 * (L + 1)))

    def vector(dpm, dgm):
        alm = oracle.map2alm(dpm, nside, L, spin=0, niter=c["niter"])
        eb = oracle.map2alm(dgm, nside, L, spin=2, niter=c["niter"])
        return dr.mc_vector(oracle.alm2cl(alm[0]), oracle.alm2cl(alm[0], eb), oracle.alm2cl(eb, eb))

    for r in range(n):
        alm = dr.mc_alms(rng, s["cl"])
        dpm = oracle.alm2map(alm[:1], nside, L) * s["masks"][0]
        dgm = oracle.alm2map(alm[1:], nside, L, spin=2) * s["masks"][1]
        cp = dr.deproject_double(dpm, units["P"]["f"], units["P"]["M"])
        cg = dr.deproject_double(dgm, units["G"]["f"], units["G"]["M"])
        delta[r] = vector(cp, cg) - vector(dpm, dgm)
    zmax, zrms = dr.mc_statistic(delta, bias, L + 1, c["lmin"])
    zmax0, zrms0 = dr.mc_statistic(delta, np.zeros_like(bias), L + 1, c["lmin"])
    print(f"Monte Carlo, oracle, n = {n}: max |z| = {zmax:.2f}, rms z = {zrms:.3f}; with the bias set to zero: max |z| = {zmax0:.1f}, rms z = {zrms0:.2f}")
    assert zmax0 > 6, zmax0  # the check can tell a missing bias
    assert zmax <= 6, zmax
    assert 0.8 <= zrms <= 1.2, zrms
