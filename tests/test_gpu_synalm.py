"""hx_synalm / hx_cl_cholesky and their Python surface on the GPU against the numpy restatement of the definition
(tests/synalm_reference.py; pinned on its own in tests/test_synalm_host.py).

Tolerance against the reference: |delta| <= 1e-12 max|a_ref| per component -- the project's figure for f64 results against a
long-hand restatement.  The differences are libm's log / sin / cos / sqrt on |z| <= 8.6 and FMA contraction in sums of <= N terms."""

import ctypes

import numpy as np
import pytest

import synalm_reference as sr

pytestmark = pytest.mark.gpu

TOL = 1e-12

# the tiling of the generator kernel (csrc/hx_synalm.hip; tests/test_synalm_host.py holds these against the source)
from heracles_amd.mocks import MAX_COMPONENTS, TILE_COMP, TILE_COMP_SMALL, TILE_L, TILE_M  # noqa: E402

WAVE = 64
#: (N, lmax): the issue's three, then one case on each side of every tile constant (lmax + 1 multipoles and orders, N components)
FULL_CASES = [
    (1, 4), (3, 33), (9, 70),
    (2, TILE_M - 1), (2, TILE_M),              # one chunk of orders / a second chunk with one order
    (2, WAVE - 1), (2, WAVE),                  # one full wave / one lane into the next
    (3, TILE_L - 1), (2, TILE_L),              # one full work-group of multipoles / one into the next
    (TILE_COMP_SMALL, 12), (TILE_COMP_SMALL + 1, 12),  # the last call of the small-block kernel / the first of the large-block one
    (TILE_COMP, 12), (TILE_COMP + 1, 12),      # one full register block / one row into the next
    (2 * TILE_COMP + 1, 9),                    # three register blocks
]


@pytest.fixture(scope="module")
def hx():
    import heracles_amd

    heracles_amd.init(0)
    return heracles_amd


def assert_close(got, ref):
    for i, (g, r) in enumerate(zip(got, ref)):
        err, scale = np.abs(g - r).max(), np.abs(r).max()
        print(f"component {i}: max |delta| = {err:.3e}, max |a_ref| = {scale:.3e}, ratio {err / scale if scale else 0:.2e}")
        assert err <= TOL * scale, (i, err, scale)


def identity(lmax):
    return sr.pack(np.broadcast_to(np.eye(2)[:, :, None], (2, 2, lmax + 1)))


# ---- 1. identity spectra ---------------------------------------------------------------------------------------------------------------

def test_identity_spectra(hx):
    seed = (1 << 35) + 17
    got = {lmax: hx.synalm_components(identity(lmax), 2, seed=seed) for lmax in (0, 1, 5)}
    for lmax, a in got.items():
        l, m = sr.lm_index(lmax)
        assert a.shape == (2, l.size)
        assert_close(a, sr.synalm(identity(lmax), 2, seed))  # the alms are the normals themselves
        assert (a[:, m == 0].imag == 0).all()
        assert (hx.synalm_components(identity(lmax), 2, seed=seed) == a).all()  # bit-identical on a second call
    a = got[5]
    assert (hx.synalm_components(identity(5), 2, seed=seed + 1) != a).all()
    assert (hx.synalm_components(identity(5), 2, seed=seed + (1 << 32)) != a).all()  # the high key word
    assert (hx.synalm_components(identity(5), 2, seed=seed, realisation=1) != a).all()
    assert (a[0] != a[1]).all()
    l5, _ = sr.lm_index(5)
    assert (a[:, l5 <= 1] == got[1]).all()  # lmax 5 extends lmax 1 bit for bit
    assert (a[:, l5 == 0] == got[0]).all()


# ---- 2. full matrices --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ncomp,lmax", FULL_CASES)
def test_full_matrix(hx, ncomp, lmax):
    packed = sr.pack(sr.conditioned_spectra(ncomp, lmax, 100 * ncomp + lmax))
    seed = (1 << 32) * (ncomp + 3) + lmax
    got = hx.synalm_components(packed, ncomp, seed=seed, realisation=2)
    assert_close(got, sr.synalm(packed, ncomp, seed, realisation=2))


# ---- 3. semi-definite input ------------------------------------------------------------------------------------------------------------

def test_component_without_power(hx):
    C = sr.conditioned_spectra(3, 20, 5)
    C[2, :, :] = C[:, 2, :] = 0.0
    C[:, :, :2] = 0.0
    got = hx.synalm_components(sr.pack(C), 3, seed=1 << 33)
    l, _ = sr.lm_index(20)
    assert (got[2] == 0).all() and (got[:, l < 2] == 0).all()
    assert (got[:2][:, l >= 2] != 0).all()
    assert_close(got, sr.synalm(sr.pack(C), 3, 1 << 33))


def test_identical_components_give_identical_rows(hx):
    lmax = 17
    c = 4.0 ** -(np.arange(lmax + 1) % 6)  # exact square roots: the second pivot is exactly 0 in any arithmetic
    got = hx.synalm_components(np.stack([c, c, c]), 2, seed=(1 << 34) + 1)
    assert (got[0] == got[1]).all() and (got[0] != 0).all()
    assert_close(got, sr.synalm(np.stack([c, c, c]), 2, (1 << 34) + 1))


@pytest.mark.parametrize("ncomp,lmax", [(1, 4), (3, 33), (9, 70)])
def test_cl_cholesky(hx, ncomp, lmax):
    from heracles_amd.mocks import cl_cholesky

    packed = sr.pack(sr.conditioned_spectra(ncomp, lmax, 100 * ncomp + lmax))
    got, ref = cl_cholesky(packed, ncomp), sr.cholesky(packed, ncomp)
    # per l: the entries of L_l share the scale 1 / (l + 1)
    err, scale = np.abs(got - ref).max(axis=0), np.abs(ref).max(axis=0)
    print(f"factor: worst |delta| / max|L_l| = {(err / scale).max():.2e}")
    assert (err <= TOL * scale).all()


# ---- 4. rejection --------------------------------------------------------------------------------------------------------------------------

def test_rejection(hx):
    C = np.zeros((2, 2, 6))
    C[0, 0] = C[1, 1] = 1.0
    C[:, :, 3] = [[1, 2], [2, 1]]
    C[:, :, 5] = [[1, 3], [3, 1]]  # a later failure: the smallest l is the one named
    out = np.full((2, 21), -7.5 + 2j)
    with pytest.raises(hx.HxError, match=r"l = 3\b") as e:
        hx.synalm_components(sr.pack(C), 2, seed=1, out=out)
    assert e.value.code == -1
    assert (out == -7.5 + 2j).all()
    import torch

    dev = torch.full((2, 21), -7.5 + 2j, dtype=torch.complex128, device="cuda")
    with pytest.raises(hx.HxError, match=r"l = 3\b"):
        hx.synalm_components(torch.from_numpy(sr.pack(C)).cuda(), 2, seed=1, out=dev)
    assert bool((dev == -7.5 + 2j).all())
    bad = identity(4)
    bad[1, 2] = np.nan
    with pytest.raises(hx.HxError, match="NaN"):
        hx.synalm_components(bad, 2, seed=1)
    bad[1, 2] = np.inf
    with pytest.raises(hx.HxError):
        hx.synalm_components(bad, 2, seed=1)
    n = MAX_COMPONENTS + 1
    with pytest.raises(hx.HxError) as e:
        hx.synalm_components(np.ones((n * (n + 1) // 2, 2)), n, seed=1)
    assert e.value.code == -1
    L = hx._lib.load()
    chol = np.full((3, 6), 9.0)
    assert L.hx_cl_cholesky(2, 5, hx._lib.ptr(sr.pack(C)), hx._lib.ptr(chol)) == -1 and (chol == 9.0).all()
    assert L.hx_synalm(0, 5, hx._lib.ptr(chol), ctypes.c_uint64(1), 0, hx._lib.ptr(out)) == -1
    assert L.hx_synalm(1, -1, hx._lib.ptr(chol), ctypes.c_uint64(1), 0, hx._lib.ptr(out)) == -1


# ---- 5. round trip through the public interface ------------------------------------------------------------------------------------------

def test_round_trip(hx):
    C = sr.roundtrip_matrix()
    cls = sr.matrix_to_cls(C, sr.ROUNDTRIP_FIELDS)
    alms = hx.synalm(cls, seed=sr.ROUNDTRIP_SEED, device="cuda")
    assert all(isinstance(a, hx.DeviceArray) for a in alms.values())
    base = alms["POS", 1].tensor.data_ptr()
    nlm = (sr.ROUNDTRIP_LMAX + 1) * (sr.ROUNDTRIP_LMAX + 2) // 2
    rows, _ = sr.field_rows(sr.ROUNDTRIP_FIELDS)
    for key, a in alms.items():  # views of one (N, nlm) tensor
        assert a.tensor.data_ptr() == base + 16 * nlm * rows[key][0]
    est = hx.angular_power_spectra(alms, debias=False)
    assert list(est) == list(cls)
    for key in cls:
        assert est[key].shape == cls[key].shape, key
        assert est[key].spin == (cls[key].dtype.metadata["spin_1"], cls[key].dtype.metadata["spin_2"])
    sr.assert_spectra_statistics(C, sr.cls_to_matrix({k: np.asarray(v) for k, v in est.items()}, sr.ROUNDTRIP_FIELDS))
    got = np.concatenate([a.numpy().reshape(-1, nlm) for a in alms.values()])
    assert_close(got, sr.synalm(sr.pack(C), 6, sr.ROUNDTRIP_SEED))
    # the host route gives the same alms bit for bit
    host = hx.synalm(cls, seed=sr.ROUNDTRIP_SEED)
    assert (np.concatenate([a.reshape(-1, nlm) for a in host.values()]) == got).all()
    assert host["SHE", 2].dtype.metadata["spin"] == 2 and host["SHE", 2].shape == (2, nlm)


# ---- 6. gaussian_maps --------------------------------------------------------------------------------------------------------------------

@pytest.mark.filterwarnings("ignore:HipHealpixMapper")
def test_gaussian_maps(hx):
    nside, lmax = 16, 24
    mapper = hx.HipHealpixMapper(nside, lmax, deconvolve=False)
    fields = {"POS": hx.Positions(mapper, "ra", "dec"), "SHE": hx.Shears(mapper, "ra", "dec", "g1", "g2")}
    layout = (("POS", 0, 0), ("SHE", 0, 2))
    C = sr.conditioned_spectra(3, lmax, 9, {1: 2, 2: 2})
    cls = sr.matrix_to_cls(C, layout)
    seed = (1 << 36) + 5
    maps = hx.gaussian_maps(fields, cls, seed=seed, realisation=4)
    alms = hx.synalm(cls, seed=seed, realisation=4, lmax=lmax)
    plan = hx.get_plan(nside, lmax)
    assert list(maps) == [("POS", 0), ("SHE", 0)]
    assert maps["POS", 0].shape == (12 * nside**2,) and maps["SHE", 0].shape == (2, 12 * nside**2)
    for key, spin in ((("POS", 0), 0), (("SHE", 0), 2)):
        assert (maps[key] == plan.alm2map(alms[key], spin)).all()
        md = maps[key].dtype.metadata
        assert (md["spin"], md["nside"], md["kernel"]) == (spin, nside, "healpix")
    back = hx.transform(fields, maps)
    assert list(back) == list(maps)
    assert [a.dtype.metadata["spin"] for a in back.values()] == [0, 2]
    # band-limited maps on 16 x 16 x 12 pixels with unit weights: the alms come back to quadrature accuracy
    for key in maps:
        assert np.abs(back[key] - alms[key]).max() < 0.05 * np.abs(alms[key]).max()
    # a field with a smaller band limit gets the cut of the same realisation
    small = hx.HipHealpixMapper(nside, 16, deconvolve=False)
    fields2 = {"POS": hx.Positions(small, "ra", "dec"), "SHE": fields["SHE"]}
    maps2 = hx.gaussian_maps(fields2, cls, seed=seed, realisation=4)
    assert (maps2["SHE", 0] == maps["SHE", 0]).all()
    cut = hx.alm_resample(alms["POS", 0], 16)
    assert (maps2["POS", 0] == hx.get_plan(nside, 16).alm2map(cut, 0)).all()
    dev = hx.gaussian_maps(fields, cls, seed=seed, realisation=4, device="cuda")
    assert (dev["SHE", 0].numpy() == maps["SHE", 0]).all() and dev["SHE", 0].dtype.metadata["spin"] == 2


# ---- 7. pointer kinds --------------------------------------------------------------------------------------------------------------------

def test_pointer_kinds(hx):
    import torch

    packed = sr.pack(sr.conditioned_spectra(3, 33, 133))
    seed = (1 << 33) + 3
    host = hx.synalm_components(packed, 3, seed=seed)
    dev = hx.synalm_components(torch.from_numpy(packed).cuda(), 3, seed=seed)
    assert dev.is_cuda and (dev.cpu().numpy() == host).all()
    out = torch.empty((3, host.shape[1]), dtype=torch.complex128, device="cuda")
    assert hx.synalm_components(packed, 3, seed=seed, out=out) is out  # host spectra, device result
    assert (out.cpu().numpy() == host).all()
