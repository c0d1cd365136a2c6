"""hx_rotate_alm and its Python surface on the GPU against the numpy restatement of the definition (tests/rotation_reference.py;
pinned on its own in tests/test_rotation_host.py).

Tolerance against the restatement: |delta| <= 1e-12 max|a_ref| per component -- the project's figure for f64 results against a
long-hand restatement (tests/test_gpu_synalm.py).  The scaled-seed test at lmax 700 prints the restatement's own unitarity defect next
to its figures.  Production lmax and small angles: tests/test_gpu_rotate_alm_fullsize.py."""

import numpy as np
import pytest

import rotation_reference as rr

pytestmark = pytest.mark.gpu

TOL = 1e-12

# the tiling of the kernel (csrc/hx_rotate.hip; tests/test_rotation_host.py holds these against the source)
from heracles_amd.rotation import TILE_COLS, TILE_COMP, TILE_L, TILE_M  # noqa: E402

GENERIC = (0.7, 1.234, -2.1)
#: lmax: the issue's six, then one below and one at every tile constant (lmax + 1 orders and multipoles; lmax = TILE_M is the first
#: with a second block of pairs, lmax = TILE_L the first column with a second tile, lmax = TILE_COLS the first with a second group of
#: columns)
LMAX_CASES = sorted({0, 1, 2, 3, 33, 96, TILE_COMP - 1, TILE_COMP, TILE_COLS - 1, TILE_COLS, TILE_L - 1, TILE_L, TILE_M - 1, TILE_M})
#: the issue's four (one block, one block + 1) and 2: with one, two and three or four components a work-group deals its (column,
#: component) pairs to its waves in different ways
NCOMP_CASES = [1, 2, 3, TILE_COMP, TILE_COMP + 1]


@pytest.fixture(scope="module")
def hx():
    import heracles_amd

    heracles_amd.init(0)
    return heracles_amd


def assert_close(got, ref, tol=TOL, what=""):
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    assert got.shape == ref.shape
    for i, (g, r) in enumerate(zip(got, ref)):
        err, scale = np.abs(g - r).max(), np.abs(r).max()
        print(f"{what} component {i}: max |delta| = {err:.3e}, max |a_ref| = {scale:.3e}, ratio {err / scale if scale else 0:.2e}")
        assert err <= tol * scale, (what, i, err, scale)


@pytest.fixture(scope="module")
def case40():
    """One alm at lmax 40 for the angle edges."""
    return rr.random_alm(np.random.default_rng(40), 40, 2)


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lmax", LMAX_CASES)
def test_restatement(hx, lmax):
    rng = np.random.default_rng(100 + lmax)
    alm = rr.random_alm(rng, lmax, max(NCOMP_CASES))
    ref = rr.rotate_alm_ref(alm, lmax, *GENERIC)
    for ncomp in NCOMP_CASES:
        got = hx.rotate_alm(alm[:ncomp], *GENERIC)
        assert got.shape == (ncomp, alm.shape[1]) and got.dtype == np.complex128
        assert_close(got, ref[:ncomp], what=f"lmax {lmax} ncomp {ncomp}")


# ---- 2. the defining identity on the GPU ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("psi,theta,phi", [GENERIC, (-2.9, 2.6, 0.3)])
def test_defining_identity(hx, psi, theta, phi):
    lmax, npts = 24, 200
    rng = np.random.default_rng(24)
    alm = rr.random_alm(rng, lmax)
    th, ph = np.arccos(rng.uniform(-1, 1, npts)), rng.uniform(0, 2 * np.pi, npts)
    back_th, back_ph = rr.angles(rr.rotation_matrix(psi, theta, phi).T @ rr.directions(th, ph))
    want = rr.values(alm, lmax, back_th, back_ph)  # f(R^-1 n)
    got = rr.values(hx.rotate_alm(alm, psi, theta, phi), lmax, th, ph)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"identity: max |delta| = {err:.3e}, max |f| = {scale:.3e}")
    assert err <= TOL * scale


# ---- 3. angle edges ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("theta", [0.0, np.pi, np.pi / 2, 1e-8, np.pi - 1e-8, -0.7, 4.0])
def test_angle_edges(hx, case40, theta):
    psi, phi = 0.9, -1.7
    got = hx.rotate_alm(case40, psi, theta, phi)
    assert_close(got, rr.rotate_alm_ref(case40, 40, psi, theta, phi), what=f"theta {theta!r}")
    if theta == 0.0:  # the z-rotation phases and nothing else
        _, m = rr.lm_index(40)
        assert_close(got, case40 * np.exp(-1j * m * (psi + phi)), tol=4e-16 * 40, what="phases")


def test_pure_z_rotation_and_forms(hx, case40):
    _, m = rr.lm_index(40)
    got = hx.rotate_alm(case40, 0.0, 0.0, 1.1)
    assert_close(got, rr.rotate_alm_ref(case40, 40, 0.0, 0.0, 1.1), what="z")
    assert_close(got, case40 * np.exp(-1j * m * 1.1), tol=4e-16 * 40, what="z phases")
    # matrix= and coord= are the equivalent angles, bit for bit
    R = hx.matrix_from_euler(*GENERIC)
    assert (hx.rotate_alm(case40, matrix=R) == hx.rotate_alm(case40, *hx.euler_from_matrix(R))).all()
    assert_close(hx.rotate_alm(case40, matrix=R), rr.rotate_alm_ref(case40, 40, *GENERIC), what="matrix")
    gc = hx.coord_matrix("G", "C")
    by_coord = hx.rotate_alm(case40, coord=("G", "C"))
    assert (by_coord == hx.rotate_alm(case40, *hx.euler_from_matrix(gc))).all()
    assert_close(by_coord, rr.rotate_alm_ref(case40, 40, *hx.euler_from_matrix(gc)), what="coord")


# ---- 4. scaled seeds ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def alm700():
    return rr.random_alm(np.random.default_rng(700), 700)


@pytest.mark.parametrize("theta", [0.02, np.pi - 0.02, 1.3])
def test_scaled_seeds(hx, alm700, theta):
    """At theta = 0.02 the seeds sqrt(C(2A, A+B)) cos^(A+B) sin^(A-B) of the chains leave the range of a double near m ~ 180."""
    lmax, psi, phi = 700, 0.4, -0.8
    got = hx.rotate_alm(alm700, psi, theta, phi)
    l, _ = rr.lm_index(lmax)
    for ll in (699, 700, 350):
        sel = np.flatnonzero(l == ll)
        d = rr.wigner_d(ll, theta)
        defect = np.abs(d.T @ d - np.eye(2 * ll + 1)).max()
        ref = rr.rotate_rows(alm700[sel], ll, psi, theta, phi)
        err, scale = np.abs(got[sel] - ref).max(), np.abs(ref).max()
        bound = TOL  # no allowance for the restatement: sin(theta) < 0.1 is rotated in two passes and stays below 2e-13 here
        print(f"theta {theta!r} l {ll}: max |delta| / max|a_ref| = {err / scale:.3e}, unitarity defect of the restatement {defect:.3e}, bound {bound:.3e}")
        assert err <= bound * scale, (ll, err, scale, defect)


# ---- 5. group properties -----------------------------------------------------------------------------------------------------------------

def test_group_properties(hx):
    lmax = 512
    alm = rr.random_alm(np.random.default_rng(512), lmax, 3)
    psi, theta, phi = GENERIC
    once = hx.rotate_alm(alm, psi, theta, phi)
    assert_close(hx.rotate_alm(once, -phi, -theta, -psi), alm, what="inverse")
    cl0, cl1 = hx.alm2cl(alm), hx.alm2cl(once)
    for i in range(3):
        err, scale = np.abs(cl1[i, i] - cl0[i, i]).max(), np.abs(cl0[i, i]).max()
        print(f"alm2cl component {i}: max |delta| = {err:.3e}, max = {scale:.3e}")
        assert err <= TOL * scale
    second = (-1.3, 0.6, 2.4)
    product = hx.matrix_from_euler(*second) @ hx.matrix_from_euler(psi, theta, phi)
    assert_close(hx.rotate_alm(once, *second), hx.rotate_alm(alm, matrix=product), what="composition")


# ---- 6. determinism and layout -----------------------------------------------------------------------------------------------------------

def test_determinism_and_batching(hx):
    lmax, ncomp = 70, 2 * TILE_COMP + 1
    alm = rr.random_alm(np.random.default_rng(70), lmax, ncomp)
    got = hx.rotate_alm(alm, *GENERIC)
    assert (hx.rotate_alm(alm, *GENERIC) == got).all()
    _, m = rr.lm_index(lmax)
    assert (got[:, m == 0].imag == 0).all()
    for i in range(ncomp):  # one by one: the same bits
        assert (hx.rotate_alm(alm[i], *GENERIC) == got[i]).all()
    for theta in (0.0, np.pi):
        assert (hx.rotate_alm(alm, 0.3, theta, 0.5)[:, m == 0].imag == 0).all()


def test_rotate_alms_keeps_keys_order_and_metadata(hx):
    import torch

    rng = np.random.default_rng(6)
    a33, b33, a20 = rr.random_alm(rng, 33), rr.random_alm(rng, 33, 2), rr.random_alm(rng, 20)
    hx.update_metadata(a33, spin=0, nside=16)
    hx.update_metadata(b33, spin=2)
    dev = hx.DeviceArray(torch.from_numpy(rr.random_alm(rng, 33, 2)).cuda(), {"spin": 1})
    alms = {("K", 1): a33, ("G", 0): a20, ("SHE", 1): b33, ("D", 2): dev}
    out = hx.rotate_alms(alms, *GENERIC)
    assert list(out) == list(alms)
    assert out["K", 1].dtype.metadata == {"spin": 0, "nside": 16} and out["SHE", 1].dtype.metadata == {"spin": 2}
    assert out["G", 0].dtype.metadata is None
    assert isinstance(out["D", 2], hx.DeviceArray) and out["D", 2].dtype.metadata == {"spin": 1} and out["D", 2].tensor.is_cuda
    for key, alm in alms.items():
        one = hx.rotate_alm(alm, *GENERIC)
        assert out[key].shape == alm.shape
        both = [x.numpy() if isinstance(x, hx.DeviceArray) else x for x in (out[key], one)]
        assert (both[0] == both[1]).all()
    by_coord = hx.rotate_alms({"a": a20}, coord=("E", "G"))
    assert (by_coord["a"] == hx.rotate_alm(a20, matrix=hx.coord_matrix("E", "G"))).all()


def test_pointer_kinds_out_and_errors(hx):
    import torch

    lmax = 33
    alm = rr.random_alm(np.random.default_rng(33), lmax, 3)
    host = hx.rotate_alm(alm, *GENERIC)
    assert isinstance(host, np.ndarray)
    t = torch.from_numpy(alm).cuda()
    dev = hx.rotate_alm(t, *GENERIC)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and (dev.cpu().numpy() == host).all()
    assert (t.cpu().numpy() == alm).all()  # the input is left alone
    out = np.empty_like(alm)
    assert hx.rotate_alm(alm, *GENERIC, out=out) is out and (out == host).all()
    dout = torch.empty_like(t)
    assert hx.rotate_alm(alm, *GENERIC, out=dout) is dout and (dout.cpu().numpy() == host).all()  # host in, device out
    up = hx.rotate_alm(alm, *GENERIC, device="cuda")
    assert isinstance(up, hx.DeviceArray) and (up.numpy() == host).all()
    assert (hx.rotate_alm(alm, *GENERIC, lmax=lmax) == host).all()
    # overlap: there is no in-place rotation
    for a in (alm.copy(), t.clone()):
        with pytest.raises(hx.HxError, match="overlap") as e:
            hx.rotate_alm(a, *GENERIC, out=a)
        assert e.value.code == -1
    flat = np.zeros(2 * alm.size, dtype=np.complex128)
    with pytest.raises(hx.HxError, match="overlap"):
        hx.rotate_alm(flat[: alm.size].reshape(alm.shape), *GENERIC, out=flat[alm.shape[1] :][: alm.size].reshape(alm.shape))
    L = hx._lib.load()
    p, q = hx._lib.ptr(alm), hx._lib.ptr(out)
    assert L.hx_rotate_alm(-1, 1, p, q, 0.1, 0.2, 0.3) == -1
    assert L.hx_rotate_alm(lmax, 0, p, q, 0.1, 0.2, 0.3) == -1
    assert L.hx_rotate_alm(lmax, 1, p, q, 0.1, float("nan"), 0.3) == -1
    assert L.hx_rotate_alm(lmax, 1, p, q, float("inf"), 0.2, 0.3) == -1
    assert b"finite" in L.hx_last_error()
    # beyond the supported lmax: refused before the pointers (which hold lmax 33) are looked at
    assert L.hx_rotate_alm(32001, 1, p, q, 0.1, 0.2, 0.3) == -5
    assert b"32000" in L.hx_last_error()


def test_flops_and_profile(hx):
    alm = rr.random_alm(np.random.default_rng(5), 40)
    hx._lib.executed_flops(reset=True)
    hx._lib.profile_enable(True)
    hx._lib.profile_reset()
    hx.rotate_alm(alm, *GENERIC)
    hx._lib.profile_enable(False)
    _, valu = hx._lib.executed_flops(reset=True)
    # 41 columns, 41 pairs each, chains from max(m, m') to lmax: sum over (m, m') of (40 - max(m, m')) recurrence steps of 25 flops
    steps = sum(40 - max(m, p) for m in range(41) for p in range(41))
    assert valu >= 25 * steps
    assert hx._lib.profile_get("rotate_alm")[0] == 1
