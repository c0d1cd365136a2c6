"""hx_rotate_alm at the sizes it is used and timed at (lmax 2048, 6144) and above the size to which DESIGN.md 4.18 argues its square
roots exact (lmax 10240), and at small rotation angles, against the long-double column restatement ``rotation_reference.rotate_column_ref``
(pinned on its own in tests/test_rotation_host.py: against the eigh restatement, its seeds against exact integers, its row norms at
lmax 2048).

Tolerance: |delta| <= 1e-12 max |a_ref| of the column's component, the contract of tests/test_gpu_rotate_alm.py, with no allowance.
Every comparison prints its error, the scale and the yardstick: the same recurrence with float64 chains on the CPU against the long
double one (what plain FP64 can give; never asserted).

Inputs above lmax 2048 are zeros except random rows l >= l_lo.  The kernel does the same work whatever the values, the reference sums
the live rows only, and every output row l < l_lo has to be exactly 0.0 in both parts: the whole output detects a NaN, an Inf or an
overflow anywhere in the chains at no reference cost."""

import functools

import numpy as np
import pytest

import rotation_reference as rr

pytestmark = pytest.mark.gpu

TOL = 1e-12
PSI, PHI = 0.4, -0.8
PI_BELOW = float(np.nextafter(np.pi, 0))

#: all four waves of a group, both sides of the first pair-block edge, the middle, the last two columns
COLUMNS_2048 = [0, 1, 2, 3, 63, 64, 65, 1023, 2047, 2048]
SWEEP_COLUMNS = [2, 65, 1023]


@pytest.fixture(scope="module")
def hx():
    import heracles_amd

    heracles_amd.init(0)
    return heracles_amd


class Case:
    """One single-component input: the alm, its live rows, the phased rows of the reference per psi and the kernel's output per angles."""

    def __init__(self, lmax, lmin, seed):
        self.lmax, self.lmin = lmax, lmin
        self.alm = rr.sparse_alm(np.random.default_rng(seed), lmax, lmin)
        self.rows = functools.lru_cache(maxsize=2)(lambda psi: rr.phased_rows(self.alm, lmax, psi, lmin))
        self._out = {}

    def rotated(self, hx, psi, theta, phi):
        """The kernel's output, checked as a whole: finite everywhere, exactly zero below the first live row, Im a'_l0 = 0."""
        key = (psi, theta, phi)
        if key not in self._out:
            self._out.clear()  # one output at a time: 0.8 GB at lmax 10240
            out = hx.rotate_alm(self.alm, psi, theta, phi)
            assert out.shape == self.alm.shape and out.dtype == np.complex128
            assert np.isfinite(out.real).all() and np.isfinite(out.imag).all(), "non-finite output"
            for m in range(min(self.lmin, self.lmax + 1)):
                at = m * (2 * self.lmax + 1 - m) // 2 + m
                dead = out[at : at + self.lmin - m]
                assert not dead.real.any() and not dead.imag.any(), f"column {m}: output below the first live row {self.lmin} is not exactly zero"
            assert not out[: self.lmax + 1].imag.any()
            self._out[key] = out
        return self._out[key]

    def check(self, hx, columns, psi, theta, phi):
        out = self.rotated(hx, psi, theta, phi)
        bad = []
        for m in columns:
            ref = rr.rotate_column_ref(self.alm, self.lmax, m, psi, theta, phi, lmin=self.lmin, rows=self.rows(psi))
            yard = rr.rotate_column_ref(self.alm, self.lmax, m, psi, theta, phi, np.float64, lmin=self.lmin, rows=self.rows(psi))
            got = out[rr.column_slice(self.lmax, m)]
            err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            print(f"lmax {self.lmax} theta {theta!r} column {m}: max |delta| = {err:.3e}, max |a_ref| = {scale:.3e}, ratio {err / scale:.2e}; "
                  f"float64 chains on the CPU: {float(np.abs(yard - ref).max()) / scale:.2e}")
            if not err <= TOL * scale:
                bad.append((m, err / scale))
        assert not bad, f"theta {theta!r}: columns beyond {TOL} of max |a_ref|: {bad}"


@functools.lru_cache(maxsize=1)
def case(lmax, lmin):
    return Case(lmax, lmin, seed=lmax)


def gc_angles(hx):
    return tuple(float(a) for a in hx.euler_from_matrix(hx.coord_matrix("G", "C")))


# ---- lmax 2048, dense ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", COLUMNS_2048)
@pytest.mark.parametrize("theta", [1.234, 1e-8])
def test_lmax_2048_every_column_kind(hx, theta, m):
    case(2048, 0).check(hx, [m], PSI, theta, PHI)


@pytest.mark.parametrize("theta", [0.02, np.pi - 0.02, 1e-3, 3e-4, 1e-5, np.pi - 1e-8, PI_BELOW])
def test_lmax_2048_theta_sweep(hx, theta):
    case(2048, 0).check(hx, SWEEP_COLUMNS, PSI, theta, PHI)


def test_lmax_2048_galactic_to_equatorial(hx):
    case(2048, 0).check(hx, SWEEP_COLUMNS, *gc_angles(hx))


def test_lmax_2048_components(hx):
    """Five components: a block of four and a block of one.  Each is the single-component call bit for bit."""
    lmax, ncomp, m = 2048, 5, 1023
    rng = np.random.default_rng(5)
    alm = np.stack([rr.sparse_alm(rng, lmax) for _ in range(ncomp)])
    got = hx.rotate_alm(alm, PSI, 1.234, PHI)
    assert got.shape == alm.shape and np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    for i in range(ncomp):
        assert (hx.rotate_alm(alm[i], PSI, 1.234, PHI) == got[i]).all(), i
    for i in (0, 4):
        ref = rr.rotate_column_ref(alm[i], lmax, m, PSI, 1.234, PHI)
        yard = rr.rotate_column_ref(alm[i], lmax, m, PSI, 1.234, PHI, np.float64)
        err, scale = float(np.abs(got[i][rr.column_slice(lmax, m)] - ref).max()), float(np.abs(ref).max())
        print(f"component {i} column {m}: max |delta| = {err:.3e}, max |a_ref| = {scale:.3e}, ratio {err / scale:.2e}; "
              f"float64 chains on the CPU: {float(np.abs(yard - ref).max()) / scale:.2e}")
        assert err <= TOL * scale


# ---- lmax 2048, edges ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("theta", [1e-300, 5e-324])
def test_tiny_theta_is_the_z_rotation(hx, theta):
    """Not theta = 0: these take the recurrence, not the closed form, and have to give its phases (4e-16 lmax: the figure of
    tests/test_gpu_rotate_alm.py for a phase formed from m (psi + phi) in doubles)."""
    c = case(2048, 0)
    out = c.rotated(hx, PSI, theta, PHI)
    _, m = rr.lm_index(2048)
    want = c.alm * np.exp(-1j * m * (PSI + PHI))
    err, scale = np.abs(out - want).max(), np.abs(want).max()
    print(f"theta {theta!r}: max |delta| = {err:.3e}, max |a| = {scale:.3e}, ratio {err / scale:.2e}")
    assert err <= 4e-16 * 2048 * scale


@pytest.mark.parametrize("theta", [2 * np.pi, -np.pi, 3 * np.pi, 2 * np.pi - 1e-9, 1e6])
def test_theta_outside_zero_to_pi(hx, theta):
    """fmodl and the fold (psi - pi, 2 pi - theta, phi + pi) of the entry point; the reference does no range reduction at all."""
    case(2048, 0).check(hx, [2, 1023], PSI, theta, PHI)


# ---- lmax 6144 and 10240, rows l >= l_lo live ------------------------------------------------------------------------------------------

#: sin(0.1) = 0.0998 and sin(0.1003) = 0.1001: the last angle rotated in two passes and the first rotated in one (ROT_SPLIT_SIN = 0.1
#: of csrc/hx_rotate.hip), where a single pass is at its weakest
@pytest.mark.parametrize("which", ["G->C", "0.02", "0.1", "0.1003", "3.0413"])
def test_lmax_6144(hx, which):
    angles = gc_angles(hx) if which == "G->C" else (PSI, float(which), PHI)
    case(6144, 6000).check(hx, [4096, 5001, 6143, 6144], *angles)


def test_lmax_6144_long_chains_in_one_pass(hx):
    """Columns 0 and 2048 at an angle rotated in one pass: the longest chains where nothing of l(l+1) cos(theta) - m m' cancels.  With
    cos(theta) = x_hi + x_lo split at the nearest double the kernel's inner fma rounded x_lo away and column 0 was off by 1.7e-12 here."""
    case(6144, 6000).check(hx, [0, 2048], PSI, 0.15, PHI)


def test_lmax_10240(hx):
    """Above l + 1 = 9741 the argument ((l+1)^2 - m^2)((l+1)^2 - m'^2) of the kernel's rsqrt is no longer an exact double."""
    case(10240, 9742).check(hx, [10000, 10239, 10240], PSI, 1.234, PHI)
