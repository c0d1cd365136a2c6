"""The run-time-spin sweeps (k_legendre_valu<SPIN_ANY>, k_legendre_synth_valu<SPIN_ANY, 1>, k_alm_reduce_spin) at BASELINE.json's full
size, nside 4096 / lmax 6144: recursions of 6000 steps, seed factors from 6000-term products, chains that start at extended exponents
near -75, 64 ring groups summed per order.  Against the long-double direct sums of tests/spin_reference.py and
tests/spin_synthesis_reference.py on a sample of orders (tests/test_spin_reference.py ties them to the oracle at this lmax to 1e-11),
against each other (adjointness), and, for spin 2 through these sweeps, against the oracle on every 512th m.  Every input is built on
the device; sparse maps keep the direct sums at a few seconds."""

import numpy as np
import pytest

import helpers
from healpix_pixels import pixel_angles, ring_of, ring_table, special_pixels
from spin_reference import points2alm_spin
from spin_synthesis_reference import alm2points_spin

pytestmark = pytest.mark.gpu

NSIDE, LMAX = 4096, 6144
NPIX = 12 * NSIDE * NSIDE
NLM = (LMAX + 1) * (LMAX + 2) // 2
# orders below the weights (the m < s seeds, chains from l0 = s > m), m = s, a low odd order, the quarters of the range, and the last
# orders (m = lmax: one row)
ORDERS = (0, 1, 2, 3, 97, 1536, 3072, 4608, 6000, 6143, 6144)


@pytest.fixture(scope="module")
def plan():
    import heracles_amd as hx

    return hx.get_plan(NSIDE, LMAX)


def _rows(orders=ORDERS):
    """Positions of the rows l = m .. lmax of the given orders in an m-major alm array."""
    return np.concatenate([np.arange(helpers.idx(LMAX, m, m), helpers.idx(LMAX, m, m) + LMAX - m + 1) for m in orders])


def _tolerance(theta):
    """Of the largest value.  1e-10: the yardstick of tests/test_gpu_fullsize.py's test_map2alm_against_oracle_on_sampled_m (both sides
    evaluate lambda_lm with relative error O(m eps)); near a pole the conditioning bound of tests/test_gpu_pointsht.py's
    test_long_transforms_on_sampled_m, 10 lmax 1.1e-16 / sin(theta_min) (a three-term recursion through x = cos(theta) in float64),
    theta_min the smallest co-latitude that carries a value."""
    return max(1e-10, 10 * LMAX * 1.1e-16 / np.sin(theta).min())


_SETS = {}


def _pixel_set(kind):
    """About 150 pixels.  'belt': the pixels where the ring geometry changes (healpix_pixels.special_pixels) and random ones, on rings
    with sin(theta) >= 0.1.  'polar': every pixel of the first two and the last two rings, the ends of ring nside and pixels between,
    and a few random pixels."""
    if kind not in _SETS:
        rng = np.random.default_rng(4096 + len(kind))
        start, nphi, _, sth, _ = ring_table(NSIDE)
        if kind == "belt":
            pix = special_pixels(NSIDE, rng, 160)
            pix = pix[sth[ring_of(NSIDE, pix)] >= 0.1]
        else:
            r = NSIDE - 1  # (0-based: ring nside)
            pix = np.concatenate([np.arange(12), np.arange(NPIX - 12, NPIX), [start[r], start[r] + nphi[r] - 1],
                                  rng.integers(start[r], start[r] + nphi[r], 6), rng.choice(NPIX, 118, replace=False)])
            pix = np.unique(pix.astype(np.int64))
        assert 130 <= pix.size <= 160
        theta, phi = pixel_angles(NSIDE, pix)
        for a in (pix, theta, phi):
            a.setflags(write=False)
        _SETS[kind] = (pix, theta, phi)
    return _SETS[kind]


def _low_rows_are_zero(alm, s):
    """alm: a device tensor (2, NLM)."""
    return not any(bool(alm[:, helpers.idx(LMAX, m, m) : helpers.idx(LMAX, s, m)].any()) for m in range(s))


# ---- a. map2alm against the direct sum --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["belt", "polar"])
@pytest.mark.parametrize("s", [1, 3])
def test_map2alm_against_direct_sum_on_sampled_m(plan, s, kind):
    import torch

    pix, theta, phi = _pixel_set(kind)
    rng = np.random.default_rng(10 * s + len(kind))
    vals = rng.standard_normal((2, pix.size))
    x = torch.zeros((2, NPIX), dtype=torch.float64, device="cuda")
    x[:, torch.as_tensor(np.array(pix)).cuda()] = torch.as_tensor(vals).cuda()  # (a copy: the shared set is read-only)
    b = torch.empty((2, NLM), dtype=torch.complex128, device="cuda")
    plan.map2alm(x, s, out=b, niter=0)
    assert plan.last_chunks == 1
    rows = _rows()
    got = b[:, torch.as_tensor(rows).cuda()].cpu().numpy()
    want = points2alm_spin(theta, phi, vals * (4 * np.pi / NPIX), LMAX, s, orders=ORDERS)[:, rows]
    tol, scale = _tolerance(theta), np.abs(want).max()
    worst, at = 0.0, 0
    for m in ORDERS:  # (the rows of the orders follow each other in `rows`)
        e = np.abs(got[:, at : at + LMAX - m + 1] - want[:, at : at + LMAX - m + 1]).max() / scale
        print(f"  s {s} {kind} m {m}: {e:.3e}")
        worst, at = max(worst, e), at + LMAX - m + 1
    print(f"nside {NSIDE} lmax {LMAX} s {s} {kind} map ({pix.size} pixels): err {worst:.3e}, bound {tol:.3e}")
    assert scale > 0 and worst < tol
    assert _low_rows_are_zero(b, s)


# ---- b. alm2map against the direct sum --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 3])
def test_alm2map_against_direct_sum_on_sampled_m(plan, s):
    """alms in the orders ORDERS only, drawn as in tests/test_gpu_fullsize.py's test_synthesis_against_closed_form_on_rings (random
    values / sqrt(1 + l)), zero below l = s; compared at the pixels of the two sets of (a), each with its own bound and scale."""
    import torch

    rng = np.random.default_rng(99 + s)
    alm = np.zeros((2, NLM), dtype=np.complex128)
    for m in ORDERS:
        l0 = max(m, s)
        if l0 > LMAX:
            continue
        lo, n = helpers.idx(LMAX, l0, m), LMAX - l0 + 1
        v = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n)) * (m > 0)
        alm[:, lo : lo + n] = v / np.sqrt(1.0 + np.arange(l0, LMAX + 1))
    y = torch.empty((2, NPIX), dtype=torch.float64, device="cuda")
    plan.alm2map(torch.as_tensor(alm).cuda(), s, out=y)
    sets = [_pixel_set(kind) for kind in ("belt", "polar")]
    pix = np.concatenate([p for p, _, _ in sets])
    want = alm2points_spin(np.concatenate([t for _, t, _ in sets]), np.concatenate([f for _, _, f in sets]), alm, LMAX, s, orders=ORDERS)
    got = y[:, torch.as_tensor(pix).cuda()].cpu().numpy()
    at = 0
    for kind, (p, theta, _) in zip(("belt", "polar"), sets):
        w, g = want[:, at : at + p.size], got[:, at : at + p.size]
        at += p.size
        err, tol = np.abs(g - w).max() / np.abs(w).max(), _tolerance(theta)
        print(f"nside {NSIDE} lmax {LMAX} s {s} {kind} pixels ({p.size}): err {err:.3e}, bound {tol:.3e}")
        assert err < tol, kind


# ---- c. adjointness ---------------------------------------------------------------------------------------------------------------
def _random_alm(torch, seed, s):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn((2, NLM, 2), dtype=torch.float64, device="cuda", generator=g)
    a[:, : LMAX + 1, 1] = 0.0  # m = 0 is real
    a = torch.view_as_complex(a)
    for m in range(s):  # l < s carries nothing
        a[:, helpers.idx(LMAX, m, m) : helpers.idx(LMAX, s, m)] = 0.0
    return a


@pytest.mark.parametrize("s", [1, 3])
def test_analysis_is_the_adjoint_of_synthesis(plan, s):
    """The identity of tests/test_gpu_fullsize.py's test of this name, with its bound, for dense random (Q, U) and (E, B): exact up to
    rounding, so every (l, m, ring) term of the run-time-spin analysis is tied to the run-time-spin synthesis; and bit-reproducible:
    the 64 ring groups of an order are summed in a fixed order."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(170 + s)
    x = torch.randn((2, NPIX), dtype=torch.float64, device="cuda", generator=g)
    a = _random_alm(torch, 230 + s, s)
    y = torch.empty_like(x)
    plan.alm2map(a, s, out=y)
    b = torch.empty_like(a)
    plan.map2alm(x, s, out=b, niter=0)
    w = torch.full((NLM,), 2.0, dtype=torch.float64, device="cuda")
    w[: LMAX + 1] = 1.0
    lhs = float((x * y).sum()) * 4.0 * np.pi / NPIX
    rhs = float((w * (a.real * b.real + a.imag * b.imag)).sum())
    scale = float(torch.linalg.vector_norm(x) * torch.linalg.vector_norm(y)) * 4.0 * np.pi / NPIX
    print(f"nside {NSIDE} lmax {LMAX} s {s}: lhs {lhs:.15e} rhs {rhs:.15e} diff / scale {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 1e-10 * scale, (lhs, rhs, scale)
    assert _low_rows_are_zero(b, s) and bool(torch.isfinite(b.real).all()) and bool(torch.isfinite(b.imag).all())
    b2 = torch.empty_like(b)
    plan.map2alm(x, s, out=b2, niter=0)
    assert torch.equal(b, b2)


# ---- d. spin 2 through the general sweeps -----------------------------------------------------------------------------------------
def test_spin2_through_the_general_sweep_against_oracle_on_sampled_m(plan, oracle, monkeypatch):
    """HX_SPIN_GENERIC=1 (read on every call) sends s = 2 through the run-time-spin sweep: a dense random map against the oracle's own
    map2alm with its Legendre stage restricted to every 512th m, exactly as tests/test_gpu_fullsize.py's
    test_map2alm_against_oracle_on_sampled_m judges the spin-2 kernel.  The result differs from the spin-2 kernel's somewhere (the
    hook did take the other path), and without the variable the spin-2 kernel's result is bit for bit what it was."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((2, NPIX), dtype=torch.float64, device="cuda", generator=g)
    usual, gen, after = (torch.empty((2, NLM), dtype=torch.complex128, device="cuda") for _ in range(3))
    plan.map2alm(x, 2, out=usual, niter=0)
    monkeypatch.setenv("HX_SPIN_GENERIC", "1")
    plan.map2alm(x, 2, out=gen, niter=0)
    monkeypatch.delenv("HX_SPIN_GENERIC")
    plan.map2alm(x, 2, out=after, niter=0)
    stride = 512
    oracle.set_mstride(stride)
    try:
        ref = oracle.map2alm(x.cpu().numpy(), NSIDE, LMAX, spin=2)
    finally:
        oracle.set_mstride(1)
    got = gen.cpu().numpy()
    scale = np.abs(got).max()
    worst = 0.0
    for m in range(0, LMAX + 1, stride):
        sl = slice(helpers.idx(LMAX, m, m), helpers.idx(LMAX, m, m) + LMAX - m + 1)
        worst = max(worst, np.abs(got[:, sl] - ref[:, sl]).max())
    print(f"nside {NSIDE} lmax {LMAX}: general sweep against the oracle {worst / scale:.3e}, "
          f"against the spin-2 kernel {float((gen - usual).abs().max()) / scale:.3e}")
    assert worst <= 1e-10 * scale
    assert float((gen - usual).abs().max()) > 0.0
    assert torch.equal(after, usual)
