"""The ring Fourier stage on its own, against the independent numpy reference of tests/ring_reference.py (direct per-ring
np.fft, the published HEALPix geometry): the analysis half through hx_ring_modes (HipStages.ring_modes: (F_N, F_S)(m, ring pair)
with phase and quadrature weight applied, the same launch_subdft_classes<0> as map2alm), the synthesis half through alm2map of
single (l, m) coefficients (one frequency on every ring whatever lambda_lm is), and the Jacobi residual pass of map2alm(niter).

The end-to-end SHT tests bound the ring stage only at the Legendre error (1e-11 .. 1e-9); these bound it at its own rounding.

Error measure, analysis: |F_gpu - F_ref| / (w_rp (||f_N w_pix||_2 + ||f_S w_pix||_2)), w_rp = rw[rp] 4 pi / npix, per FFT class of
the ring pair (M = fft_size_for(n) of its sub-DFTs, n = nphi / 4); synthesis: leakage max_{k != +-m} |X_k| / (sqrt(nphi) ||v||_2),
phase and north/south mirror likewise.  Measured on the MI355X (max over every case of this file, divided by log2 M):
    analysis   pair 1.78e-16, subdft-2^k 4.20e-16, Bluestein 3.23e-16, split Bluestein 1.85e-16
    synthesis  pair 6.64e-17, subdft-2^k 2.03e-16, Bluestein 1.09e-16, split Bluestein 6.67e-17
The bounds are about 8x these, capped at the ceiling 2e-15 log2 M (analysis subdft-2^k: 4.8x, analysis Bluestein: 6.2x); the
reference itself is good to < 2e-16 log2 M (tests/test_ring_reference.py).  There is no split plain class: a plan whose plain 2^k rings exceed the LDS limit is refused."""

import math

import numpy as np
import pytest

from helpers import idx, lambda_lm_column
from ring_reference import _rows, fft_size_for, ring_cos_sin, ring_pair_geometry, ring_phase, ring_spectra_ms

pytestmark = pytest.mark.gpu

CEIL = 2e-15  # x log2 M
# per class, x log2 M: about 8x the measured maximum (module docstring)
TOL_A = {"pair": 1.5e-15, "subdft-2^k": CEIL, "bluestein": CEIL, "split-bluestein": 1.5e-15}
TOL_S = {"pair": 5.5e-16, "subdft-2^k": 1.6e-15, "bluestein": 9e-16, "split-bluestein": 5.5e-16}
MEASURED = {"analysis": {}, "synthesis": {}}


def _lds_slots(M):
    return M + (M >> 4) + (M >> 9) + 1


def fft_class(n, cap=8192):
    """The kernel a ring pair with sub-DFTs of length n runs on (hx_ring_fft.hip: ring_class_is_pair, ring_fft_plan_init)."""
    M = fft_size_for(n)
    if M == n:
        pair = 16 <= M <= cap and (2 * _lds_slots(M) + (4 * M) // 64 + 1 + 64) * 16 + 4096 <= 160 * 1024
        return "pair" if pair else "subdft-2^k"
    return "split-bluestein" if M > cap else "bluestein"


def _tol(tab, cls, M):
    assert tab[cls] <= CEIL
    return tab[cls] * math.log2(max(M, 2))


def _record(kind, cls, val):
    MEASURED[kind][cls] = max(MEASURED[kind].get(cls, 0.0), float(val))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for kind, d in MEASURED.items():
        print(f"\nring stage {kind}: max err / log2 M: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(d.items())))


class _LdsCap:
    """hx_set_max_lds_fft(cap) for the plans created inside; the limit is restored to 8192 whatever happens."""

    def __init__(self, cap):
        self.cap = cap

    def __enter__(self):
        import heracles_amd as hx

        hx._lib.check(hx._lib.load().hx_set_max_lds_fft(self.cap))

    def __exit__(self, *exc):
        import heracles_amd as hx

        hx._lib.check(hx._lib.load().hx_set_max_lds_fft(8192))


def symmetric_pixel_weights(rng, nside):
    """Random weights with the symmetry of healpy's full weights: the same over the four quadrants of a ring and from its
    northern to its southern ring (pw_mode 2 of the plan, the WSYM ring kernels)."""
    geo = ring_pair_geometry(nside)
    w = np.empty(12 * nside**2)
    for rp in range(2 * nside):
        n = geo["nphi"][rp] // 4
        v = np.tile(1.0 + 0.2 * rng.standard_normal(n), 4)
        w[geo["startN"][rp] : geo["startN"][rp] + 4 * n] = v
        if geo["startS"][rp] >= 0:
            w[geo["startS"][rp] : geo["startS"][rp] + 4 * n] = v
    return w


def _ring_norms(maps, nside, pw):
    """||f w_pix||_2 of the northern and southern ring of every ring pair: [comp][rp] each."""
    geo = ring_pair_geometry(nside)
    ncomp = maps.shape[0]
    nN, nS = np.zeros((ncomp, 2 * nside)), np.zeros((ncomp, 2 * nside))
    for nphi in np.unique(geo["nphi"]):
        rps = np.flatnonzero(geo["nphi"] == nphi)
        for out, start in ((nN, geo["startN"]), (nS, geo["startS"])):
            live = rps[start[rps] >= 0]
            for b0 in range(0, live.size, 256):
                sub = live[b0 : b0 + 256]
                for c in range(ncomp):
                    f = _rows(maps[c], start[sub], int(nphi))
                    if pw is not None:
                        f = f * _rows(pw, start[sub], int(nphi))
                    out[c, sub] = np.linalg.norm(f, axis=1)
    return nN, nS


def _modes(plan, maps, sets, pw=None, rw=None):
    """HipStages.ring_modes into a NaN-filled send buffer: per set, (ncomp, count, nrp_pad, 4) on the host."""
    from heracles_amd.distributed import HipStages

    st = HipStages(plan)
    ncomp = maps.shape[0]
    flat = st.send_buffer(ncomp, sets)
    flat.fill_(float("nan"))
    blocks = st.ring_modes(maps, sets, pix_weights=pw, ring_weights=rw, out=flat)
    nrp_pad = (2 * plan.nside + 63) // 64 * 64
    return [b.view(ncomp, s[1], nrp_pad, 4).cpu().numpy() for b, s in zip(blocks, sets)], flat


def _check_block(blk, ms, ref, norms, w, nside, cap, ctx):
    """One set's block against the reference at its orders ms: layout, pruning, exact zeros and the per-class bound."""
    nrp = 2 * nside
    FNr, FSr = ref
    nN, nS = norms
    nan = np.isnan(blk)
    assert (nan == nan[..., :1]).all(), ctx  # a pruned entry is pruned as a whole
    nan = nan[..., 0]                         # (ncomp, count, nrp_pad)
    lead = np.where(nan.all(axis=2), blk.shape[2], np.argmin(nan, axis=2))
    assert (lead == lead[:1]).all(), ctx      # pruning depends on m only
    for k in range(blk.shape[1]):
        L = int(lead[0, k])
        assert L % 256 == 0 or L == blk.shape[2], (ctx, ms[k], L)
        assert not nan[:, k, L:].any(), (ctx, ms[k], "NaN behind the first written ring pair")
    written = ~nan
    pad = blk[:, :, nrp:]
    assert (pad[written[:, :, nrp:]] == 0).all(), ctx
    eq = blk[:, :, nrp - 1, 2:]
    assert (eq[written[:, :, nrp - 1]] == 0).all(), ctx
    FN = blk[:, :, :nrp, 0] + 1j * blk[:, :, :nrp, 1]
    FS = blk[:, :, :nrp, 2] + 1j * blk[:, :, :nrp, 3]
    err = np.maximum(np.abs(FN - FNr), np.abs(FS - FSr))            # (ncomp, count, nrp)
    scale = w[None, :] * (nN + nS)                                   # (ncomp, nrp)
    rel = np.where(written[:, :, :nrp], err / np.maximum(scale[:, None, :], 1e-300), 0.0).max(axis=(0, 1))  # per rp
    geo = ring_pair_geometry(nside)
    n = geo["nphi"] // 4
    for cls in {fft_class(int(v), cap) for v in n}:
        sel = np.array([fft_class(int(v), cap) == cls for v in n])
        lg = np.log2(np.maximum([fft_size_for(int(v)) for v in n], 2))
        worst = (rel[sel] / lg[sel]).max()
        _record("analysis", cls, worst)
        Ms = np.array([fft_size_for(int(v)) for v in n])[sel]
        bad = rel[sel] > np.array([_tol(TOL_A, cls, M) for M in Ms])
        assert not bad.any(), (ctx, cls, "worst rel err / log2 M %.3e" % worst, np.flatnonzero(sel)[bad][:8])


def _run_analysis(plan, nside, cap, maps, sets, pw, rw, ctx):
    import torch

    d_maps = torch.as_tensor(maps).cuda()
    d_pw = None if pw is None else torch.as_tensor(pw).cuda()
    d_rw = None if rw is None else torch.as_tensor(rw).cuda()
    blocks, flat = _modes(plan, d_maps, sets, d_pw, d_rw)
    w = (np.ones(2 * nside) if rw is None else rw) * 4 * np.pi / (12 * nside**2)
    norms = _ring_norms(maps, nside, pw)
    for (first, count, step), blk in zip(sets, blocks):
        ms = first + step * np.arange(count)
        assert blk.shape[1] == count
        if count == 0:
            continue
        ref = ring_spectra_ms(maps, nside, ms, pix_weights=pw, ring_weights=rw)
        _check_block(blk, ms, ref, norms, w, nside, cap, ctx)
    return d_maps, d_pw, d_rw, flat


# (nside, lmax, LDS cap, pixel weights, ring weights, ncomp, order sets)
ANALYSIS_CASES = [
    (1, 2, 8192, None, False, 1, "all"),
    (2, 6, 8192, "generic", True, 3, "cyclic5"),
    (4, 12, 8192, None, True, 16, "all"),
    (8, 24, 8192, "sym", False, 17, "cyclic5"),
    (12, 40, 8192, "generic", True, 3, "all"),
    (16, 48, 8192, "sym", True, 1, "edges"),
    (48, 100, 8192, None, False, 16, "all"),
    (32, 100, 32, "generic", True, 3, "all"),
    (48, 150, 64, "sym", True, 3, "cyclic5"),
    (64, 200, 64, None, False, 17, "all"),
    (256, 400, 8192, "generic", True, 3, "cyclic5"),
    (512, 1024, 8192, None, False, 3, "all"),
    (1024, 1535, 8192, "sym", True, 1, "cyclic5"),
]


def _sets(kind, lmax):
    if kind == "all":
        return [(0, lmax + 1, 1)]
    if kind == "cyclic5":
        return [(q, max(0, (lmax - q) // 5 + 1), 5) for q in range(5)]
    return [(lmax, 1, 1), (0, 0, 1), (0, 1, 1)]  # only m = lmax, an empty set, only m = 0


@pytest.mark.parametrize("nside,lmax,cap,pwk,rwk,ncomp,sets", ANALYSIS_CASES)
def test_ring_modes_against_reference(nside, lmax, cap, pwk, rwk, ncomp, sets):
    """Every class launch_subdft_classes dispatches (pair, small 2^k and Bluestein k_ring_subdft, split Bluestein under a lowered
    LDS limit), every weight mode (none / symmetric / generic pixel weights, ring weights off / random), batches of 1, 3, 16, 17
    components (17: a second ring-FFT launch) and the order sets all / cyclic step 5 / only lmax / empty."""
    import heracles_amd as hx

    rng = np.random.default_rng(1000 * nside + lmax + ncomp)
    npix = 12 * nside**2
    maps = rng.standard_normal((ncomp, npix))
    pw = {None: None, "generic": lambda: rng.uniform(0.5, 1.5, npix), "sym": lambda: symmetric_pixel_weights(rng, nside)}[pwk]
    pw = pw() if pw else None
    rw = rng.uniform(0.5, 1.5, 2 * nside) if rwk else None
    with _LdsCap(cap):
        plan = hx.Plan(nside, lmax)
    try:
        sets_ = _sets(sets, lmax)
        d_maps, d_pw, d_rw, flat = _run_analysis(plan, nside, cap, maps, sets_, pw, rw, (nside, lmax, cap, pwk, rwk, ncomp, sets))
        # two calls are bitwise equal; host inputs give what device inputs give
        again = _modes(plan, d_maps, sets_, d_pw, d_rw)[1]
        host = _modes(plan, maps, sets_, pw, rw)[1]
        np.testing.assert_array_equal(again.cpu().numpy(), flat.cpu().numpy())
        np.testing.assert_array_equal(host.cpu().numpy(), flat.cpu().numpy())
    finally:
        plan.close()


def test_ring_modes_fullsize_all_orders():
    """nside 4096 / lmax 6144, one component, every m and every ring pair, compared in m-chunks: the 16384-point pair rings of the
    belt, every polar length and the 8192-point Bluestein rings."""
    import torch

    import heracles_amd as hx

    nside, lmax = 4096, 6144
    rng = np.random.default_rng(4096)
    maps = rng.standard_normal((1, 12 * nside**2))
    rw = rng.uniform(0.5, 1.5, 2 * nside)
    plan = hx.get_plan(nside, lmax)
    d_maps, d_rw = torch.as_tensor(maps).cuda(), torch.as_tensor(rw).cuda()
    w = rw * 4 * np.pi / (12 * nside**2)
    norms = _ring_norms(maps, nside, None)
    chunk = 2048
    for m0 in range(0, lmax + 1, chunk):
        cnt = min(chunk, lmax + 1 - m0)
        (blk,), _ = _modes(plan, d_maps, [(m0, cnt, 1)], None, d_rw)
        ms = np.arange(m0, m0 + cnt)
        _check_block(blk, ms, ring_spectra_ms(maps, nside, ms, ring_weights=rw), norms, w, nside, 8192, ("4096", m0))
        del blk


def test_ring_modes_nside8192():
    """nside 8192 / lmax 8000, one component, all ring pairs: the split-Bluestein cap rings (4096 < n < 8192, 16384-point
    convolutions in two halves) and the plain 8192-point belt.  Orders: every residue mod 4 and mod 64 (0..127), both sides of 4096,
    the top order and a few in between."""
    import torch

    import heracles_amd as hx

    nside, lmax = 8192, 8000
    g = torch.Generator(device="cuda").manual_seed(8192)
    d_maps = torch.randn((1, 12 * nside**2), dtype=torch.float64, device="cuda", generator=g)
    maps = d_maps.cpu().numpy()
    rng = np.random.default_rng(8192)
    rw = rng.uniform(0.5, 1.5, 2 * nside)
    ms = np.array(sorted(set(range(128)) | {255, 256, 1000, 2047, 2048, 4095, 4096, 4097, 6000, 7999, 8000}))
    plan = hx.Plan(nside, lmax, 1)
    try:
        blocks, _ = _modes(plan, d_maps, [(int(m), 1, 1) for m in ms], None, torch.as_tensor(rw).cuda())
        del d_maps
        blk = np.concatenate(blocks, axis=1)
        w = rw * 4 * np.pi / (12 * nside**2)
        _check_block(blk, ms, ring_spectra_ms(maps, nside, ms, ring_weights=rw), _ring_norms(maps, nside, None), w, nside, 8192, "8192")
    finally:
        plan.close()


# ---- synthesis: spectral purity of single-coefficient alm2map ----
def _synth_check(plan, nside, lmax, spin, coeffs, rps, cap, ctx):
    """coeffs: per component (spin 0) / field (spin 2) (l, m, alpha, 'E' | 'B'); alm2map of all in ONE call, then per ring of rps:
    (a) leakage off the bins +-m mod nphi, (b) the phase of the bin m, (c) spin 0: the north/south mirror (-1)^(l+m),
    (d) spin 0: an all-zero ring only where 2 |lambda_lm| <= 1e-12 max |lambda_lm|."""
    import torch

    nf = len(coeffs)
    ncomp = nf * (2 if spin else 1)
    alm = np.zeros((ncomp, plan.nlm), dtype=np.complex128)
    for f, (l, m, al, eb) in enumerate(coeffs):
        alm[f if spin == 0 else 2 * f + (eb == "B"), idx(lmax, l, m)] = np.exp(1j * al)
    out = plan.alm2map(torch.as_tensor(alm).cuda(), spin)
    geo = ring_pair_geometry(nside)
    z, sth = ring_cos_sin(nside)
    rps = np.asarray(rps)
    pix = []  # per ring pair of rps: its northern ring, then its southern ring
    for rp in rps:
        for start in (geo["startN"][rp], geo["startS"][rp]):
            if start >= 0:
                pix.append(np.arange(start, start + geo["nphi"][rp]))
    allpix = np.concatenate(pix)
    vals = out[:, torch.as_tensor(allpix).cuda()].cpu().numpy()
    del out
    worst = {}
    for f, (l, m, al, eb) in enumerate(coeffs):
        lam = None
        if spin == 0:
            lam = np.abs(lambda_lm_column(m, l, z, sth)[-1]).astype(np.float64)
        s = 0
        for rp in rps:
            nphi = int(geo["nphi"][rp])
            n = nphi // 4
            cls, M = fft_class(n, cap), fft_size_for(n)
            b, bm = m % nphi, (-m) % nphi
            ph = ring_phase([m], nphi, bool(geo["shifted"][rp]))[0] * np.exp(-1j * al)
            halves = []
            for half in (0, 1):
                if half and geo["startS"][rp] < 0:
                    continue
                comps = (f,) if spin == 0 else (2 * f, 2 * f + 1)
                v2 = vals[list(comps), s + half * nphi : s + (half + 1) * nphi]
                nrm = np.linalg.norm(v2, axis=1).sum()  # spin 2: ||Q|| + ||U|| (one of them is exactly 0 at m = 0)
                if nrm == 0:
                    assert spin != 0 or 2 * lam[rp] <= 1e-12 * lam.max(), (ctx, l, m, rp, "pruned ring with lambda_lm %.3e" % lam[rp])
                    continue
                if nrm < 1e-280:
                    continue
                sc = math.sqrt(nphi) * nrm
                for t, c in enumerate(comps):
                    X = np.fft.fft(v2[t])
                    off = np.delete(np.abs(X), sorted({b, bm}))
                    errs = [off.max() / sc if off.size else 0.0]
                    zb = X[b] * ph
                    if b not in (0, nphi // 2):
                        if spin == 0:
                            bad = zb.imag
                        else:
                            q = c == 2 * f
                            bad = zb.imag if (q == (eb == "E")) else zb.real
                        errs.append(abs(bad) / sc)
                    if spin == 0:
                        halves.append((zb, nrm))
                    e = max(errs)
                    worst[cls] = max(worst.get(cls, 0.0), e / math.log2(max(M, 2)))
                    assert e <= _tol(TOL_S, cls, M), (ctx, spin, l, m, eb, rp, half, cls, e / math.log2(max(M, 2)))
            if spin == 0 and len(halves) == 2:
                (zn, an), (zs, as_) = halves
                e = abs(zs - (-1) ** (l + m) * zn) / (math.sqrt(nphi) * (an + as_))
                worst[cls] = max(worst.get(cls, 0.0), e / math.log2(max(M, 2)))
                assert e <= _tol(TOL_S, cls, M), (ctx, l, m, rp, "mirror", e / math.log2(max(M, 2)))
            s += nphi * (1 if geo["startS"][rp] < 0 else 2)
    for cls, v in worst.items():
        _record("synthesis", cls, v)


def _coeffs(lm, spin, rng):
    out = []
    for l, m in lm:
        al = 0.0 if m == 0 else float(rng.uniform(0, 2 * np.pi))
        if spin == 0:
            out.append((l, m, al, "E"))
        else:
            out += [(max(l, 2), m, al, "E"), (max(l, 2), m, al, "B")]
    return out


@pytest.mark.parametrize("nside,cap", [(16, 8192), (64, 8192), (12, 8192), (48, 8192), (48, 64), (32, 32)])
@pytest.mark.parametrize("spin", [0, 2])
def test_synthesis_spectral_purity(nside, cap, spin):
    """alm2map of one (l, m) per component (10 components per call: the batched synthesis sweeps) puts only the bins +-m mod nphi on
    every ring, with the phase of the coefficient; m up to 3 nside + 1 (m >= nphi on the polar rings)."""
    import heracles_amd as hx

    rng = np.random.default_rng(31 * nside + cap + spin)
    lmax = 3 * nside + 1
    ms = sorted({0, 1, 2, 3, 4, 5, nside - 1, nside, nside + 1, 2 * nside, lmax - 1, lmax})
    lm = [(min(m + d, lmax), m) for m in ms for d in (0, 7)]
    coeffs = _coeffs(lm, spin, rng)
    with _LdsCap(cap):
        plan = hx.Plan(nside, lmax)
    try:
        per = 10 if spin == 0 else 5
        for q in range(0, len(coeffs), per):
            _synth_check(plan, nside, lmax, spin, coeffs[q : q + per], range(2 * nside), cap, (nside, cap, q))
    finally:
        plan.close()


@pytest.mark.parametrize("spin", [0, 2])
def test_synthesis_spectral_purity_fullsize(spin):
    """nside 4096 / lmax 6144: every residue of m mod 4, both sides of the 64-entry phase-table boundary, m >= nphi on the polar
    rings; l = m and min(m + 40, lmax); a sample of ring pairs (the first polar rings, where high orders are pruned, the cap / belt
    boundary, the equator, and every 512th)."""
    import heracles_amd as hx

    nside, lmax = 4096, 6144
    rng = np.random.default_rng(6144 + spin)
    ms = [0, 1, 2, 3, 5, 63, 64, 65, 255, 256, 1023, 2047, 2048, 4095, 4096, 4097, 6143, 6144]
    lm = sorted({(min(m + d, lmax), m) for m in ms for d in (0, 40)}, key=lambda t: (t[1], t[0]))
    coeffs = _coeffs(lm, spin, rng)
    rps = sorted({0, 1, 2, 3, 7, 15, 16, 31, 63, 64, 65, 255, 1023, 1024, 1536, 2047, 4094, 4095, 4096, 4097, 8190, 8191}
                 | set(range(0, 2 * nside, 512)))
    plan = hx.get_plan(nside, lmax)
    per = 10 if spin == 0 else 5
    for q in range(0, len(coeffs), per):
        _synth_check(plan, nside, lmax, spin, coeffs[q : q + per], rps, 8192, ("4096", q))


# ---- the Jacobi residual pass of map2alm(niter) ----
def _apply_fl(a, fl, lmax):
    out = a.clone()
    for m in range(lmax + 1):
        s = idx(lmax, m, m)
        out[..., s : s + lmax + 1 - m] *= fl[m:]
    return out


@pytest.mark.parametrize("nside,lmax,spin,ncomp", [(64, 128, 0, 3), (64, 128, 2, 4), (4096, 6144, 0, 10), (4096, 6144, 2, 4)])
def test_jacobi_residual_identity(nside, lmax, spin, ncomp):
    """map2alm(x, niter) = the same iteration written out: a0 = map2alm(x); a_{k+1} = a_k + map2alm(x - alm2map(a_k)), the same pixel
    and ring weights on both sides, fl once at the end.  Rounding only: 1e-13 of max|a|, normwise.  nside 4096 with 10 spin-0 maps
    and 4 spin-2 components is the shape of the bench's niter-3 leg."""
    import torch

    import heracles_amd as hx

    npix = 12 * nside**2
    g = torch.Generator(device="cuda").manual_seed(nside + spin)
    x = torch.randn((ncomp, npix), dtype=torch.float64, device="cuda", generator=g)
    pw = 1.0 + 0.1 * torch.rand(npix, dtype=torch.float64, device="cuda", generator=g)
    rw = 1.0 + 0.1 * torch.rand(2 * nside, dtype=torch.float64, device="cuda", generator=g)
    fl = torch.rand(lmax + 1, dtype=torch.float64, device="cuda", generator=g) + 0.5
    plan = hx.get_plan(nside, lmax)
    a0 = plan.map2alm(x, spin, pix_weights=pw, ring_weights=rw)
    got1 = plan.map2alm(x, spin, pix_weights=pw, ring_weights=rw, niter=1)
    want1 = a0 + plan.map2alm(x - plan.alm2map(a0, spin), spin, pix_weights=pw, ring_weights=rw)
    scale = want1.abs().max().item()
    assert (got1 - want1).abs().max().item() <= 1e-13 * scale
    a = a0
    for _ in range(3):
        a = a + plan.map2alm(x - plan.alm2map(a, spin), spin, pix_weights=pw, ring_weights=rw)
    want3 = _apply_fl(a, fl, lmax)
    got3 = plan.map2alm(x, spin, pix_weights=pw, ring_weights=rw, niter=3, fl=fl)
    assert (got3 - want3).abs().max().item() <= 1e-13 * want3.abs().max().item()
