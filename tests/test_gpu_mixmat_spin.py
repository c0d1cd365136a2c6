"""Mixing matrices for fields of any spin weight: the Wigner-d tables from the general seed, ``mixmat`` for (s, 0) / (0, s),
``mixmat_eb`` for any two non-zero spins, the context with its table cache (binned rows, eviction), the old and new C entry points,
and the way on through ``invert_mixing_matrix`` / ``apply_mixing_matrix``.

The matrices are defined by the quadrature form G^{(ab)} of hx_mixmat.hip, which is (-1)^{s1+s2} times the bare product of 3j
symbols the oracle sums (pinned for these spins by tests/test_oracle_spin_3j.py): the full-sky tests below fix that sign."""

import ctypes
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NODES = np.array([-0.999, -0.93, -0.2, 0.0, 0.31, 0.9, 0.9985, 0.99995])
OLD_PAIRS = [(0, 0), (2, 0), (2, 2), (2, -2), (1, 1), (-1, 1), (1, -1)]


def wigner_d_exact(lmax, a, b, x, digits=50):
    """d^l_{ab}(x), l = 0 .. lmax, by Wigner's explicit finite sum in mpmath, good to ``digits`` digits of the largest term's size
    relative to 1: the terms of the alternating sum reach ~2^l, so the working precision is ``digits`` plus their decimal exponent.
    In the sign convention of the tables (d^1_{10} = +sin(theta) / sqrt 2):
      d^l_{ab} = sum_k (-1)^k sqrt((l+a)! (l-a)! (l+b)! (l-b)!) / ((l+b-k)! k! (l-k-a)! (k+a-b)!) c^{2l-2k+b-a} s^{2k+a-b},
    c = cos(theta / 2), s = sin(theta / 2).  Consecutive terms differ by a rational factor times (s / c)^2."""
    import mpmath as mp

    out = np.zeros(lmax + 1)
    with mp.workdps(digits + int(0.302 * lmax) + 10):
        xx = mp.mpf(float(x))
        c2, s2 = (1 + xx) / 2, (1 - xx) / 2
        c, s, t = mp.sqrt(c2), mp.sqrt(s2), s2 / c2
        for l in range(max(abs(a), abs(b)), lmax + 1):
            k0, k1 = max(0, b - a), min(l + b, l - a)
            f = mp.factorial
            term = (-1) ** k0 * mp.sqrt(f(l + a) * f(l - a) * f(l + b) * f(l - b)) / (f(l + b - k0) * f(k0) * f(l - k0 - a) * f(k0 + a - b))
            term *= c ** (2 * l - 2 * k0 + b - a) * s ** (2 * k0 + a - b)
            tot = term
            for k in range(k0, k1):
                term = -term * t * ((l + b - k) * (l - k - a)) / ((k + 1) * (k + a - b + 1))
                tot += term
            out[l] = float(tot)
    return out


def _cl(L, seed=None):
    """the mask spectrum of test_gpu_mixmat.py::test_mixmat_vs_3j"""
    rng = np.random.default_rng(L if seed is None else seed)
    return rng.uniform(0.5, 1.5, L + 1) / (1 + np.arange(L + 1)) ** 2


def ref_one(oracle, cl, spin, **kw):
    s = abs(spin[0]) + abs(spin[1])
    return (-1) ** s * oracle.mixmat(cl, spin=spin, **kw)


def ref_three(oracle, cl, spin, **kw):
    s1, s2 = abs(spin[0]), abs(spin[1])
    sg = (-1) ** (s1 + s2)
    p = sg * oracle.mixmat(cl, spin=(s1, s2), **kw)
    q = sg * oracle.mixmat(cl, spin=(s1, -s2), **kw)
    return np.array([(p + q) / 2, (p - q) / 2, q])


def ref_any(oracle, cl, spin, **kw):
    return ref_three(oracle, cl, spin, **kw) if all(spin) else ref_one(oracle, cl, spin, **kw)


def hx_any(cl, spin, **kw):
    import heracles_amd as hx

    return (hx.mixmat_eb if all(spin) else hx.mixmat)(cl, spin=spin, **kw)


# ---- 1. tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ab", [(1, 0), (3, 0), (2, 1), (2, -1), (3, -2), (3, 3), (4, 1), (1, 2)])
def test_wigner_tables_any_pair(ab):
    import heracles_amd as hx

    lmax = 150
    T = hx.wigner_d_table(lmax, ab[0], ab[1], NODES)
    ref = np.array([wigner_d_exact(lmax, ab[0], ab[1], xx) for xx in NODES])
    assert T.shape == ref.shape
    print("max |table - exact|:", np.abs(T - ref).max())
    np.testing.assert_allclose(T, ref, rtol=0, atol=1e-13)
    assert (T[:, : max(abs(ab[0]), abs(ab[1]))] == 0).all()


def test_wigner_tables_old_pairs_from_the_general_seed(monkeypatch):
    """The pairs that keep a seed branch of their own give the same bits when the general seed is forced (HX_WIGNER_SEED=general),
    and a pair beyond the table's lmax or beyond the supported spin is zeros / an error."""
    import heracles_amd as hx

    lmax = 150
    x = np.concatenate([NODES, np.random.default_rng(4).uniform(-1, 1, 200)])
    own = {ab: hx.wigner_d_table(lmax, ab[0], ab[1], x) for ab in OLD_PAIRS}
    monkeypatch.setenv("HX_WIGNER_SEED", "general")
    for ab in OLD_PAIRS:
        np.testing.assert_array_equal(hx.wigner_d_table(lmax, ab[0], ab[1], x), own[ab], err_msg=str(ab))
    monkeypatch.delenv("HX_WIGNER_SEED")
    assert (hx.wigner_d_table(3, 5, 1, NODES) == 0).all()
    with pytest.raises(hx.HxError):
        hx.wigner_d_table(lmax, 33, 0, NODES)
    with pytest.raises(hx.HxError):
        hx.mixmat(_cl(16), spin=(0, 33))


# ---- 2. small matrices against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [16, 40, 130])
def test_mixmat_one_spin_zero_vs_3j(oracle, L):
    import heracles_amd as hx

    cl = _cl(L)
    for s in (1, 3):
        for spin in ((s, 0), (0, s)):
            out = hx.mixmat(cl, spin=spin)
            ref = ref_one(oracle, cl, spin)
            assert out.shape == (L + 1, L + 1)
            np.testing.assert_allclose(out, ref, rtol=0, atol=1e-13 * np.abs(ref).max(), err_msg=str(spin))
        np.testing.assert_array_equal(hx.mixmat(cl, spin=(s, 0)), hx.mixmat(cl, spin=(0, -s)))


@pytest.mark.parametrize("L", [16, 40, 130])
def test_mixmat_eb_any_spins_vs_3j(oracle, L):
    import heracles_amd as hx

    cl = _cl(L)
    got = {}
    for spin in [(1, 1), (1, 2), (2, 1), (3, 2), (3, 3)]:
        out = got[spin] = hx.mixmat_eb(cl, spin=spin)
        ref = ref_three(oracle, cl, spin)
        assert out.shape == (3, L + 1, L + 1)
        np.testing.assert_allclose(out, ref, rtol=0, atol=1e-13 * np.abs(ref).max(), err_msg=str(spin))
        np.testing.assert_allclose(out[2], out[0] - out[1], rtol=0, atol=1e-14)
    np.testing.assert_array_equal(got[1, 2], got[2, 1])
    np.testing.assert_array_equal(hx.mixmat_eb(cl, spin=(-3, 2)), got[3, 2])  # (spins enter by magnitude)


# ---- 3. rectangular and truncated builds --------------------------------------------------------------------------------------------
def test_mixmat_any_spin_shapes(oracle):
    cl = np.random.default_rng(2).uniform(0.5, 1.5, 31)
    for kw in ({"l1max": 10, "l2max": 20}, {"l1max": 20, "l2max": 10}, {"l1max": 5, "l2max": 5, "l3max": 12},
               {"l1max": 150, "l2max": 129}):
        for spin in ((1, 0), (1, 2)):
            out, ref = hx_any(cl, spin, **kw), ref_any(oracle, cl, spin, **kw)
            assert out.shape == ref.shape == ((3,) if all(spin) else ()) + (kw["l1max"] + 1, kw["l2max"] + 1)
            np.testing.assert_allclose(out, ref, rtol=0, atol=1e-13 * np.abs(ref).max(), err_msg=f"{spin} {kw}")


# ---- 4. full sky: the sign convention -----------------------------------------------------------------------------------------------
def _check_identity(M, first, atol):
    ident = np.zeros(M.shape[0])
    ident[first:] = 1.0
    np.testing.assert_allclose(np.diagonal(M), ident, rtol=0, atol=atol)
    off = M.copy()
    np.fill_diagonal(off, 0.0)
    assert np.abs(off).max() <= atol


def test_full_sky_mask_gives_the_identity():
    import heracles_amd as hx

    L = 48
    one = np.zeros(L + 1)
    one[0] = 4 * np.pi
    for s in (1, 2, 3):
        for spin in ((s, 0), (0, s)):
            _check_identity(hx.mixmat(one, spin=spin), s, 1e-13)
    for spin in [(1, 1), (1, 2), (2, 1), (3, 2), (3, 3)]:
        eb = hx.mixmat_eb(one, spin=spin)
        _check_identity(eb[0], max(spin), 1e-13)
        assert np.abs(eb[1]).max() <= 1e-13
        np.testing.assert_allclose(eb[2], eb[0], rtol=0, atol=1e-13)


@pytest.mark.parametrize("spin", [(1, 0), (3, 2)])
def test_full_sky_identity_lmax4096(spin):
    """every row of the new tables and every node of the L = 4096 build (orthogonality of the tables under the nodes); the bound of
    test_gpu_mixmat.py::test_mixmat_eb_full_sky_identity_lmax4096"""
    L = 4096
    one = np.zeros(L + 1)
    one[0] = 4 * np.pi
    M = hx_any(one, spin)
    if all(spin):
        _check_identity(M[0], max(spin), 2e-11)
        assert np.abs(M[1]).max() <= 2e-11
        assert np.abs(M[2] - M[0]).max() <= 2e-11
    else:
        _check_identity(M, max(spin), 2e-11)


# ---- 5. high l ----------------------------------------------------------------------------------------------------------------------
def _mask_spectrum(L):
    ell = np.arange(L + 1)
    # a survey-like mask spectrum: a broad Gaussian core plus a slow power-law tail, so that every l3 up to L contributes
    return 4 * np.pi * 0.35 * np.exp(-ell * (ell + 1) / 3000.0) + 0.2 / (1.0 + ell) ** 1.5


def _blocks(L, first):
    """test_gpu_mixmat.py::_blocks with the low-row block starting at the first row the field has"""
    h = L // 2
    return [((L - 23, L), (L - 200, L)), ((h - 12, h + 11), (h - 100, h + 100)), ((L - 23, L), (h - 100, h + 100)),
            ((h - 12, h + 11), (L - 200, L)), ((first, first + 23), (L - 200, L)), ((0, 23), (0, 200))]


@pytest.mark.parametrize("spin", [(1, 0), (3, 1)])
def test_any_spin_blocks_at_high_l_vs_3j(oracle, spin):
    L = 4096
    wl = _mask_spectrum(L)
    got = hx_any(wl, spin)
    assert got.shape == ((3,) if all(spin) else ()) + (L + 1, L + 1)
    scale = np.abs(got).max()
    sg = (-1) ** (spin[0] + spin[1])
    worst = 0.0
    for rows, cols in _blocks(L, max(spin)):
        p = sg * oracle.mixmat_block(wl, rows, cols, spin=spin)
        assert np.abs(p).max() > 0
        if all(spin):
            q = sg * oracle.mixmat_block(wl, rows, cols, spin=(spin[0], -spin[1]))
            ref = np.array([(p + q) / 2, (p - q) / 2, q])
        else:
            ref = p
        err = np.abs(got[..., rows[0]:rows[1] + 1, cols[0]:cols[1] + 1] - ref).max()
        worst = max(worst, err / scale)
        assert err <= 1e-12 * scale, (spin, rows, cols, err / scale)
    print("worst block error / max|M|:", worst)


# ---- 6. context, binned rows, eviction ----------------------------------------------------------------------------------------------
def _job():
    L = 24
    rng = np.random.default_rng(12)
    cls = {("V", "V", 0, 0): rng.uniform(0.1, 1.0, L + 1) / (1.0 + np.arange(L + 1)) ** 2,
           ("V", "W", 0, 1): rng.uniform(0.1, 1.0, L + 1) / (1.0 + np.arange(L + 1)),
           ("W", "W", 1, 1): rng.uniform(0.1, 1.0, L + 1)}
    flds = {"P": types.SimpleNamespace(mask="V", spin=0), "D": types.SimpleNamespace(mask="W", spin=1),
            "G": types.SimpleNamespace(mask="W", spin=2), "K": types.SimpleNamespace(mask="V", spin=3)}
    return L, cls, flds


def test_mixing_matrices_fields_of_spins_0_to_3(oracle):
    import heracles_amd as hx
    from heracles_amd import twopoint as tp
    from heracles_amd.binning import BinPlan

    L, cls, flds = _job()
    kw = {"l1max": 20, "l2max": 22, "l3max": L}
    mms = hx.mixing_matrices(flds, cls, **kw)
    todo = tp.mixing_requests(flds, cls)
    assert list(mms) == [t for t, _, _ in todo] and len(mms) == 10
    assert {tuple(sorted(sp)) for _, _, sp in todo} >= {(0, 1), (0, 3), (1, 1), (1, 2), (1, 3), (2, 3), (3, 3)}
    full = {}
    for (f1, f2, i1, i2), res in mms.items():
        spin = (flds[f1].spin, flds[f2].spin)
        assert res.spin == spin
        cl = cls[flds[f1].mask, flds[f2].mask, i1, i2]
        full[f1, f2, i1, i2] = got = np.asarray(res.array)
        np.testing.assert_array_equal(got, hx_any(cl, spin, **kw))
        ref = ref_any(oracle, cl, spin, **kw)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13 * np.abs(ref).max(), err_msg=str(spin))
    edges = np.array([2, 5, 9, 14, 21])
    plan = BinPlan(np.arange(21), edges, "2l+1")
    binned = hx.mixing_matrices(flds, cls, bins=edges, weights="2l+1", **kw)
    assert list(binned) == list(mms)
    for key, res in binned.items():
        got, want = np.asarray(res.array), plan.apply(full[key], full[key].ndim - 2)
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14 * np.abs(want).max(), err_msg=str(key))
        assert (got[want == 0] == 0).all(), key
    # a single edge: no bin at all, empty rows of the right shape for every pair of spins
    empty = hx.mixing_matrices(flds, cls, bins=np.array([3]), weights="2l+1", **kw)
    for (f1, f2, _, _), res in empty.items():
        assert np.asarray(res.array).shape == ((3,) if flds[f1].spin and flds[f2].spin else ()) + (0, 23)


def test_context_drops_and_rebuilds_tables(monkeypatch):
    """HX_MIX_TABLES=2: a context that may keep two tables beside (0,0) serves six pairs (ten tables) and then the first again, whose
    tables have been dropped in between, with the same bits; so do its binned rows."""
    import heracles_amd as hx
    from heracles_amd.binning import BinPlan

    L = 24
    cl = _cl(L, seed=5)
    pairs = [(1, 2), (3, 0), (3, 3), (0, 1), (2, 2), (3, 1)]
    monkeypatch.setenv("HX_MIX_TABLES", "2")
    with hx.MixmatContext(20, 22, L) as ctx:
        ctx.set_bins(BinPlan(np.arange(21), np.array([2, 5, 9, 14, 21]), "2l+1"))
        first = [ctx(cl, sp).copy() for sp in pairs]
        np.testing.assert_array_equal(ctx(cl, pairs[0]), first[0])
        firstb = [ctx.binned(cl, sp).copy() for sp in pairs]
        np.testing.assert_array_equal(ctx.binned(cl, pairs[0]), firstb[0])
    monkeypatch.delenv("HX_MIX_TABLES")
    with hx.MixmatContext(20, 22, L) as ctx:  # (the default keeps them all)
        for sp, m in zip(pairs, first):
            np.testing.assert_array_equal(ctx(cl, sp), m, err_msg=str(sp))


def test_context_restages_spectra_of_other_lengths():
    """One context fed a spectrum longer than l3max + 1, then a shorter one, then the first again: the mask spectrum staged inside the
    context is truncated / zero-padded anew every time (no stale tail), and host and device destinations get the same bits, which
    are those of a fresh one-shot build; so are the binned rows of the short spectrum against a fresh context."""
    import torch

    import heracles_amd as hx
    from heracles_amd import _lib
    from heracles_amd.binning import BinPlan

    L = 40
    kw = {"l1max": 20, "l2max": 22, "l3max": L}
    long_, short = _cl(59, seed=21), _cl(11, seed=22)
    assert long_.size == 60 > L + 1 > short.size == 12
    plan = BinPlan(np.arange(21), np.array([2, 5, 9, 14, 21]), "2l+1")
    with hx.MixmatContext(20, 22, L) as ctx, hx.MixmatContext(20, 22, L) as fresh:
        ctx.set_bins(plan)
        fresh.set_bins(plan)
        for spin in [(0, 0), (2, 0), (3, 1)]:
            for cl in (long_, short, long_):
                got = ctx(cl, spin)
                hx.mixmat_release()  # (the one-shot entry points keep a context of their own: drop it, so that this one is fresh)
                np.testing.assert_array_equal(got, hx_any(cl, spin, **kw), err_msg=f"{spin} {cl.size}")
                # the spectrum from device memory takes the other staging path (memset + device copy) in the same context
                src = torch.as_tensor(cl, device="cuda")
                from_dev = np.full(got.shape, np.nan)
                _lib.check(_lib.load().hx_mixctx_apply_spin(ctx._h, _lib.ptr(src), cl.size, spin[0], spin[1], _lib.ptr(from_dev)))
                np.testing.assert_array_equal(from_dev, got, err_msg=f"{spin} {cl.size} device spectrum")
                dev = torch.full(got.shape, float("nan"), dtype=torch.float64, device="cuda")
                assert ctx(cl, spin, out=dev) is dev
                np.testing.assert_array_equal(dev.cpu().numpy(), got, err_msg=f"{spin} {cl.size} device")
                dev.fill_(float("nan"))
                hx_any(cl, spin, out=dev, **kw)
                np.testing.assert_array_equal(dev.cpu().numpy(), got, err_msg=f"{spin} {cl.size} one-shot, device")
            # `fresh` never sees the long spectrum
            np.testing.assert_array_equal(ctx(short, spin), fresh(short, spin), err_msg=str(spin))
            np.testing.assert_array_equal(ctx.binned(short, spin), fresh.binned(short, spin), err_msg=str(spin))


# ---- 7. old and new entry points ----------------------------------------------------------------------------------------------------
def test_old_and_new_entry_points_agree():
    import heracles_amd as hx
    from heracles_amd import _lib

    L = 130
    cl = _cl(L)
    lib = _lib.load()
    hx.init()
    h = lib.hx_mixctx_create(L, L, L)
    assert h
    try:
        for kind, (s1, s2) in ((1, (0, 0)), (2, (2, 0)), (4, (2, 2))):
            shape = ((3,) if kind == 4 else ()) + (L + 1, L + 1)
            old, new = np.full(shape, np.nan), np.full(shape, np.nan)
            _lib.check(lib.hx_mixctx_apply(h, _lib.ptr(cl), L + 1, kind, _lib.ptr(old)))
            _lib.check(lib.hx_mixctx_apply_spin(h, _lib.ptr(cl), L + 1, s1, s2, _lib.ptr(new)))
            np.testing.assert_array_equal(old, new)
            np.testing.assert_array_equal(new, hx_any(cl, (s1, s2)))
    finally:
        lib.hx_mixctx_destroy(ctypes.c_void_p(h))
    old, new = np.full((3, L + 1, L + 1), np.nan), np.full((3, L + 1, L + 1), np.nan)
    _lib.check(lib.hx_mixmat_eb(_lib.ptr(cl), L + 1, L, L, L, _lib.ptr(old)))
    _lib.check(lib.hx_mixmat_eb_spin(_lib.ptr(cl), L + 1, L, L, L, 2, 2, _lib.ptr(new)))
    np.testing.assert_array_equal(old, new)
    assert lib.hx_mixmat_eb_spin(_lib.ptr(cl), L + 1, L, L, L, 2, 0, _lib.ptr(new)) != 0


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------
def test_unmixing_round_trip_for_spin_1_fields():
    """mixing_matrices -> invert_mixing_matrix -> apply_mixing_matrix for a spin-1 field (the README's Deflection) beside a scalar and a
    spin-2 field: M^-1 (M c) = c on l >= the larger spin, to the bound of test_gpu_widen.py's invert / apply test (1e-8 of the largest)."""
    import heracles_amd as hx

    L = 24
    wl = 0.3 * _cl(L, seed=8)
    wl[0] += 4 * np.pi * 0.7
    flds = {"D": types.SimpleNamespace(mask="V", spin=1), "P": types.SimpleNamespace(mask="V", spin=0),
            "G": types.SimpleNamespace(mask="V", spin=2)}
    mms = hx.mixing_matrices(flds, {("V", "V", 0, 0): wl}, l1max=L, l2max=L, l3max=L)
    keys = {("D", "G", 0, 0): (1, 2), ("D", "P", 0, 0): (1, 0)}
    mms = {k: mms[k] for k in keys}
    assert {k: v.spin for k, v in mms.items()} == keys
    rng = np.random.default_rng(3)
    c = {}
    for k, sp in keys.items():
        a = rng.uniform(0.5, 1.5, ((2, 2) if all(sp) else (1,)) + (L + 1,))
        a[..., : max(sp)] = 0.0
        c[k] = hx.Result(a if all(sp) else a[0], spin=sp, axis=-1)
    mixed = hx.apply_mixing_matrix(c, mms)
    back = hx.apply_mixing_matrix(mixed, hx.invert_mixing_matrix(mms))
    for k, sp in keys.items():
        got, want = np.asarray(back[k].array), np.asarray(c[k].array)
        assert np.abs(np.asarray(mixed[k].array) - want).max() > 1e-3  # (the mask does mix)
        np.testing.assert_allclose(got[..., max(sp):], want[..., max(sp):], rtol=0, atol=1e-8 * np.abs(want).max(), err_msg=str(k))
