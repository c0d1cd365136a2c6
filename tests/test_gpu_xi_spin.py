"""Cl <-> xi for fields of any spin weight: hx_cl2corr_cols_spin / hx_corr2cl_cols_spin (columns tied to a pair (a, b): k_xi_fwd /
k_xi_back against the pair tables) and ``exact_spin`` of cl2corr / corr2cl / naturalspice / naturalspice_batch.

1. columns against the long-double truth of tests/xi_spin_reference.py, per column
       forward  |xi - truth| <= (16 eps + 1e-13) sum_l |(2l + 1) / 4 pi a_l|,      back  |b - truth| <= (16 eps + 1e-13) 2 pi sum_k w_k |xi_k|
   (the rounding floor of corr_reference.cl2corr_floor plus the 1e-13 at which tests/test_gpu_mixmat_spin.py pins the tables), the truth
   at the nodes x + xlo the tables are built at;
2. the edges: nl <= l0, lmax < l0, a pair beyond HX_MAX_MIX_SPIN, more pairs than HX_XI_TABLES, batch independence;
3. agreement with the mixing matrices, an independently written kernel: corr2cl(cl2corr(e_l2) xi_W)[l1] = G[l1, l2] to 1e-12 max |G|;
4. NaturalSpice undoes pseudo-spectra formed explicitly from the mixing matrices, to 1e-11 max |C|;
5. the round trip at lmax 4096 beside the family path's.
Nothing here is fitted to what the GPU returned."""

import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import corr_reference as cr
import xi_spin_reference as xr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(1, 0), (1, 1), (1, -1), (3, 1), (3, -1), (3, 3), (2, 1), (5, -2), (0, 0), (2, 2), (2, -2), (2, 0)]
NL_CUT = {5: 3, 63: 61, 64: 50, 130: 77}  # a second nl per lmax, none a multiple of 16


def _hx():
    import heracles_amd as hx
    from heracles_amd import _lib, transforms as tr

    _lib.ensure_init()
    return hx, _lib, tr, _lib.load()


def _nodes_dd(n):
    """(x, w, x + xlo in long double): the nodes the pair tables are built at."""
    hx, _lib, tr, L = _hx()
    x, w, xlo = np.empty(n), np.empty(n), np.empty(n)
    _lib.check(L.hx_gauss_legendre_dd(n, _lib.ptr(x), _lib.ptr(w), _lib.ptr(xlo)))
    x0, w0 = hx.gauss_legendre(n)
    assert (x == x0).all() and (w == w0).all()  # (the family path's nodes and weights, bit for bit)
    return x, w, x.astype(cr.LD) + xlo.astype(cr.LD)


@functools.lru_cache(maxsize=None)
def _case(lmax):
    """65 columns at lmax, pairs mixed through the batch (column c: PAIRS[c % 12]; white, red and single-l probes by c // 12), their
    truth forward at both nl, correlation columns (white noise, or the truth of the column) and their truth back.  Computed once per
    lmax and left unchanged."""
    rng = np.random.default_rng(1000 + lmax)
    n, ncol = lmax + 1, 65
    x, w, xld = _nodes_dd(n)
    tabs = xr.Tables(lmax, xld, w)
    pairs = [PAIRS[c % len(PAIRS)] for c in range(ncol)]
    a = np.empty((ncol, n))
    for c in range(ncol):
        kind = (c // len(PAIRS)) % 3
        if kind == 0:
            a[c] = cr.white_spectra(rng, lmax)[0, :, 0]
        elif kind == 1:
            a[c] = cr.red_spectra(rng, lmax)[0, :, 0]
        else:
            a[c] = 0.0
            a[c, int(rng.integers(0, n))] = 1.0
    out = dict(w=w, pairs=pairs, a=a, fwd={}, back={})
    for nl in (n, NL_CUT[lmax]):
        out["fwd"][nl] = tabs.forward(a[:, :nl], pairs)
    xi = np.where((np.arange(ncol) % 2 == 0)[:, None], rng.standard_normal((ncol, n)), out["fwd"][n].astype(np.float64))
    out["xi"] = xi
    for nl in (n, NL_CUT[lmax]):
        out["back"][nl] = tabs.back(xi, pairs, nl)
    for v in (a, xi):
        v.flags.writeable = False
    return out


@pytest.mark.parametrize("ncol", [1, 65])
@pytest.mark.parametrize("lmax", [5, 63, 64, 130])
def test_columns_against_truth(lmax, ncol):
    hx, _lib, tr, L = _hx()
    case, n = _case(lmax), lmax + 1
    pairs = np.array(case["pairs"], dtype=np.int32)
    batches = [np.arange(65)] if ncol == 65 else [np.array([c]) for c in range(len(PAIRS))]  # alone: every pair once
    failures = []
    for nl in (n, NL_CUT[lmax]):
        for sel in batches:
            a, xi = np.ascontiguousarray(case["a"][sel, :nl]), np.ascontiguousarray(case["xi"][sel])
            got_xi = tr.cl2corr_columns(a, pairs[sel], lmax)
            got_b = tr.corr2cl_columns(xi, pairs[sel], lmax, nl=nl)
            assert got_xi.shape == (len(sel), n) and got_b.shape == (len(sel), nl)
            e_f = np.abs(got_xi - case["fwd"][nl][sel]).max(axis=1).astype(np.float64)
            e_b = np.abs(got_b - case["back"][nl][sel]).max(axis=1).astype(np.float64)
            b_f, b_b = xr.forward_bound(a, pairs[sel].tolist()), xr.back_bound(xi, case["w"])
            for i, c in enumerate(sel):
                p = tuple(pairs[c])
                print(f"lmax {lmax} nl {nl} ncol {len(sel)} column {c} {p}: forward {e_f[i]:.2e} (bound {b_f[i]:.2e}) back {e_b[i]:.2e} (bound {b_b[i]:.2e})")
                if not e_f[i] <= b_f[i]:
                    failures.append(f"forward nl {nl} column {c} {p}: {e_f[i]:.3e} > {b_f[i]:.3e}")
                if not e_b[i] <= b_b[i]:
                    failures.append(f"back nl {nl} column {c} {p}: {e_b[i]:.3e} > {b_b[i]:.3e}")
                assert (got_b[i, : max(abs(p[0]), abs(p[1]))] == 0).all()
    assert not failures, "\n".join(failures)


def test_pair_sign_follows_the_order_of_the_pair():
    """(1,2) and (2,1) share a table and differ by (-1)^{a-b}: xi changes its sign, bit for bit; there and back does not."""
    hx, _lib, tr, L = _hx()
    lmax = 40
    a = cr.red_spectra(np.random.default_rng(2), lmax, 2)[:, :, 0]
    p21, p12 = np.array([[2, 1]] * 2, dtype=np.int32), np.array([[1, 2]] * 2, dtype=np.int32)
    xi = tr.cl2corr_columns(a, p21, lmax)
    np.testing.assert_array_equal(tr.cl2corr_columns(a, p12, lmax), -xi)
    np.testing.assert_array_equal(tr.cl2corr_columns(a, np.array([[-1, -2]] * 2, dtype=np.int32), lmax), xi)
    np.testing.assert_array_equal(tr.corr2cl_columns(-xi, p12, lmax), tr.corr2cl_columns(xi, p21, lmax))
    x, w = hx.gauss_legendre(lmax + 1)
    d = hx.wigner_d_table(lmax, 1, 2, x)  # (n, lmax + 1) at the rounded nodes: the sign and the values to the tables' 1e-13
    unit = np.zeros((1, lmax + 1))
    unit[0, 7] = 4 * np.pi / 15
    assert np.abs(tr.cl2corr_columns(unit, p12[:1], lmax)[0] - d[:, 7]).max() < 2e-13


# ---- 2. edges -------------------------------------------------------------------------------------------------------------------------
def test_nothing_above_the_band_gives_zeros():
    hx, _lib, tr, L = _hx()
    rng = np.random.default_rng(3)
    # nl <= l0: pair (3,1) with two multipoles
    p = np.array([[3, 1], [0, 0]], dtype=np.int32)
    xi = tr.cl2corr_columns(rng.standard_normal((2, 2)), p, 20)
    assert (xi[0] == 0).all() and (xi[1] != 0).any()
    b = tr.corr2cl_columns(rng.standard_normal((2, 21)), p, 20, nl=2)
    assert b.shape == (2, 2) and (b[0] == 0).all() and (b[1] != 0).all()
    # nl = l0 + 1: the one live multipole
    b = tr.corr2cl_columns(rng.standard_normal((1, 21)), p[:1], 20, nl=4)
    assert (b[0, :3] == 0).all() and b[0, 3] != 0
    # lmax < l0: pair (3,3) at lmax 2, no error; inputs below l0 are not read (nan in, zeros out)
    p = np.array([[3, 3]], dtype=np.int32)
    assert (tr.cl2corr_columns(np.full((1, 3), np.nan), p, 2) == 0).all()
    assert (tr.corr2cl_columns(rng.standard_normal((1, 3)), p, 2) == 0).all()
    a = rng.standard_normal((1, 12))
    nan_below = np.array(a)
    nan_below[0, :3] = np.nan
    np.testing.assert_array_equal(tr.cl2corr_columns(nan_below, p, 11), tr.cl2corr_columns(a, p, 11))


def test_pair_beyond_the_supported_spin_raises():
    hx, _lib, tr, L = _hx()
    a = np.ones((2, 40))
    for bad in ((33, 0), (0, -33), (2, 33)):
        for fn in (tr.cl2corr_columns, tr.corr2cl_columns):
            with pytest.raises(hx.HxError) as e:
                fn(a, np.array([[1, 1], bad], dtype=np.int32), 39)
            assert e.value.code == _lib.HX_ERR_UNSUPPORTED
    assert np.isfinite(tr.cl2corr_columns(a, np.array([[32, -32], [32, 0]], dtype=np.int32), 39)).all()
    # the arguments of the family entry points are checked the same way
    src, dst, p = np.ones((1, 9)), np.full((1, 9), 777.0), np.zeros((1, 2), dtype=np.int32)
    P = _lib.ptr
    for fn in (L.hx_cl2corr_cols_spin, L.hx_corr2cl_cols_spin):
        for args in ((-1, 9, 1, P(p), P(src), P(dst)), (8, 0, 1, P(p), P(src), P(dst)), (8, 10, 1, P(p), P(src), P(dst)), (8, 9, 0, P(p), P(src), P(dst)),
                     (8, 9, 1, None, P(src), P(dst)), (8, 9, 1, P(p), None, P(dst)), (8, 9, 1, P(p), P(src), None)):
            assert fn(*args) == _lib.HX_ERR_ARG
            assert (dst == 777.0).all()


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from heracles_amd import transforms as tr
d = np.load(sys.argv[2])
xi = tr.cl2corr_columns(d["a"], d["pairs"], int(d["lmax"]))
b = tr.corr2cl_columns(d["xi"], d["pairs"], int(d["lmax"]), nl=int(d["nl"]))
again = tr.cl2corr_columns(d["a"], d["pairs"], int(d["lmax"]))
np.savez(sys.argv[3], xi=xi, b=b, again=again)
"""


def test_more_pairs_than_tables(tmp_path):
    """HX_XI_TABLES is read at first use, so a child process runs with 2: a batch of twelve distinct pairs (twelve tables, dropped and
    rebuilt within the call and between calls) gives the bits the default gives here."""
    hx, _lib, tr, L = _hx()
    lmax, nl = 70, 59
    rng = np.random.default_rng(4)
    pairs = np.array([PAIRS[c % len(PAIRS)] for c in range(29)], dtype=np.int32)
    a, xi = cr.white_spectra(rng, lmax, 29)[:, :, 0], rng.standard_normal((29, lmax + 1))
    np.savez(tmp_path / "in.npz", a=a, xi=xi, pairs=pairs, lmax=lmax, nl=nl)
    env = dict(os.environ, HX_XI_TABLES="2")
    run = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = np.load(tmp_path / "out.npz")
    np.testing.assert_array_equal(out["xi"], tr.cl2corr_columns(a, pairs, lmax))
    np.testing.assert_array_equal(out["again"], out["xi"])
    np.testing.assert_array_equal(out["b"], tr.corr2cl_columns(xi, pairs, lmax, nl=nl))


def test_batch_independence_residence_repeatability():
    """As tests/test_gpu_xi_columns.py::test_batch_independence_residence_repeatability, for pair columns: a column alone is bitwise the
    column at positions 0, 15, 16 and 36 of a 37-column batch of mixed pairs; CUDA tensors in and out give the bits numpy arrays give and
    leave the input untouched; two runs agree bitwise, also across hx_release_caches."""
    import torch

    hx, _lib, tr, L = _hx()
    lmax, ncol = 300, 37
    n = lmax + 1
    rng = np.random.default_rng(9)
    base_pairs = np.array([PAIRS[(7 * c + 1) % len(PAIRS)] for c in range(ncol)], dtype=np.int32)
    for fn in (tr.cl2corr_columns, tr.corr2cl_columns):
        base = np.concatenate([cr.red_spectra(rng, lmax, 19)[:, :, 1], cr.white_spectra(rng, lmax, 18)[:, :, 2]])
        for p in ((1, 0), (3, -1), (1, 2), (2, 2)):
            col = cr.white_spectra(rng, lmax, 1)[:, :, 0]
            alone = fn(col, np.array([p], dtype=np.int32), lmax)
            assert alone.shape == (1, n)
            for pos in (0, 15, 16, 36):
                batch, pairs = np.array(base), np.array(base_pairs)
                batch[pos], pairs[pos] = col[0], p
                np.testing.assert_array_equal(fn(batch, pairs, lmax)[pos], alone[0], err_msg=f"{fn.__name__} pair {p} at position {pos}")
        first = fn(base, base_pairs, lmax)
        np.testing.assert_array_equal(fn(base, base_pairs, lmax), first)
        tin = torch.from_numpy(base).cuda()
        keep = tin.clone()
        tout = fn(tin, base_pairs, lmax)
        assert tout.is_cuda and tout.dtype == torch.float64 and tuple(tout.shape) == first.shape
        np.testing.assert_array_equal(tout.cpu().numpy(), first)
        given = torch.full_like(tout, float("nan"))
        assert fn(tin, base_pairs, lmax, out=given) is given
        np.testing.assert_array_equal(given.cpu().numpy(), first)
        assert torch.equal(tin, keep)
        hx.release_caches()
        np.testing.assert_array_equal(fn(base, base_pairs, lmax), first)
    # the family entry points beside them do not move: the same bits before and after the pair tables were in use
    fam = (np.arange(ncol, dtype=np.int32) * 7 + 1) % 4
    before = tr.cl2corr_columns(base, fam, lmax)
    tr.cl2corr_columns(base, base_pairs, lmax)
    np.testing.assert_array_equal(tr.cl2corr_columns(base, fam, lmax), before)
    hx.release_caches()


# ---- 3. agreement with the mixing matrices ----------------------------------------------------------------------------------------
def test_agreement_with_the_mixing_matrices():
    """G^{(ab)}[l1, l2] = (2 l2 + 1) / 2 sum_k w_k xi_W(x_k) d^{l1}_{ab}(x_k) d^{l2}_{ab}(x_k) is what a unit spectrum e_{l2} gives when it
    goes forward on the pair, is multiplied by the mask's correlation function and comes back: exact at N = lmax = 64 for
    l1, l2, l3 <= 32 (l1 + l2 + l3 <= 96 <= 2 N + 1).  The matrices come from k_mixmat_gemm_dma on tables and nodes of their own."""
    hx, _lib, tr, L = _hx()
    N, lt = 64, 32
    rng = np.random.default_rng(11)
    W = rng.uniform(0.5, 1.5, lt + 1) * rng.choice([-1.0, 1.0], lt + 1)
    W[0] = 4.0
    xi_w = tr.cl2corr_columns(W[None], np.zeros((1, 2), dtype=np.int32), N)[0]
    unit = np.eye(lt + 1)
    failures = []

    def check(pair, G):
        xi = tr.cl2corr_columns(unit, np.array([pair] * (lt + 1), dtype=np.int32), N)
        got = tr.corr2cl_columns(np.ascontiguousarray(xi * xi_w), np.array([pair] * (lt + 1), dtype=np.int32), N, nl=lt + 1)  # [l2][l1]
        err = np.abs(got.T - G).max()
        print(f"pair {pair}: max |d| {err:.2e}, max |G| {np.abs(G).max():.2e}")
        if not err <= 1e-12 * np.abs(G).max():
            failures.append(f"{pair}: {err:.3e} > 1e-12 * {np.abs(G).max():.3e}")

    for s in (1, 3):
        check((s, 0), hx.mixmat(W, lt, lt, lt, spin=(s, 0)))
    for s1, s2 in ((1, 1), (2, 1), (3, 1), (3, 3)):
        eb = hx.mixmat_eb(W, lt, lt, lt, spin=(s1, s2))
        check((s1, s2), eb[0] + eb[1])
        check((s1, -s2), eb[2])
    assert not failures, "\n".join(failures)


# ---- 4. NaturalSpice recovers the spectra -----------------------------------------------------------------------------------------
FIELDS = {"POS": types.SimpleNamespace(mask="W", spin=0), "DEF": types.SimpleNamespace(mask="W", spin=1),
          "SHE": types.SimpleNamespace(mask="W", spin=2), "FLX": types.SimpleNamespace(mask="W", spin=3)}
SPINS = {("POS", "DEF", 0, 0): (0, 1), ("DEF", "DEF", 0, 0): (1, 1), ("DEF", "SHE", 0, 0): (1, 2), ("FLX", "FLX", 0, 0): (3, 3),
         ("POS", "POS", 0, 0): (0, 0), ("SHE", "SHE", 0, 0): (2, 2)}
MKEY = ("W", "W", 0, 0)
NM, ND = 64, 41  # multipoles of the mask and of the pseudo-spectra; of the true spectra


@functools.lru_cache(maxsize=None)
def _mask_and_matrices():
    """W_l of xi_W(x) = 0.6 + 0.4 ((1 + x) / 2)^8 by quadrature (a polynomial of degree 8: band limit 8, exact), zero-padded to 64
    multipoles, and the matrices of every pair of spins in SPINS (l1max 63, l2max 40, l3max 8)."""
    hx, _lib, tr, L = _hx()
    x, w = np.polynomial.legendre.leggauss(16)
    xi_w = 0.6 + 0.4 * ((1 + x) / 2) ** 8
    W = np.zeros(NM)
    W[:9] = 2 * np.pi * (np.polynomial.legendre.legvander(x, 8) * (w * xi_w)[:, None]).sum(axis=0)
    G = {}
    for s1, s2 in set(SPINS.values()):
        if s1 and s2:
            eb = hx.mixmat_eb(W[:9], NM - 1, ND - 1, 8, spin=(s1, s2))
            G[(s1, s2)] = (eb[0] + eb[1], np.array(eb[2]))  # G^{(s1,s2)}, G^{(s1,-s2)}
        else:
            G[(s1, s2)] = hx.mixmat(W[:9], NM - 1, ND - 1, 8, spin=(s1, s2))
    return W, G


def _truth_and_pseudo(rng, scale=1.0):
    import heracles_amd as hx

    W, G = _mask_and_matrices()
    truth, pseudo = {}, {}
    for k, s in SPINS.items():
        s1, s2 = s
        red = scale / (1.0 + np.arange(ND)) ** 2
        red[: max(s)] = 0.0  # (a spectrum of spins (s1, s2) starts at l = max(s1, s2))
        if s1 and s2:
            c = rng.standard_normal((2, 2, ND)) * red
            gp, gm = G[s]
            ee_p_bb, ee_m_bb = gp @ (c[0, 0] + c[1, 1]), gm @ (c[0, 0] - c[1, 1])
            be_m_eb, eb_p_be = gp @ (c[1, 0] - c[0, 1]), gm @ (c[0, 1] + c[1, 0])
            p = np.array([[(ee_p_bb + ee_m_bb) / 2, (eb_p_be - be_m_eb) / 2], [(eb_p_be + be_m_eb) / 2, (ee_p_bb - ee_m_bb) / 2]])
        elif s1 or s2:
            c = rng.standard_normal((2, ND)) * red
            p = np.array([G[s] @ c[0], G[s] @ c[1]])
        else:
            c = rng.standard_normal(ND) * red
            p = G[s] @ c
        truth[k] = np.concatenate([c, np.zeros(c.shape[:-1] + (NM - ND,))], axis=-1)
        pseudo[k] = hx.Result(p, spin=s, axis=-1, ell=np.arange(NM))
    return truth, pseudo


def _mask():
    import heracles_amd as hx

    return {MKEY: hx.Result(np.array(_mask_and_matrices()[0]), spin=(0, 0), axis=-1, ell=np.arange(NM))}


def test_naturalspice_recovers_the_spectra():
    """xi_W >= 0.6, so every damping factor is exactly 1 in double (1 + exp(-50 (log10 0.6 + 5)) = 1), whatever the count.
    1e-11 max |C|: two orders above the 1e-13 at which tables and matrices are each pinned; the division by >= 0.6 and two 64-term sums
    lie between."""
    from heracles_amd import unmixing as um

    rng = np.random.default_rng(21)
    sets = [_truth_and_pseudo(rng, scale) for scale in (1.0, 2.5, 0.3)]
    single = [um.naturalspice(p, _mask(), FIELDS, exact_spin=True) for _, p in sets]
    batch = um.naturalspice_batch({i: p for i, (_, p) in enumerate(sets)}, _mask(), FIELDS, exact_spin=True)
    old_single = um.naturalspice(sets[0][1], _mask(), FIELDS)
    old_batch = um.naturalspice_batch({0: sets[0][1]}, _mask(), FIELDS)
    failures = []
    for i, (truth, pseudo) in enumerate(sets):
        assert list(single[i]) == list(SPINS) == list(batch[i])
        for k, s in SPINS.items():
            c = truth[k]
            top = np.abs(c).max()
            e_s, e_b = np.abs(single[i][k].array - c).max(), np.abs(batch[i][k].array - c).max()
            e_sb = np.abs(single[i][k].array - batch[i][k].array).max()
            print(f"sample {i} spins {s}: single {e_s / top:.2e} batch {e_b / top:.2e} single - batch {e_sb / top:.2e} (of max |C|)")
            assert single[i][k].array.shape == c.shape == batch[i][k].array.shape and single[i][k].spin == s
            if not (e_s <= 1e-11 * top and e_b <= 1e-11 * top):
                failures.append(f"sample {i} {s}: {e_s / top:.3e}, {e_b / top:.3e} > 1e-11")
            if not e_sb <= 1e-13 * top:
                failures.append(f"sample {i} {s}: single - batch {e_sb / top:.3e} > 1e-13")
    assert not failures, "\n".join(failures)
    # the keys of spins {0, 2} do not change a bit with the keyword
    for k in (("POS", "POS", 0, 0), ("SHE", "SHE", 0, 0)):
        np.testing.assert_array_equal(single[0][k].array, old_single[k].array)
        np.testing.assert_array_equal(batch[0][k].array, old_batch[0][k].array)
    # what the feature is for: "like spin 2" misses the (1,1) spectra
    k11 = ("DEF", "DEF", 0, 0)
    top = np.abs(sets[0][0][k11]).max()
    for old in (old_single, old_batch[0]):
        miss = np.abs(old[k11].array - sets[0][0][k11]).max()
        print(f"(1,1) like spin 2: {miss / top:.2e} of max |C|")
        assert miss > 1e-3 * top


def test_dict_drivers_with_exact_spin():
    """cl2corr / corr2cl(exact_spin=True): the columns of a key on its pairs, placed as the spin-2 cases are; shapes, ell and dtype as
    without the keyword; keys of spins {0, 2} bit for bit; there and back is the identity from l0 on."""
    import heracles_amd as hx
    from heracles_amd import transforms as tr

    rng = np.random.default_rng(22)
    _, pseudo = _truth_and_pseudo(rng)
    wd, old = tr.cl2corr(pseudo, exact_spin=True), tr.cl2corr(pseudo)
    x, _ = hx.gauss_legendre(NM)
    for k, s in SPINS.items():
        a = np.asarray(pseudo[k].array)
        assert wd[k].array.shape == a.shape and wd[k].array.dtype == a.dtype and wd[k].spin == s
        np.testing.assert_array_equal(wd[k].ell, x)
        cols = np.asarray(wd[k].array).reshape(-1, NM)
        pairs = np.array(tr.spin_pairs(s), dtype=np.int32)
        if set(s) <= {0, 2}:
            np.testing.assert_array_equal(wd[k].array, old[k].array)
        else:
            packed = a[None] if a.ndim == 1 else np.stack([a[0] + a[1], a[0] - a[1]]) if a.ndim == 2 else \
                np.stack([a[0, 0] + a[1, 1], a[1, 0] - a[0, 1], -a[0, 1] - a[1, 0], a[0, 0] - a[1, 1]])
            np.testing.assert_array_equal(cols, tr.cl2corr_columns(packed, pairs, NM - 1))
    back = tr.corr2cl(wd, exact_spin=True)
    for k, s in SPINS.items():
        a, l0 = np.asarray(pseudo[k].array), max(s)
        assert (np.asarray(back[k].array)[..., :l0] == 0).all()
        assert np.abs(np.asarray(back[k].array) - a)[..., l0:].max() <= 1e-12 * np.abs(a).max()
        np.testing.assert_array_equal(back[k].ell, np.arange(NM))


# ---- 5. at size ---------------------------------------------------------------------------------------------------------------------
def test_round_trip_at_lmax_4096_beside_the_family_path():
    """max |corr2cl_columns(cl2corr_columns(a)) - a| from l0 on, eight white columns, one launch each way per table.  The quadrature is
    exact (degree 2 lmax at lmax + 1 nodes), so what is left is the rounding of tables, nodes, weights and sums.  The pair path may be at
    most 4 x the family path's worst column in the same run (other weights have other pole behaviour)."""
    hx, _lib, tr, L = _hx()
    lmax = 4096
    rng = np.random.default_rng(4096)
    a = np.ascontiguousarray(cr.white_spectra(rng, lmax, 8)[:, :, 0])
    fam = np.array([0, 1, 2, 3, 0, 1, 2, 3], dtype=np.int32)
    pairs = np.array([(1, 1), (3, -1), (2, 2), (2, -2), (2, 0), (0, 0), (1, 1), (3, -1)], dtype=np.int32)

    def worst(tables, l0):
        back = tr.corr2cl_columns(tr.cl2corr_columns(a, tables, lmax), tables, lmax)
        return [float(np.abs(back[c, l0[c]:] - a[c, l0[c]:]).max()) for c in range(8)]

    e_fam = worst(fam, [0 if f == 0 else 2 for f in fam])
    e_pair = worst(pairs, [max(abs(p), abs(q)) for p, q in pairs])
    hx.release_caches()
    print("family path, families 0..3 twice:", " ".join(f"{e:.2e}" for e in e_fam))
    print("pair path", [tuple(p) for p in pairs.tolist()], ":", " ".join(f"{e:.2e}" for e in e_pair))
    assert max(e_pair) <= 4 * max(e_fam), (max(e_pair), max(e_fam))
