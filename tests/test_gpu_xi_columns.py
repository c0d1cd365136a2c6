"""hx_cl2corr_cols / hx_corr2cl_cols (k_xi_fwd, k_xi_back: the Cl <-> xi transforms of single columns as FP64 GEMMs against the cached
Wigner tables) and hx_xi_ratio, against the long-double truth of tests/corr_reference.py with the yardstick of
tests/test_gpu_corr_stage.py: per input kind, column and band
    E_gpu = max |gpu - truth|  <=  8 E_ref + floor,   E_ref = max |oracle - truth|,  floor = 16 eps sum |terms|.
A column of family f is compared in the four-column layout of hx_cl2corr (family 0: TT; 1: EE = BB = a / 2; 2: EE = -BB = a / 2;
3: TE), in which truth and oracle are defined.  Nothing here is fitted to what the GPU returned.

Measured on the MI355X: E_gpu / E_ref = 0.99 .. 1.01 in every band at lmax 2048 with 80 columns; the file
takes 15 s, 11 of them the long-double truth of the 2048 x 80 case."""

import ctypes
import functools

import numpy as np
import pytest

import corr_reference as cr

pytestmark = pytest.mark.gpu

NCOLS = (1, 15, 16, 17, 33)
KINDS = ("red", "white", "probes")


def _hx():
    import heracles_amd as hx
    from heracles_amd import _lib, transforms as tr

    _lib.ensure_init()
    return hx, _lib, tr, _lib.load()


def _embed(cols, fam):
    """[ncol][len] columns -> [ncol][len][4]; family 1 as EE = BB = a / 2, family 2 as EE = -BB = a / 2."""
    out = np.zeros(cols.shape + (4,))
    for c, f in enumerate(fam):
        if f == 0 or f == 3:
            out[c, :, f] = cols[c]
        else:
            out[c, :, 1] = cols[c] / 2
            out[c, :, 2] = cols[c] / 2 if f == 1 else -cols[c] / 2
    return out


def _xi_layout(cols, fam):
    """[ncol][n] correlation columns -> [ncol][n][4]: column f of the four-column layout holds the column, the others are zero."""
    out = np.zeros(cols.shape + (4,))
    for c, f in enumerate(fam):
        out[c, :, f] = cols[c]
    return out


def _oracle4(oracle, name, arr, x, w):
    xw = np.concatenate([x, w])
    out = np.empty_like(arr)
    fn = getattr(oracle.lib(), name)
    for s in range(arr.shape[0]):
        fn(ctypes.c_int(arr.shape[1] - 1), oracle._p(np.ascontiguousarray(arr[s])), oracle._p(xw), oracle._p(out[s]))
    return out


def _case(lmax, ncol):
    """The first ncol columns of the 33 computed once per lmax."""
    full = _columns(lmax, max(NCOLS))
    return {k: v if k in ("x", "w") else v[:ncol] for k, v in full.items()}


@functools.lru_cache(maxsize=2)
def _columns(lmax, ncol):
    """Inputs, truth and oracle results of `ncol` columns at lmax, families and kinds mixed through the batch; computed once per
    lmax and left unchanged.  Column c: family c % 4; kind red, white or single-l probe by (c // 4) % 3."""
    from oracle import hxoracle as oracle

    hx, _lib, tr, L = _hx()
    rng = np.random.default_rng(lmax)
    x, w = hx.gauss_legendre(lmax + 1)
    fam = np.arange(ncol, dtype=np.int32) % 4
    kind = [KINDS[(c // 4) % 3] for c in range(ncol)]
    ls = cr.probe_multipoles(rng, lmax, x)
    a = np.empty((ncol, lmax + 1))
    for c in range(ncol):
        ix = int(fam[c])
        if kind[c] == "red":
            a[c] = cr.red_spectra(rng, lmax)[0, :, ix]
        elif kind[c] == "white":
            a[c] = cr.white_spectra(rng, lmax)[0, :, ix]
        else:
            a[c] = cr.probe_spectra(lmax, [ls[int(rng.integers(len(ls)))]])[0, :, 0]
    cls4 = _embed(a, fam)
    truth = cr.cl2corr_truth(cls4, x)
    ref = _oracle4(oracle, "hxo_cl2corr", cls4, x, w)
    # the way back: the truth xi of the column (red, probes) or white noise (white)
    xi = np.stack([rng.standard_normal(lmax + 1) if kind[c] == "white" else truth[c, :, fam[c]].astype(np.float64) for c in range(ncol)])
    xi4 = _xi_layout(xi, fam)
    truth2 = cr.corr2cl_truth(xi4, x, w)
    ref2 = _oracle4(oracle, "hxo_corr2cl", xi4, x, w)
    for v in (a, xi, cls4, xi4, ref, ref2, truth, truth2):
        v.flags.writeable = False
    return dict(x=x, w=w, fam=fam, kind=kind, a=a, cls4=cls4, truth=truth, ref=ref, xi=xi, xi4=xi4, truth2=truth2, ref2=ref2)


def _back_layout(b, fam):
    """[ncol][nl] spectra columns that came back -> (TT, EE, BB, TE): family 1 is EE + BB of (xi+, 0), family 2 EE - BB of (0, xi-)."""
    out = np.zeros(b.shape + (4,))
    for c, f in enumerate(fam):
        if f == 0 or f == 3:
            out[c, :, f] = b[c]
        else:
            out[c, :, 1] = b[c] / 2
            out[c, :, 2] = b[c] / 2 if f == 1 else -b[c] / 2
    return out


def _yardstick(tag, case, got_xi, got_b, lmax):
    failures = []
    bands, lb = cr.node_bands(case["x"]), cr.ell_bands(lmax)
    floor, floor2 = cr.cl2corr_floor(case["cls4"]), cr.corr2cl_floor(case["xi4"], case["w"])
    got4, got24 = _xi_layout(got_xi, case["fam"]), _back_layout(got_b, case["fam"])
    for kind in KINDS:
        specs = [c for c, k in enumerate(case["kind"]) if k == kind]
        if not specs:
            continue
        for name, rows in ((f"cl2corr_cols {tag} {kind}", cr.yardstick(got4, case["ref"], case["truth"], floor, bands, specs)),
                           (f"corr2cl_cols {tag} {kind}", cr.yardstick(got24, case["ref2"], case["truth2"], floor2, lb, specs))):
            print(cr.format_rows(name, rows))
            for ix, band, eg, er, bound in rows:
                if not eg <= bound:
                    failures.append(f"{name} column {ix} band {band}: E_gpu {eg:.3e} > 8 * E_ref {er:.3e} + floor = {bound:.3e}")
    return failures


@pytest.mark.parametrize("lmax,ncol", [(lm, nc) for lm in (0, 1, 2, 3, 62, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512) for nc in NCOLS])
def test_error_against_truth(lmax, ncol):
    """n = lmax + 1 around the 64 x 64 tiles, the 16-multipole blocks of k_xi_fwd and the 16-node blocks of k_xi_back; ncol around the
    16-row blocks of the matrix instruction, one column alone, and two wave rows."""
    hx, _lib, tr, L = _hx()
    case = _case(lmax, ncol)
    got = tr.cl2corr_columns(case["a"], case["fam"], lmax)
    back = tr.corr2cl_columns(case["xi"], case["fam"], lmax)
    assert got.shape == (ncol, lmax + 1) and back.shape == (ncol, lmax + 1)
    if lmax < 2:
        assert (got[case["fam"] > 0] == 0).all() and (back[case["fam"] > 0] == 0).all(), "no polarisation below l = 2"
    else:
        assert (back[case["fam"] > 0][:, :2] == 0).all()
    failures = _yardstick(f"{lmax} x {ncol}", case, got, back, lmax)
    assert not failures, "\n".join(failures)


def test_error_against_truth_past_one_tile_everywhere():
    """lmax 2048 with 80 columns (not a multiple of 16): more than one tile of nodes, multipoles and columns in every family."""
    hx, _lib, tr, L = _hx()
    lmax, ncol = 2048, 80
    case = _columns(lmax, ncol)
    got = tr.cl2corr_columns(case["a"], case["fam"], lmax)
    back = tr.corr2cl_columns(case["xi"], case["fam"], lmax)
    failures = _yardstick(f"{lmax} x {ncol}", case, got, back, lmax)
    hx.release_caches()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("nl", [1, 2, 3, 17, 64, 65, 128])
def test_nl_cut(nl):
    """Forward: nl multipoles give what the column zero-padded to lmax + 1 gives, within the floor of the sum (both are roundings of the
    same exact sum).  Back: the first nl multipoles of the full result within the floor, and nothing is written past [ncol][nl]."""
    import torch

    hx, _lib, tr, L = _hx()
    lmax, ncol = 127, 9
    n = lmax + 1
    rng = np.random.default_rng(nl)
    x, w = hx.gauss_legendre(n)
    fam = np.arange(ncol, dtype=np.int32) % 4
    a = np.concatenate([cr.red_spectra(rng, lmax, 5)[:, :, 0], cr.white_spectra(rng, lmax, 4)[:, :, 0]])
    padded = np.array(a)
    padded[:, nl:] = 0
    cut = tr.cl2corr_columns(np.ascontiguousarray(a[:, :nl]), fam, lmax)
    full = tr.cl2corr_columns(padded, fam, lmax)
    floor = cr.cl2corr_floor(_embed(padded, fam))
    for c, f in enumerate(fam):
        assert np.abs(cut[c] - full[c]).max() <= floor[c, f], (c, f)
    xi = rng.standard_normal((ncol, n))
    bfull = tr.corr2cl_columns(xi, fam, lmax)
    floor2 = cr.corr2cl_floor(_xi_layout(xi, fam), w)
    for dst in (np.full(ncol * n, 777.0), torch.full((ncol * n,), 777.0, dtype=torch.float64, device="cuda")):
        _lib.check(L.hx_corr2cl_cols(lmax, nl, ncol, _lib.ptr(fam), _lib.ptr(xi), _lib.ptr(dst)))
        flat = dst if isinstance(dst, np.ndarray) else dst.cpu().numpy()
        assert (flat[ncol * nl:] == 777.0).all(), "written past [ncol][nl]"
        b = flat[: ncol * nl].reshape(ncol, nl)
        assert not (b == 777.0).any()
        for c, f in enumerate(fam):
            # (the polarisation columns of the floor each take half of both polarisation terms: b = EE +- BB takes twice that)
            assert np.abs(b[c] - bfull[c, :nl]).max() <= (2 * floor2[c, 1] if f in (1, 2) else floor2[c, f]), (c, f)
            if f > 0:
                assert (b[c, :2] == 0).all()


def test_batch_independence_residence_repeatability():
    """A column alone is bitwise the same column at positions 0, 15, 16 and 36 of a 37-column batch (every family, both directions);
    CUDA tensors in and out give the bits numpy arrays give and leave the input untouched; two runs agree bitwise, also across
    hx_release_caches."""
    import torch

    hx, _lib, tr, L = _hx()
    lmax, ncol = 300, 37
    n = lmax + 1
    rng = np.random.default_rng(9)
    base_fam = (np.arange(ncol, dtype=np.int32) * 7 + 1) % 4
    for fn in (tr.cl2corr_columns, tr.corr2cl_columns):
        base = np.concatenate([cr.red_spectra(rng, lmax, 19)[:, :, 1], cr.white_spectra(rng, lmax, 18)[:, :, 2]])
        assert len({r.tobytes() for r in base}) == ncol
        for f in range(4):
            col = cr.white_spectra(rng, lmax, 1)[:, :, 0]
            alone = fn(col, np.array([f], dtype=np.int32), lmax)
            assert alone.shape == (1, n)
            for pos in (0, 15, 16, 36):
                batch, fam = np.array(base), np.array(base_fam)
                batch[pos], fam[pos] = col[0], f
                np.testing.assert_array_equal(fn(batch, fam, lmax)[pos], alone[0], err_msg=f"{fn.__name__} family {f} at position {pos}")
        first = fn(base, base_fam, lmax)
        np.testing.assert_array_equal(fn(base, base_fam, lmax), first)
        tin = torch.from_numpy(base).cuda()
        keep = tin.clone()
        tout = fn(tin, base_fam, lmax)
        assert tout.is_cuda and tout.dtype == torch.float64 and tuple(tout.shape) == first.shape
        np.testing.assert_array_equal(tout.cpu().numpy(), first)
        given = torch.full_like(tout, float("nan"))
        assert fn(tin, base_fam, lmax, out=given) is given
        np.testing.assert_array_equal(given.cpu().numpy(), first)
        assert torch.equal(tin, keep)
        hx.release_caches()
        np.testing.assert_array_equal(fn(base, base_fam, lmax), first)
    hx.release_caches()


def _ratio_numpy(xi_d, xi_num, num_col, ndamp, xi_den, den_col, x0, k):
    from heracles_amd.unmixing import logistic

    out = np.empty_like(xi_d)
    with np.errstate(all="ignore"):
        for c in range(xi_d.shape[0]):
            alpha = np.array(xi_num[num_col[c]])
            if xi_den is not None and den_col[c] >= 0:
                alpha = alpha / xi_den[den_col[c]]
            for _ in range(ndamp[c]):
                alpha *= logistic(np.log10(abs(alpha)), x0=x0, k=k)  # unmixing._damp_in_place
            out[c] = xi_d[c] / alpha
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ratio_against_the_numpy_formulas(n):
    """|alpha| in [1e-8, 1] with both signs, one and two dampings, with and without the second mask.  rtol 1e-12: the exponent's argument
    is at most 400 in magnitude, its ulp 5.7e-14; one ulp of log10 times k = 50 is 9e-14 on the exponential; two dampings compound to
    well under 1e-12."""
    hx, _lib, tr, L = _hx()
    rng = np.random.default_rng(n)
    ncol, nden = 11, 3
    alpha = 10.0 ** rng.uniform(-8, 0, (ncol, n)) * rng.choice([-1.0, 1.0], (ncol, n))
    alpha[0, 0], alpha[1, -1] = 1e-8, -1.0
    xi_d = rng.standard_normal((ncol, n))
    xi_den = 10.0 ** rng.uniform(-1, 1, (nden, n)) * rng.choice([-1.0, 1.0], (nden, n))
    num_col = rng.permutation(ncol).astype(np.int32)
    den_col = rng.integers(-1, nden, ncol).astype(np.int32)
    den_col[0], den_col[1] = -1, nden - 1
    ndamp = (1 + np.arange(ncol) % 2).astype(np.int32)
    xi_num = np.empty((ncol, n))
    xi_num[num_col] = alpha
    xi_num2 = np.empty((ncol, n))  # numerators of the two-mask case: alpha = num / den
    xi_num2[num_col] = np.where((den_col >= 0)[:, None], alpha * xi_den[np.maximum(den_col, 0)], alpha)
    for x0 in (-5.0, -2.3):
        got = tr.xi_ratio(xi_d, xi_num, num_col, ndamp, x0=x0)
        np.testing.assert_allclose(got, _ratio_numpy(xi_d, xi_num, num_col, ndamp, None, None, x0, 50), rtol=1e-12, atol=0)
        got = tr.xi_ratio(xi_d, xi_num2, num_col, ndamp, xi_den=xi_den, den_col=den_col, x0=x0)
        np.testing.assert_allclose(got, _ratio_numpy(xi_d, xi_num2, num_col, ndamp, xi_den, den_col, x0, 50), rtol=1e-12, atol=0)
    # in place, on the device
    import torch

    t = torch.from_numpy(xi_d).cuda()
    assert tr.xi_ratio(t, torch.from_numpy(xi_num).cuda(), num_col, ndamp, x0=-5.0, out=t) is t
    np.testing.assert_array_equal(t.cpu().numpy(), tr.xi_ratio(xi_d, xi_num, num_col, ndamp, x0=-5.0))


def test_ratio_special_values():
    """alpha = 0 (nan), alpha = 1e-300 (an infinite divisor: 0 out) and 0 / 0 in the second division (nan): the finite / inf / nan
    pattern of numpy, and its values where finite."""
    hx, _lib, tr, L = _hx()
    xi_d = np.array([[1.0, -2.0, 3.0, 0.0, 5.0, -6.0]] * 3)
    xi_num = np.array([[0.0, 1e-300, 0.5, -0.0, -1e-300, 1e-6]])
    xi_den = np.array([[0.0, 1.0, 0.0, 1.0, 2.0, 1.0]])
    num_col = np.zeros(3, dtype=np.int32)
    ndamp = np.array([1, 2, 1], dtype=np.int32)
    den_col = np.array([-1, -1, 0], dtype=np.int32)
    got = tr.xi_ratio(xi_d, xi_num, num_col, ndamp, xi_den=xi_den, den_col=den_col, x0=-5.0)
    ref = _ratio_numpy(xi_d, xi_num, num_col, ndamp, xi_den, den_col, -5.0, 50)
    print(got, ref, sep="\n")
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(np.isinf(got), np.isinf(ref))
    fin = np.isfinite(ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(np.signbit(got[fin]), np.signbit(ref[fin]))
    # (what the cases are there for: alpha = 0, alpha = 1e-300 damped once and twice, 0 / 0 and 0.5 / 0 in the second division)
    assert np.isnan(ref[0, 0]) and ref[0, 1] == 0 and ref[1, 1] == 0 and np.isnan(ref[2, 0]) and ref[2, 2] == 0


def test_argument_errors():
    """nl out of range, a family outside 0 .. 3, ncol < 1, NULL pointers and indices out of range return HX_ERR_ARG and write nothing."""
    hx, _lib, tr, L = _hx()
    lmax, ncol = 8, 3
    n = lmax + 1
    src = np.ascontiguousarray(cr.red_spectra(np.random.default_rng(0), lmax, ncol)[:, :, 0])
    fam = np.array([0, 1, 3], dtype=np.int32)
    bad_fam = (np.array([0, 4, 3], dtype=np.int32), np.array([-1, 1, 3], dtype=np.int32))
    P = _lib.ptr
    for fn in (L.hx_cl2corr_cols, L.hx_corr2cl_cols):
        cases = [(-1, n, ncol, fam, "in", "out"), (lmax, 0, ncol, fam, "in", "out"), (lmax, n + 1, ncol, fam, "in", "out"),
                 (lmax, -2, ncol, fam, "in", "out"), (lmax, n, 0, fam, "in", "out"), (lmax, n, -1, fam, "in", "out"),
                 (lmax, n, ncol, None, "in", "out"), (lmax, n, ncol, fam, None, "out"), (lmax, n, ncol, fam, "in", None)]
        cases += [(lmax, n, ncol, f, "in", "out") for f in bad_fam]
        for args in cases:
            dst = np.full_like(src, 777.0)
            a = [P(v) if isinstance(v, np.ndarray) else P(src) if v == "in" else P(dst) if v == "out" else v for v in args]
            assert fn(*a) == _lib.HX_ERR_ARG, args
            assert (dst == 777.0).all(), args
        dst = np.full_like(src, 777.0)
        _lib.check(fn(lmax, n, ncol, P(fam), P(src), P(dst)))
        assert np.isfinite(dst).all() and not (dst == 777.0).any()
    one = np.array([[0.5] * n] * 2)
    ix = {"num": np.array([0, 1, 0], dtype=np.int32), "den": np.array([-1, 0, 1], dtype=np.int32), "nd": np.array([1, 2, 1], dtype=np.int32)}

    def ratio(n_=n, ncol_=ncol, d="in", num=one, numc=ix["num"], den=one, denc=ix["den"], nd=ix["nd"], out="out"):
        dst = np.full_like(src, 777.0)
        rc = L.hx_xi_ratio(n_, ncol_, P(src) if d == "in" else None, P(num), P(numc), P(den), P(denc), P(nd), -5.0, 50.0, P(dst) if out == "out" else None)
        return rc, dst

    neg = lambda a, v: np.array([a[0], v, a[2]], dtype=np.int32)  # noqa: E731
    for kw in (dict(n_=0), dict(ncol_=0), dict(d=None), dict(num=None), dict(numc=None), dict(nd=None), dict(out=None), dict(den=None),
               dict(numc=neg(ix["num"], -1)), dict(denc=neg(ix["den"], -2)), dict(nd=neg(ix["nd"], -1))):
        rc, dst = ratio(**kw)
        assert rc == _lib.HX_ERR_ARG, kw
        assert (dst == 777.0).all(), kw
    for kw in ({}, dict(den=None, denc=None)):
        rc, dst = ratio(**kw)
        assert rc == _lib.HX_OK and np.isfinite(dst).all() and not (dst == 777.0).any(), kw
