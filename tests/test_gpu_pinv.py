"""``hx_pinv`` (hx_svd.hip: blocked one-sided Jacobi SVD behind ``invert_mixing_matrix``) against the long-double reference of
tests/svd_reference.py, which tests/test_svd_reference.py ties to known answers first.

The comparison rule for every pinv here (``svd_reference.assert_pinv_close``): on the same double-rounded input,
|X_gpu - X_ref|_F <= 4 max(|np.linalg.pinv(M, rcond) - X_ref|_F, tau |X_ref|_F), tau = max(1e-14, 16 * 1.1e-16 sqrt(n_tall)) the
orthogonality the kernel stops at.  Nothing in it comes from the GPU's output.  The ``info`` outputs: ``kept`` exactly; ``largest`` to
1e-13 relative everywhere (LAPACK's own error on it: <= 6e-15); ``smallest_kept`` to 1e-13 where every singular value is kept, to
1e-12 on the column-scaled matrices, and to max(1e-13, 4 * 1.1e-16 s_max / s_kept) below a cut in a graded spectrum: a backward-stable
double algorithm moves a singular value by eps |M|_2 p(n) (Weyl), p(n) = 4 as in the rule -- 1.5e-10 at the deepest cut here (kappa
3.5e5), where LAPACK's own error is up to 4e-12.  At 2240 x 2079 both get 4 max(LAPACK's own error on that value, tau) = 3.3e-13.

Shapes: the column block is 32 with the block count padded to even (33..64 columns: two blocks; 65..96: three and an all-zero
fourth), the LDS tile is 64 rows, rows are padded to 128, and Gram / rotation kernels work in chunks of 256 rows whose partial sums
meet in f64 atomics.  Every reference is computed once per process (lru_cache) and shared by the orientations and switches."""

import ctypes
import functools
import time

import numpy as np
import pytest

import svd_reference as sr

pytestmark = pytest.mark.gpu

LD = sr.LD
EPS = 1.1e-16


def _frozen(M):
    M = np.ascontiguousarray(M, dtype=np.float64)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def _matrix(kind, n, m):
    if kind == "gauss":
        return _frozen(sr.gaussian(n, m))
    if kind == "graded":
        return _frozen(sr.graded(n, m))
    if kind == "colscaled":
        return _frozen(sr.column_scaled(n, m))
    if kind == "band":
        return _frozen(sr.band(n, m))
    if kind == "deficient":
        a = sr.gaussian(n, m).copy()
        a[:, 40], a[:, 69], a[:, 10] = a[:, 3], a[:, 64], 0.0
        return _frozen(a)
    if kind == "rankone":
        rng = np.random.default_rng(n + m)
        return _frozen(np.outer(rng.standard_normal(n), rng.standard_normal(m)))
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _factors(kind, n, m):
    """Long-double factors of the (tall) matrix: shared by every rcond and by the transposed orientation."""
    return sr.factors(_matrix(kind, n, m))


@functools.lru_cache(maxsize=None)
def _reference(kind, n, m, rcond):
    return sr.pinv_from_factors(_factors(kind, n, m), rcond)


@functools.lru_cache(maxsize=None)
def _lapack(kind, n, m, rcond):
    return np.linalg.pinv(_matrix(kind, n, m), rcond=rcond)


def _oriented(M, ref, lapack, transposed):
    """The wide orientation of a tall case: pinv(M^T) = pinv(M)^T exactly, so the tall reference serves both.  (LAPACK's result is
    transposed with it rather than recomputed: its two orientations differ at its own rounding level.)"""
    if not transposed:
        return M, ref, lapack
    return np.ascontiguousarray(M.T), sr.PinvRef(ref.pinv.T, ref.s, ref.kept), lapack.T


def _rel(a, b):
    return abs(float((LD(a) - LD(b)) / LD(b)))


def _check(got, info, M, rcond, ref, lapack, label, smallest_rtol, scale=1.0, largest_rtol=1e-13):
    """kept, largest, smallest_kept and the pinv of one call against the reference (``scale``: the call ran on scale * M)."""
    k = ref.kept
    print(f"pinv {label}: info={info}")
    assert got.shape == (M.shape[1], M.shape[0])
    assert info["kept"] == k, (info, k)
    assert 1 <= info["sweeps"] < 60
    e_large = _rel(info["largest"] / scale, ref.s[0])
    e_small = _rel(info["smallest_kept"] / scale, ref.s[k - 1])
    print(f"pinv {label}: largest off by {e_large:.2e} (allowed {largest_rtol:.2e}), smallest_kept by {e_small:.2e} (allowed {smallest_rtol:.2e})")
    assert e_large <= largest_rtol
    assert e_small <= smallest_rtol
    return sr.assert_pinv_close(got * scale, M, rcond, ref, lapack, label=label)


def _run(kind, n, m, rcond, transposed, smallest_rtol=1e-13, label=None):
    from heracles_amd.twopoint import pinv

    M, ref, lapack = _oriented(_matrix(kind, n, m), _reference(kind, n, m, rcond), _lapack(kind, n, m, rcond), transposed)
    got, info = pinv(M, rcond, info=True)
    return _check(got, info, M, rcond, ref, lapack, f"{label or kind}{'^T' if transposed else ''}", smallest_rtol), info


def _below_cut_rtol(ref):
    return max(1e-13, 4 * EPS * float(ref.s[0] / ref.s[ref.kept - 1]))


# ---- a. edges ------------------------------------------------------------------------------------------------------------------
_EDGES = ([(130, c) for c in (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129)]
          + [(r, 40) for r in (63, 64, 65, 127, 128, 129, 255, 256, 257, 513)] + [(257, 65), (513, 96)])


@pytest.mark.parametrize("transposed", [False, True], ids=["tall", "wide"])
@pytest.mark.parametrize("shape", _EDGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edges_of_blocks_tiles_and_chunks(shape, transposed):
    """Gaussian entries, rcond = 1e-10 below every singular value (kappa of these is <= 1e3): every shape tall and as its transpose
    (the ``tr`` load and ``k_svd_transpose``)."""
    n, m = shape
    ref = _reference("gauss", n, m, 1e-10)
    assert ref.kept == m and ref.s[-1] > 1e-4 * ref.s[0]
    _, info = _run("gauss", n, m, 1e-10, transposed)
    assert info["kept"] == min(n, m)


# ---- b. graded spectra with a cut ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [3e-3, 3e-6])
@pytest.mark.parametrize("shape", [(97, 33), (33, 97), (200, 130), (130, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_graded_spectrum_with_a_cut(shape, target):
    """U diag(logspace(0, -8)) V^T; rcond in the middle of the two adjacent reference singular values nearest the target, which are
    at least 1.05 away from the cut on either side (asserted by ``rcond_between`` on the reference alone: logspace(0, -8, k <= 130)
    has neighbours >= 1.15 apart)."""
    n, m = shape
    tall = (max(n, m), min(n, m))
    rcond, kept = sr.rcond_between(sr.pinv_from_factors(_factors("graded", *tall), 0.0).s, target)
    ref = _reference("graded", *tall, rcond)
    assert ref.kept == kept and 0 < kept < min(n, m)
    _run("graded", *tall, rcond, transposed=n < m, smallest_rtol=_below_cut_rtol(ref), label=f"graded@{target:g}")


# ---- c. column-scaled matrices -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(200, 130), (257, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_column_scaled_small_singular_values_to_relative_accuracy(shape):
    """A diag(logspace(0, -12)), rcond = 1e-14: the singular values span twelve decades and every one of them is determined to high
    relative accuracy by the entries.  This is the case of hx_svd.hip's sentence "One-sided Jacobi computes small singular values to
    high RELATIVE accuracy": the smallest, 1e-12 of the largest, must match the reference to 1e-12 relative -- an algorithm that is
    only backward stable in the norm (LAPACK's bidiagonalisation) owes it to 1e-4."""
    n, m = shape
    ref = _reference("colscaled", n, m, 1e-14)
    assert ref.kept == m and ref.s[-1] < 1e-11 * ref.s[0]
    _run("colscaled", n, m, 1e-14, False, smallest_rtol=1e-12)


# ---- d. bands without noise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(130, 130), (130, 97)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pure_band_converges_and_matches(shape):
    """exp(-((i - j) / 3)^2 / 2) with nothing added: singular values from 7.5 down to 2e-16, numerically rank deficient, the spectrum
    the ``null2`` rule of k_svd_eig and the 60-sweep limit exist for.  rcond near 1e-5 in a gap of the reference's spectrum (68 of
    130 kept, kappa_kept 8e4).  The call must converge (an HxError here is a finding) in fewer than 60 sweeps."""
    n, m = shape
    rcond, kept = sr.rcond_between(sr.pinv_from_factors(_factors("band", n, m), 0.0).s, 1e-5)
    ref = _reference("band", n, m, rcond)
    assert ref.kept == kept and ref.s[-1] < 1e-14 * ref.s[0]
    _, info = _run("band", n, m, rcond, False, smallest_rtol=_below_cut_rtol(ref))
    assert info["sweeps"] < 60


def _mask_spectrum(lmax3, sigma):
    l = np.arange(lmax3 + 1.0)
    return (2 * l + 1) * np.exp(-l * (l + 1) * sigma**2)


def test_mixing_matrix_of_a_small_footprint_spin0():
    """The product's own band: ``mixmat`` of a smooth mask spectrum (2l + 1) exp(-l (l + 1) sigma^2), sigma = 0.02 (a footprint a
    degree across), lmax 96, through ``invert_mixing_matrix``; the singular values are dense around 1e-5 of the largest (neighbours 1.06
    apart), so the cut is the nearest middle that has a gap of 1.05 on either side (``rcond_common`` on the reference alone)."""
    import heracles_amd as hx

    lmax = 96
    M = _frozen(hx.mixmat(_mask_spectrum(2 * lmax, 0.02), lmax, lmax, 2 * lmax))
    f = sr.factors(M)
    rcond, (kept,) = sr.rcond_common([sr.pinv_from_factors(f, 0.0).s], 1e-5)   # (the middle nearest 1e-5 itself has 1.03 on either side)
    ref = sr.pinv_from_factors(f, rcond)
    assert ref.kept == kept and 10 < kept < 90 and 1e-6 < rcond < 1e-4
    key = ("POS", "POS", 0, 0)
    inv = hx.invert_mixing_matrix({key: hx.Result(M, spin=(0, 0), axis=-2, ell=np.arange(lmax + 1))}, rcond=rcond)[key].array
    sr.assert_pinv_close(inv, M, rcond, ref, label="mixmat spin-0")


def test_mixing_matrices_of_a_small_footprint_spin2():
    """``mixmat_eb`` of the same mask at lmax 64 through ``invert_mixing_matrix``: pinv(M0 + M1) = [0] + [1], pinv(M0 - M1) = [0] -
    [1], pinv(M2) = [2] (recombining the halves rounds at 1.1e-16 of the larger inverse, a hundredth of tau).  The three share one
    rcond: the admissible middle nearest 1e-5 that leaves all three spectra a gap of 1.05 (from the references alone).  Rows and
    columns l < 2 are exactly zero."""
    import heracles_amd as hx

    lmax = 64
    E = hx.mixmat_eb(_mask_spectrum(2 * lmax, 0.02), lmax, lmax, 2 * lmax)
    mats = [_frozen(E[0] + E[1]), _frozen(E[0] - E[1]), _frozen(E[2])]
    fs = [sr.factors(M) for M in mats]
    rcond, kept = sr.rcond_common([sr.pinv_from_factors(f, 0.0).s for f in fs], 1e-5)
    assert 3e-6 < rcond < 3e-5
    key = ("SHE", "SHE", 1, 1)
    inv = hx.invert_mixing_matrix({key: hx.Result(E, spin=(2, 2), axis=-2, ell=np.arange(lmax + 1))}, rcond=rcond)[key].array
    got = [inv[0] + inv[1], inv[0] - inv[1], inv[2]]
    for name, M, f, k, x in zip(("M0+M1", "M0-M1", "M2"), mats, fs, kept, got):
        ref = sr.pinv_from_factors(f, rcond)
        assert ref.kept == k <= lmax - 1
        sr.assert_pinv_close(x, M, rcond, ref, label=f"mixmat_eb {name}")


# ---- e. exact rank deficiency -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True], ids=["tall", "wide"])
def test_duplicated_and_zero_columns(transposed):
    """(130, 70) Gaussian with column 40 = column 3 (two blocks), 69 = 64 (inside the last, partial block) and column 10 = 0: rank
    67, the three null singular values are exact zeros or rounding noise."""
    ref = _reference("deficient", 130, 70, 1e-10)
    assert ref.kept == 67 and ref.s[67] < 1e-15 * ref.s[0]
    _run("deficient", 130, 70, 1e-10, transposed)


@pytest.mark.parametrize("transposed", [False, True], ids=["tall", "wide"])
def test_rank_one_outer_product(transposed):
    """u v^T (257, 65) rounded to double: one singular value, 64 of rounding size."""
    ref = _reference("rankone", 257, 65, 1e-10)
    assert ref.kept == 1 and ref.s[1] < 1e-15 * ref.s[0]
    _run("rankone", 257, 65, 1e-10, transposed)


# ---- f. at size, with an exact answer ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kron_lapack():
    c = sr.kron_case()
    return np.linalg.pinv(c["M"], rcond=c["rcond"])


KRON_BUDGET_S = 20.0


def test_kronecker_product_at_size():
    """M = A (x) B, 2240 x 2079 (65 column blocks padded to 66, 9 row chunks, dense singular vectors), rcond 1e-5 between the two
    groups of A's singular values; the answer is pinv_cut(A) (x) pinv(B) from two small long-double references: kept = 27 * 63,
    largest = 1, smallest kept = 0.3 * 0.2.  One call tall from a host array, one on the transpose as a device tensor.  The two GPU
    calls are timed and printed; together they have ``KRON_BUDGET_S`` (hx_svd.hip quotes 1.29 s for one call at n = 4097: the budget is
    there to catch a call that ran out its sweeps, not to measure)."""
    import torch

    from heracles_amd.twopoint import pinv

    c = sr.kron_case()
    M, rcond, ref, lapack = c["M"], c["rcond"], c["ref"], _kron_lapack()
    t0 = time.perf_counter()
    got, info = pinv(M, rcond, info=True)
    t1 = time.perf_counter()
    dev = torch.as_tensor(np.ascontiguousarray(M.T)).cuda()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    got_t, info_t = pinv(dev, rcond, device="cuda", info=True)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print(f"pinv kron: tall host call {t1 - t0:.3f} s ({info['sweeps']} sweeps), wide device call {t3 - t2:.3f} s ({info_t['sweeps']} sweeps)")
    assert got_t.is_cuda and got_t.dtype == torch.float64
    # largest / smallest_kept at this size: 4 max(LAPACK's own relative error on that value, tau), the rule of the pinv applied to a
    # singular value (a routine that stops at orthogonality tau = 16 * 1.1e-16 sqrt(2240) = 8.3e-14 is entitled to tau): 3.3e-13
    s_lapack = np.linalg.svd(M, compute_uv=False)
    rtol = [sr.FACTOR * max(_rel(s_lapack[j], ref.s[j]), sr.tau(max(M.shape))) for j in (0, ref.kept - 1)]
    print(f"pinv kron: allowed on largest {rtol[0]:.2e}, on smallest_kept {rtol[1]:.2e}")
    _check(got, info, M, rcond, ref, lapack, "kron", rtol[1], largest_rtol=rtol[0])
    Mt, ref_t, lapack_t = _oriented(M, ref, lapack, True)
    _check(got_t.cpu().numpy(), info_t, Mt, rcond, ref_t, lapack_t, "kron^T", rtol[1], largest_rtol=rtol[0])
    assert (t1 - t0) + (t3 - t2) < KRON_BUDGET_S


# ---- g. scale and switches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [300, -300])
@pytest.mark.parametrize("kind", ["gauss", "graded"])
def test_scale_invariance(kind, k):
    """pinv(2^k M) = 2^-k pinv(M), k = +-300, on (97, 33): the scaling is exact in double and in the reference, every measure in
    the kernel is relative, so the same reference and the same tolerance hold (``kept`` and, scaled back, ``largest`` and
    ``smallest_kept`` included).  The squared norms, 2^+-600, are inside the double range; their pairwise PRODUCTS are not."""
    from heracles_amd.twopoint import pinv

    n, m = 97, 33
    if kind == "gauss":
        rcond, rtol = 1e-10, 1e-13
    else:
        rcond, _ = sr.rcond_between(sr.pinv_from_factors(_factors(kind, n, m), 0.0).s, 3e-6)
        rtol = _below_cut_rtol(_reference(kind, n, m, rcond))
    M, ref, lapack = _matrix(kind, n, m), _reference(kind, n, m, rcond), _lapack(kind, n, m, rcond)
    scale = 2.0**k
    scaled = M * scale
    assert np.isfinite(scaled).all() and np.array_equal(scaled / scale, M)
    got, info = pinv(scaled, rcond, info=True)
    _check(got, info, M, rcond, ref, lapack, f"{kind} * 2^{k}", rtol, scale=scale)


def test_more_inner_sweeps_give_the_same_answer(monkeypatch):
    """HX_SVD_INNER (read on every call) = 4 inner Jacobi sweeps per Gram matrix instead of one."""
    monkeypatch.setenv("HX_SVD_INNER", "4")
    _run("gauss", 200, 130, 1e-10, False, label="gauss inner=4")
    rcond, _ = sr.rcond_between(sr.pinv_from_factors(_factors("graded", 200, 130), 0.0).s, 3e-6)
    _run("graded", 200, 130, rcond, False, smallest_rtol=_below_cut_rtol(_reference("graded", 200, 130, rcond)), label="graded inner=4")


def test_two_calls_agree():
    """Two calls on (257, 65), two row chunks: the Gram sums meet in f64 atomics, whose order is not fixed, so the results need
    not be bit-for-bit equal; each is within the rule of the reference, and so within twice its allowance of each other."""
    from heracles_amd.twopoint import pinv

    M, ref, lapack = _matrix("gauss", 257, 65), _reference("gauss", 257, 65, 1e-10), _lapack("gauss", 257, 65, 1e-10)
    a, b = pinv(M, 1e-10), pinv(M, 1e-10)
    sr.assert_pinv_close(a, M, 1e-10, ref, lapack, label="first call")
    e = sr.pinv_errors(b, M, 1e-10, ref, lapack)
    assert e["ratio"] <= sr.FACTOR
    diff = sr.fro(a - b)
    print(f"pinv two calls: |a - b|_F = {diff:.3e} ({'bit-for-bit' if diff == 0 else 'not bit-for-bit'})")
    assert diff <= 2 * sr.FACTOR * max(e["e_lapack"], e["floor"])


# ---- h. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [(5, 0), (129, 69)], ids=["first_block", "last_block"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("transposed", [False, True], ids=["tall", "wide"])
def test_non_finite_input_is_refused_and_nothing_written(bad, where, transposed):
    """A NaN or an infinity made the squared Frobenius norm, hence ``null2``, non-finite: every pair left the convergence measure and
    the first sweep "converged" on garbage with HX_OK.  Now an error (numpy.linalg.pinv raises LinAlgError), host and device output
    untouched."""
    import torch

    import heracles_amd as hx
    from heracles_amd.twopoint import pinv

    a = sr.gaussian(130, 70).copy()
    a[where] = bad
    a = np.ascontiguousarray(a.T) if transposed else a
    n, m = a.shape
    with pytest.raises(hx.HxError, match="NaN or an infinity"):
        pinv(a, 1e-10)
    with pytest.raises(hx.HxError, match="NaN or an infinity"):
        pinv(torch.as_tensor(a).cuda(), 1e-10, device="cuda")
    L = hx._lib.load()
    out = np.full((m, n), 7.0)
    info = (ctypes.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
    with pytest.raises(hx.HxError):
        hx._lib.check(L.hx_pinv(n, m, hx._lib.ptr(a), 1e-10, hx._lib.ptr(out), info))
    assert (out == 7.0).all() and list(info) == [-1.0] * 4
    dout = torch.full((m, n), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(hx.HxError):
        hx._lib.check(L.hx_pinv(n, m, hx._lib.ptr(torch.as_tensor(a).cuda()), 1e-10, hx._lib.ptr(dout), None))
    assert bool((dout == 7.0).all())
    # and the library is fine afterwards
    ok = sr.gaussian(9, 6)
    np.testing.assert_allclose(pinv(ok, 1e-10), np.linalg.pinv(ok, rcond=1e-10), atol=1e-13)


@pytest.mark.parametrize("device", ["cpu", "cuda"])
@pytest.mark.parametrize("dtype", ["float32", "float16", "int64", "int32"])
def test_tensors_of_other_types_are_converted(dtype, device):
    """A tensor went to hx_pinv as it was: a float32 tensor has half the bytes the kernel reads.  Now it is converted like a numpy
    array is; the result is that of the float64 copy."""
    import torch

    from heracles_amd.twopoint import pinv

    base = np.round(sr.gaussian(97, 33) * 8.0)   # small integers: exact in every one of the types
    t = torch.as_tensor(base).to(getattr(torch, dtype)).to(device)
    M = _frozen(t.cpu().to(torch.float64).numpy())
    assert np.array_equal(M, base)
    ref, lapack = sr.pinv_reference(M, 1e-10), np.linalg.pinv(M, rcond=1e-10)
    sr.assert_pinv_close(pinv(t, 1e-10), M, 1e-10, ref, lapack, label=f"{dtype} tensor on {device}")
    sr.assert_pinv_close(pinv(base.astype(dtype), 1e-10), M, 1e-10, ref, lapack, label=f"{dtype} array")
    out = pinv(t, 1e-10, device="cuda")
    assert out.dtype == torch.float64 and out.shape == (33, 97)
    sr.assert_pinv_close(out.cpu().numpy(), M, 1e-10, ref, lapack, label=f"{dtype} tensor on {device} -> device")


def test_transposed_view_gives_the_result_of_its_contiguous_copy():
    import torch

    import heracles_amd as hx
    from heracles_amd.twopoint import pinv

    M, ref, lapack = _oriented(_matrix("gauss", 130, 33), _reference("gauss", 130, 33, 1e-10), _lapack("gauss", 130, 33, 1e-10), True)
    view = torch.as_tensor(np.array(_matrix("gauss", 130, 33))).cuda().T   # (33, 130), strides (1, 33)
    assert not view.is_contiguous() and view.shape == (33, 130)
    sr.assert_pinv_close(pinv(view, 1e-10), M, 1e-10, ref, lapack, label="transposed device view")
    sr.assert_pinv_close(pinv(np.array(_matrix("gauss", 130, 33)).T, 1e-10), M, 1e-10, ref, lapack, label="transposed numpy view")
    sr.assert_pinv_close(pinv(hx.DeviceArray(view, {}), 1e-10), M, 1e-10, ref, lapack, label="DeviceArray of the view")


def test_inputs_that_are_no_matrix_raise_in_python():
    import torch

    from heracles_amd.twopoint import pinv

    for bad in (np.zeros((2, 3, 4)), np.zeros(5), torch.zeros((2, 3, 4), dtype=torch.float64), torch.zeros(5, dtype=torch.float64),
                torch.zeros((2, 3, 4), dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError, match="two-dimensional"):
            pinv(bad, 1e-5)
