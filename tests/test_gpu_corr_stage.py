"""hx_cl2corr / hx_corr2cl (k_corr_tables, k_cl2corr, k_corr2cl) at production band limits, through the C ABI, against the long-double
truth of tests/corr_reference.py evaluated at the library's own Gauss-Legendre nodes.

Yardstick: the oracle (oracle/hx_oracle.c: the reference's closed forms in P_l, P_l' in double, heracles/transforms.py:46-204) run at
the same nodes and weights.  The closed forms cancel towards x -> +-1, so the honest bound is not a fixed number but what the same
formulas give in plain double: per input kind, output column and band,
    E_gpu = max |gpu - truth|  <=  8 E_ref + floor,   E_ref = max |oracle - truth|,
floor = 16 eps sum |terms| of the sum itself.  The 8: two builds of the oracle (contracted to FMA as hipcc does, and plain) differ by
at most 2.22 in this ratio over lmax 97 .. 4096, all kinds, bands and columns; 8 leaves 3.6x over that.  Nothing here is fitted to what
the GPU returned.  The multipole at which k_corr_tables switches from the small-angle series to the closed form is NOT pinned: the two
differ there by the closed form's own noise (1e-13 .. 2e-11 on 1e-6), so an off-by-one is invisible to any honest tolerance.

Measured on the MI355X: see DESIGN.md section 2, "Tolerances"."""

import ctypes
import time

import numpy as np
import pytest

import corr_reference as cr

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _hx():
    import heracles_amd as hx
    from heracles_amd import _lib, transforms as tr

    _lib.ensure_init()
    return hx, _lib, tr, _lib.load()


def _call(fn, arr, lmax):
    """One call of hx_cl2corr / hx_corr2cl on [nspec][lmax+1][4]."""
    _, _lib, tr, _ = _hx()
    return tr._batch(fn, list(arr), lmax)


def _oracle_cl2corr(oracle, cls, x, w):
    xw = np.concatenate([x, w])
    out = np.empty_like(cls)
    for s in range(cls.shape[0]):
        oracle.lib().hxo_cl2corr(ctypes.c_int(cls.shape[1] - 1), oracle._p(np.ascontiguousarray(cls[s])), oracle._p(xw), oracle._p(out[s]))
    return out


def _oracle_corr2cl(oracle, corrs, x, w):
    xw = np.concatenate([x, w])
    out = np.empty_like(corrs)
    for s in range(corrs.shape[0]):
        oracle.lib().hxo_corr2cl(ctypes.c_int(corrs.shape[1] - 1), oracle._p(np.ascontiguousarray(corrs[s])), oracle._p(xw), oracle._p(out[s]))
    return out


def _oracle_pulse_response(oracle, lmax, xk, wk, amp):
    """What hxo_corr2cl returns for xi = amp[ix] at the single node (xk, wk) and zero elsewhere, in its own operation order (one term per
    sum), without its O(n) loop over the empty nodes: [lmax+1][4]."""
    (P, _), (d20, d22, d2m2) = oracle.legendre_funcs(lmax, float(xk))
    out = np.zeros((lmax + 1, 4))
    out[:, 0] = (wk * amp[0]) * P
    if lmax >= 2:
        T2 = (amp[1] * wk / 2.0) * d22
        T4 = (amp[2] * wk / 2.0) * d2m2
        out[2:, 1] = T2 + T4
        out[2:, 2] = T2 - T4
        out[2:, 3] = (wk * amp[3]) * d20
    return out * (2.0 * np.pi)


PULSE_AMPS = (np.array([1.0, 1.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0, 0.0]))


def _pulses(n, nodes):
    """Two unit pulses per node: (T, Q+U, cross) and (Q-U) apart, so that the output is 2 pi w_k times single table columns."""
    out = np.zeros((2 * len(nodes), n, 4))
    for i, k in enumerate(nodes):
        for j, amp in enumerate(PULSE_AMPS):
            out[2 * i + j, k] = amp
    return out


def _check(tag, rows, failures):
    print(cr.format_rows(tag, rows))
    for ix, name, eg, er, bound in rows:
        if not eg <= bound:
            failures.append(f"{tag} column {ix} band {name}: E_gpu {eg:.3e} > 8 * E_ref {er:.3e} + floor = {bound:.3e}")


def _nodes_are_the_tables_nodes(got_l1_tt, x):
    """The TT probe at l = 1 returns P_1 = x_k: the nodes the tables were built from are those of hx.gauss_legendre, to 4 ulp (the
    probe's factor f_1 c_1 is 1 only to rounding)."""
    assert (np.abs(got_l1_tt - x) <= 4 * np.spacing(np.abs(x))).all(), np.abs(got_l1_tt - x).max()


@pytest.mark.parametrize("lmax", [300, 1024, 2048, 4096, 6144])
def test_error_against_truth(oracle, lmax):
    """Red spectra, white spectra (which weight multipole l by 2l + 1 and so expose the high-l table rows a red spectrum hides) and
    single-l probes (TT = EE = TE = 4 pi / (2l + 1) at one l: the output is the table row) in ONE batched hx_cl2corr; then hx_corr2cl
    of the truth xi of the red spectrum, of white-noise xi and of unit pulses at single nodes (the output is 2 pi w_k times a table
    column).  Per kind, column and band the yardstick of the module docstring; probes and pulses pooled (one probe row at 8 nodes is a
    single draw of a drifting recursion error: two correct implementations differ by up to 6x there, pooled they do not).
    Measured on the MI355X, lmax 300 .. 6144: E_gpu / E_ref = 1.00 in every xi band (largest E_gpu: 1.86e-9, probes, Q+U, the 8 nodes at
    x -> -1, lmax 6144), 0.03 .. 1.21 where the summation dominates; xi(red) coming back: max |err| (1+l)^2 = 5.7e-10 at 6144."""
    hx, _lib, tr, L = _hx()
    t0 = time.time()
    rng = np.random.default_rng(lmax)
    x, w = hx.gauss_legendre(lmax + 1)
    ox, ow = oracle.gauss_legendre(lmax + 1)
    print(f"\nlmax {lmax}: nodes vs long-double Newton max |dx| {np.abs(x - ox).max():.2e}, weights max |dw| / w {np.abs(w / ow - 1).max():.2e}")
    # (truth and oracle below both take the library's nodes and weights, so the yardstick cannot see an error in them; this does.  A node
    # is a double: 4 eps.  The weights enter corr2cl linearly and the oracle's own corr2cl is good to 3e-11 .. 4e-10 of (1+l)^-2 at lmax
    # 2048 .. 6144: a relative weight error below 1e-11 is below what anything here resolves; numpy's leggauss misses it by 1e3 at 1025 nodes)
    assert np.abs(x - ox).max() <= 4 * EPS and np.abs(w / ow - 1).max() <= 1e-11
    # ---- cl2corr: red, white and single-l probes in one batched call
    ls = cr.probe_multipoles(rng, lmax, x)
    cls = np.concatenate([cr.red_spectra(rng, lmax), cr.white_spectra(rng, lmax), cr.probe_spectra(lmax, ls)])
    got = _call(L.hx_cl2corr, cls, lmax)
    _nodes_are_the_tables_nodes(got[2 + ls.index(1), :, 0], x)
    ref = _oracle_cl2corr(oracle, cls, x, w)
    truth = cr.cl2corr_truth(cls, x)
    floor = cr.cl2corr_floor(cls)
    bands = cr.node_bands(x)
    failures = []
    kinds = {"red": [0], "white": [1], "probes": list(range(2, len(cls)))}
    for kind, specs in kinds.items():
        _check(f"cl2corr {lmax} {kind}", cr.yardstick(got, ref, truth, floor, bands, specs), failures)
    for i, l in enumerate(ls):  # per probe: reported, not asserted (one row at 8 nodes is a single draw of a drifting recursion error)
        rows = cr.yardstick(got, ref, truth, floor, bands, [2 + i])
        print(f"  probe l={l}: ratios " + " ".join(f"{eg / er:.2f}" if er else "-" for _, _, eg, er, _ in rows))
    # ---- corr2cl: the truth xi of the red spectrum, white-noise xi, unit pulses
    n = lmax + 1
    dense = np.stack([truth[0].astype(np.float64), rng.standard_normal((n, 4))])
    nodes = sorted({k for k in (0, n - 1, n // 2, 255, 256, 257) if k < n})
    xi = np.concatenate([dense, _pulses(n, nodes)])
    got2 = _call(L.hx_corr2cl, xi, lmax)
    ref2 = np.concatenate([_oracle_corr2cl(oracle, dense, x, w)] +
                          [_oracle_pulse_response(oracle, lmax, x[k], w[k], amp)[None] for k in nodes for amp in PULSE_AMPS])
    truth2 = np.concatenate([cr.corr2cl_truth(dense, x, w), cr.corr2cl_truth(xi[2:][:, nodes], x[nodes], w[nodes], lmax=lmax)])
    floor2 = cr.corr2cl_floor(xi, w)
    lb = cr.ell_bands(lmax)
    for kind, specs in {"xi(red)": [0], "normal": [1], "pulses": list(range(2, len(xi)))}.items():
        _check(f"corr2cl {lmax} {kind}", cr.yardstick(got2, ref2, truth2, floor2, lb, specs), failures)
    e = np.abs(got2[0].astype(cr.LD) - truth2[0]).astype(np.float64) * (1.0 + np.arange(n))[:, None] ** 2
    print(f"corr2cl {lmax} xi(red): max |err| (1+l)^2 = {e.max():.2e}; took {time.time() - t0:.1f} s")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("lmax", [0, 1, 2, 3, 62, 63, 64, 126, 127, 128, 254, 255, 256, 257, 511, 512])
def test_block_and_stride_edges(oracle, lmax):
    """n = lmax + 1 around the 64-thread blocks of k_corr_tables / k_cl2corr (row stride kpad = ceil64(n)) and the 256-thread stride of
    k_corr2cl: max |gpu - oracle| <= 8 max |oracle - truth| + floor per column, both directions.  lmax 126 is the case that found the
    FMA contraction of k_corr_tables: at the last node the contracted recursion was 3.9e-11 from the oracle where the oracle is 1.7e-12
    from the truth (white spectrum, Q-U); uncontracted the two agree to 2e-14 there."""
    hx, _lib, tr, L = _hx()
    rng = np.random.default_rng(1000 + lmax)
    x, w = hx.gauss_legendre(lmax + 1)
    cls = np.concatenate([cr.red_spectra(rng, lmax), cr.white_spectra(rng, lmax), cr.red_spectra(rng, lmax)])
    got = _call(L.hx_cl2corr, cls, lmax)
    ref = _oracle_cl2corr(oracle, cls, x, w)
    truth = cr.cl2corr_truth(cls, x)
    xi = np.stack([truth[0].astype(np.float64), rng.standard_normal((lmax + 1, 4)), rng.standard_normal((lmax + 1, 4))])
    got2 = _call(L.hx_corr2cl, xi, lmax)
    ref2 = _oracle_corr2cl(oracle, xi, x, w)
    truth2 = cr.corr2cl_truth(xi, x, w)
    for tag, g, r, t, fl in (("cl2corr", got, ref, truth, cr.cl2corr_floor(cls)), ("corr2cl", got2, ref2, truth2, cr.corr2cl_floor(xi, w))):
        for ix in range(4):
            d = np.abs(g[..., ix] - r[..., ix]).max()
            e_ref = float(np.abs(r[..., ix].astype(cr.LD) - t[..., ix]).max())
            print(f"{tag} lmax {lmax} column {ix}: max |gpu - oracle| {d:.2e}, max |oracle - truth| {e_ref:.2e}")
            assert d <= 8 * e_ref + fl[:, ix].max(), (tag, lmax, ix, d, e_ref)
        if lmax < 2:
            assert (g[..., 1:] == 0).all(), "no polarisation below l = 2"
    if lmax < 2:
        one = tr._cl2corr(cls[0, :, 0])
        assert one.shape == (lmax + 1, 4) and (one[:, 1:] == 0).all()
        np.testing.assert_array_equal(one[:, 0], tr._cl2corr(np.stack([cls[0, :, 0]] + [np.zeros(lmax + 1)] * 3).T)[:, 0])
        assert np.abs(one[:, 0] - truth[0, :, 0]).max() <= 8 * float(np.abs(ref[0, :, 0] - truth[0, :, 0]).max()) + cr.cl2corr_floor(cls)[0, 0]
        back = tr._corr2cl(xi[1, :, 0])
        assert back.shape == (lmax + 1, 4) and (back[:, 1:] == 0).all()
        assert np.abs(back[:, 0] - truth2[1, :, 0]).max() <= 8 * float(np.abs(ref2[1, :, 0] - truth2[1, :, 0]).max()) + cr.corr2cl_floor(xi, w)[1, 0]


@pytest.mark.parametrize("lmax", [300, 2048])
def test_batch_repeatability_residence(lmax):
    """Spectrum i of a batched call is bitwise the call with that spectrum alone (each output element is one thread's sequential sum, or
    one block's fixed tree); two identical calls agree bitwise; device-resident float64 tensors in and out give the host result and
    leave the input untouched."""
    import torch

    hx, _lib, tr, L = _hx()
    rng = np.random.default_rng(7 + lmax)
    for fn in (L.hx_cl2corr, L.hx_corr2cl):
        for nspec in (1, 2, 7, 33):
            arr = np.concatenate([cr.red_spectra(rng, lmax, nspec - nspec // 2), cr.white_spectra(rng, lmax, nspec // 2)]) if nspec > 1 \
                else cr.red_spectra(rng, lmax, 1)
            assert len({a.tobytes() for a in arr}) == nspec
            out = _call(fn, arr, lmax)
            np.testing.assert_array_equal(_call(fn, arr, lmax), out)
            for i in range(nspec):
                np.testing.assert_array_equal(_call(fn, arr[i : i + 1], lmax)[0], out[i], err_msg=f"spectrum {i} of {nspec}")
            tin = torch.from_numpy(arr).cuda()
            keep = tin.clone()
            tout = torch.full_like(tin, float("nan"))
            _lib.check(fn(int(lmax), nspec, _lib.ptr(tin), _lib.ptr(tout)))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(tout.cpu().numpy(), out)
            assert torch.equal(tin, keep)


def test_cache_across_sizes():
    """The table cache is keyed by lmax and its buffers are re-used when a smaller size follows a larger one: every time a size comes
    round again the result is bitwise what the first call at that size returned, also after hx_release_caches."""
    hx, _lib, tr, L = _hx()
    rng = np.random.default_rng(11)
    inputs = {lm: cr.red_spectra(rng, lm, 2) for lm in (300, 64, 2048)}
    first = {}
    seq = [300, 64, 300, 2048, 300]
    for i, lm in enumerate(seq):
        if i == len(seq) - 1:
            hx.release_caches()
        fwd = _call(L.hx_cl2corr, inputs[lm], lm)
        back = _call(L.hx_corr2cl, fwd, lm)
        if lm in first:
            np.testing.assert_array_equal(fwd, first[lm][0])
            np.testing.assert_array_equal(back, first[lm][1])
        else:
            first[lm] = (fwd, back)


def test_release_caches_frees_the_tables():
    """After one hx_cl2corr at lmax 4096 the tables hold 4 * 4097 * 4160 * 8 B = 545 MB; hx_release_caches hands them back.  mem_get_info
    is device-wide, so another tenant's allocation can disturb it: half of the 545 MB is the allowance for that."""
    import torch

    hx, _lib, tr, L = _hx()
    lmax = 4096
    cls = cr.red_spectra(np.random.default_rng(5), lmax, 1)
    a = _call(L.hx_cl2corr, cls, lmax)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    hx.release_caches()
    after = torch.cuda.mem_get_info()[0]
    tables = 4 * (lmax + 1) * 4160 * 8
    print(f"\nfree HBM rose by {(after - before) / 1e6:.0f} MB across release_caches (tables: {tables / 1e6:.0f} MB)")
    assert after - before >= tables // 2, (before, after)
    np.testing.assert_array_equal(_call(L.hx_cl2corr, cls, lmax), a)
    hx.release_caches()


def test_table_above_4_gib(oracle):
    """lmax 12288: 4 * 12289 * 12352 * 8 B = 4.86 GB of tables, the first size whose byte offsets pass 2^32 (naturalspice gets there with
    a mask at twice the data's band limit of 6144).  Truth at 64 chosen nodes only (each node is independent): the yardstick of
    test_error_against_truth on those nodes for a red and a white spectrum, and for unit pulses at those nodes over all l."""
    import torch

    hx, _lib, tr, L = _hx()
    lmax = 12288
    n = lmax + 1
    hx.release_caches()
    free = torch.cuda.mem_get_info()[0]
    assert free >= 12e9, f"only {free / 1e9:.1f} GB of HBM free: the 4.9 GB tables of lmax 12288 plus head room need 12 GB"
    rng = np.random.default_rng(lmax)
    x, w = hx.gauss_legendre(n)
    ser = np.flatnonzero(x > 0.998)[:-8]
    sub = set(range(8)) | set(range(n - 8, n)) | set(rng.choice(ser, 16, replace=False).tolist()) | set(range(1023, n, 1024))
    rest = np.setdiff1d(np.arange(n), sorted(sub))
    sub = np.array(sorted(sub | set(rng.choice(rest, 64 - len(sub), replace=False).tolist())))
    assert len(sub) == 64
    bands = {k: m[sub] for k, m in cr.node_bands(x).items()}
    failures = []
    try:
        cls = np.concatenate([cr.red_spectra(rng, lmax), cr.white_spectra(rng, lmax)])
        got = _call(L.hx_cl2corr, cls, lmax)[:, sub]
        ref = _oracle_cl2corr(oracle, cls, x, w)[:, sub]
        truth = cr.cl2corr_truth(cls, x[sub])
        floor = cr.cl2corr_floor(cls)
        for kind, specs in {"red": [0], "white": [1]}.items():
            _check(f"cl2corr {lmax} {kind}", cr.yardstick(got, ref, truth, floor, bands, specs), failures)
        xi = _pulses(n, sub)
        got2 = _call(L.hx_corr2cl, xi, lmax)
        ref2 = np.stack([_oracle_pulse_response(oracle, lmax, x[k], w[k], amp) for k in sub for amp in PULSE_AMPS])
        truth2 = cr.corr2cl_truth(xi[:, sub], x[sub], w[sub], lmax=lmax)
        _check(f"corr2cl {lmax} pulses", cr.yardstick(got2, ref2, truth2, cr.corr2cl_floor(xi, w), cr.ell_bands(lmax)), failures)
    finally:
        hx.release_caches()
    assert not failures, "\n".join(failures)


def test_argument_errors():
    """lmax < 0, nspec < 1 and NULL pointers return HX_ERR_ARG and write nothing."""
    hx, _lib, tr, L = _hx()
    lmax = 8
    src = cr.red_spectra(np.random.default_rng(0), lmax, 2)
    for fn in (L.hx_cl2corr, L.hx_corr2cl):
        for args in ((-1, 2, "in", "out"), (lmax, 0, "in", "out"), (lmax, -3, "in", "out"), (lmax, 2, None, "out"), (lmax, 2, "in", None)):
            dst = np.full_like(src, 777.0)
            a = [_lib.ptr(src) if v == "in" else _lib.ptr(dst) if v == "out" else v for v in args]
            assert fn(*a) == _lib.HX_ERR_ARG, args
            assert (dst == 777.0).all(), args
        dst = np.full_like(src, 777.0)
        _lib.check(fn(lmax, 2, _lib.ptr(src), _lib.ptr(dst)))
        assert np.isfinite(dst).all() and not (dst == 777.0).any()


# ---- the reference's own results past one block (tests/golden/make_golden_transforms.py) ----------------------------------------
def _reference_vectors():
    import os

    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_transforms.npz"))


@pytest.mark.parametrize("lm", [300, 1024, 2048])
def test_reference_vectors_past_one_block(lm):
    """_cl2corr / _corr2cl against heracles.transforms at lmax 300 .. 2048, within 8x what the oracle deviates from the same arrays in the
    same norm (stored in the fixture; the reference's side of that deviation is numpy's leggauss, off by up to 7e-8 in the end weights)."""
    hx, _lib, tr, L = _hx()
    g = _reference_vectors()
    cls, corr, back = g[f"c2c/{lm}/cls"], g[f"c2c/{lm}/corr"], g[f"c2c/{lm}/cls_back"]
    d1, d2 = cr.dev_xi(tr._cl2corr(cls), corr), cr.dev_cl(tr._corr2cl(corr), back)
    print(f"\nlmax {lm} vs reference: xi max |d| / max |ref| {d1} (oracle {g[f'c2c/{lm}/dev_corr']}); "
          f"cl back max |d| (1+l)^2 {d2} (oracle {g[f'c2c/{lm}/dev_back']})")
    assert (d1 <= 8 * g[f"c2c/{lm}/dev_corr"]).all(), d1 / g[f"c2c/{lm}/dev_corr"]
    assert (d2 <= 8 * g[f"c2c/{lm}/dev_back"]).all(), d2 / g[f"c2c/{lm}/dev_back"]


def test_dict_drivers_and_naturalspice_reference_vectors():
    """hx.cl2corr / hx.corr2cl at lmax 256 and hx.naturalspice with masks at lmax 512 against the reference, within 8x the deviation of
    the same Python layer on the oracle from the same arrays."""
    import types

    from helpers import key_str

    hx, _lib, tr, L = _hx()
    g = _reference_vectors()
    Ld, Lm = 256, 512
    ell, ellm = np.arange(Ld + 1), np.arange(Lm + 1)
    keys = {("POS", "POS", 0, 0): (0, 0), ("POS", "SHE", 0, 0): (0, 2), ("SHE", "SHE", 0, 0): (2, 2)}
    d = {k: hx.Result(np.array(g[f"dict/d/{key_str(k)}"]), spin=s, axis=-1, ell=ell) for k, s in keys.items()}
    wd = hx.cl2corr(d)
    back = hx.corr2cl({k: hx.Result(np.array(g[f"dict/wd/{key_str(k)}"]), spin=s, axis=-1, ell=wd[k].ell) for k, s in keys.items()})
    failures = []
    for k in d:
        ks = key_str(k)
        a, b = cr.dev_rel(wd[k].array, g[f"dict/wd/{ks}"]), cr.dev_back(back[k].array, g[f"dict/back/{ks}"])
        print(f"\ndict {ks}: xi {a:.2e} (oracle {g[f'dict/dev_wd/{ks}']:.2e}), cl back (1+l)^2 {b:.2e} (oracle {g[f'dict/dev_back/{ks}']:.2e})")
        if not (a <= 8 * g[f"dict/dev_wd/{ks}"] and b <= 8 * g[f"dict/dev_back/{ks}"]):
            failures.append(f"dict {ks}: {a:.3e} / {b:.3e}")
    fields = {"POS": types.SimpleNamespace(mask="VIS", spin=0), "SHE": types.SimpleNamespace(mask="WHT", spin=2)}
    for tag, tm in (("default", None), ("theta30", 30.0)):
        m = {k: hx.Result(np.array(g[f"ns/m/{key_str(k)}"]), spin=(0, 0), axis=-1, ell=ellm)
             for k in (("VIS", "VIS", 0, 0), ("VIS", "WHT", 0, 0), ("WHT", "WHT", 0, 0))}
        with np.errstate(over="ignore"):  # (the damping factor overflows to inf where the mask's xi vanishes, as in the reference)
            res = hx.naturalspice(d, m, fields, theta_max=tm)
        for k in d:
            ks = key_str(k)
            a = cr.dev_rel(res[k].array, g[f"ns/{tag}/{ks}"])
            print(f"naturalspice {tag} {ks}: max |d| / max |ref| {a:.2e} (oracle {g[f'ns/dev_{tag}/{ks}']:.2e})")
            if not a <= 8 * g[f"ns/dev_{tag}/{ks}"]:
                failures.append(f"naturalspice {tag} {ks}: {a:.3e} > 8 * {g[f'ns/dev_{tag}/{ks}']:.3e}")
    hx.release_caches()
    assert not failures, "\n".join(failures)
