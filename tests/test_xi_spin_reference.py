"""tests/xi_spin_reference.py (the long-double d^l_{ab} of any pair) pinned on its own, and the host side of ``exact_spin``: what
``spice_plan`` emits for keys of other spin weights, and ``run_spice_plan`` / ``naturalspice_batch`` on numpy operations built from the
reference tables against the dict route (``naturalspice``) on the same tables.  No GPU: the kernels meet the same reference in
tests/test_gpu_xi_spin.py."""

import types

import numpy as np
import pytest

import corr_reference as cr
import xi_spin_reference as xr
import heracles_amd as hx
from heracles_amd import jackknife as jk, transforms as tr, unmixing as um

LD = cr.LD
PAIRS = [(0, 0), (2, 2), (2, -2), (2, 0), (1, 0), (0, 1), (1, 1), (1, -1), (-1, 1), (2, 1), (1, 2), (3, 1), (3, -1), (-3, 1), (3, 3), (5, -2), (-2, 5),
         (4, 0), (0, -3)]


def _nodes_ld(n):
    """Gauss-Legendre nodes and weights in long double: numpy's nodes, refined by Newton steps on P_n in long double."""
    x = np.polynomial.legendre.leggauss(n)[0].astype(LD)
    for _ in range(3):
        p0, p1 = np.ones_like(x), x
        for k in range(2, n + 1):
            p0, p1 = p1, (LD(2 * k - 1) * x * p1 - LD(k - 1) * p0) / LD(k)
        dp = LD(n) * (x * p1 - p0) / (x * x - 1)
        x = x - p1 / dp
    p0, p1 = np.ones_like(x), x
    for k in range(2, n + 1):
        p0, p1 = p1, (LD(2 * k - 1) * x * p1 - LD(k - 1) * p0) / LD(k)
    dp = LD(n) * (x * p1 - p0) / (x * x - 1)
    return x, 2 / ((1 - x * x) * dp * dp)


def test_the_four_families_are_corr_reference():
    """(0,0), (2,2), (2,-2), (2,0) against corr_reference.table_truth at Gauss-Legendre nodes and next to the poles: the same recursion in
    the same arithmetic from the same start, up to the order of the seed's factors -- a few long-double roundings, each carried through at
    most lmax steps that do not amplify it (|d| <= 1): 16 lmax eps_ld."""
    lmax = 130
    x = np.concatenate([np.polynomial.legendre.leggauss(lmax + 1)[0], [-1.0, -1.0 + 1e-9, 0.0, 0.999, 1.0 - 1e-12, 1.0]])
    truth = cr.table_truth(lmax, x, range(lmax + 1))
    for ix, (a, b) in enumerate(cr.FAMILIES):
        got = xr.wigner_table(lmax, a, b, x)
        assert float(np.abs(got - truth[:, ix]).max()) <= 16 * lmax * cr.EPS_LD, (a, b)


def test_symmetries():
    """d_{ab} = (-1)^{a-b} d_{ba} = d_{-b,-a} (how pairs share a seed), and d^l_{ab}(-x) = (-1)^{l+a} d^l_{a,-b}(x), which ties tables of
    DIFFERENT normalised pairs and recursions together.  The first two hold to the bit (same seed, coefficients symmetric in a and b); the
    reflection to the rounding the recursion carries: 16 lmax eps_ld as above."""
    lmax = 40
    x = np.concatenate([np.polynomial.legendre.leggauss(lmax + 1)[0], [0.3, 0.999999]])
    for a, b in PAIRS:
        t = xr.wigner_table(lmax, a, b, x)
        flip = -1 if (a - b) % 2 else 1
        np.testing.assert_array_equal(t, flip * xr.wigner_table(lmax, b, a, x), err_msg=str((a, b)))
        np.testing.assert_array_equal(t, xr.wigner_table(lmax, -b, -a, x), err_msg=str((a, b)))
        sign = np.where((np.arange(lmax + 1) + a) % 2, -1, 1).astype(LD)[:, None]
        mirrored = xr.wigner_table(lmax, a, b, -x)
        assert float(np.abs(mirrored - sign * xr.wigner_table(lmax, a, -b, x)).max()) <= 16 * lmax * cr.EPS_LD, (a, b)
        assert (t[: max(abs(a), abs(b))] == 0).all()


def test_orthogonality_under_gauss_legendre_quadrature():
    """sum_k w_k d^l_{ab}(x_k) d^l'_{ab}(x_k) = 2 / (2l + 1) delta_{ll'} for l, l' <= lmax at lmax + 1 nodes (exact: degree 2 lmax), with
    long-double nodes and weights.  A sum of lmax + 1 terms bounded by w_k, whose total is 2, of factors carrying 16 lmax eps_ld each:
    64 lmax eps_ld."""
    lmax = 40
    x, w = _nodes_ld(lmax + 1)
    assert abs(float(w.sum() - 2)) < 64 * cr.EPS_LD
    for a, b in PAIRS:
        t = xr.wigner_table(lmax, a, b, x)
        l0 = max(abs(a), abs(b))
        gram = (t * w) @ t.T
        want = np.diag(np.where(np.arange(lmax + 1) >= l0, 2 / (2 * np.arange(lmax + 1).astype(LD) + 1), 0))
        assert float(np.abs(gram - want).max()) <= 64 * lmax * cr.EPS_LD, (a, b)


def test_forward_and_back_are_inverse_on_the_reference():
    """Tables.back(Tables.forward(a)) = a from l0 on and 0 below, whatever lies below l0 in the input (it is not read)."""
    lmax = 24
    x, w = _nodes_ld(lmax + 1)
    tabs = xr.Tables(lmax, x, w)
    rng = np.random.default_rng(1)
    pairs = [(1, 0), (1, 1), (3, -1), (5, -2), (2, 1)]
    a = rng.standard_normal((len(pairs), lmax + 1))
    b = tabs.back(tabs.forward(a, pairs).astype(np.float64), pairs, lmax + 1)
    for c, (p, q) in enumerate(pairs):
        l0 = max(abs(p), abs(q))
        assert (b[c, :l0] == 0).all()
        assert float(np.abs(b[c, l0:] - a[c, l0:]).max()) < 1e-13


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
FIELDS = {"POS": types.SimpleNamespace(mask="VIS", spin=0), "DEF": types.SimpleNamespace(mask="VIS", spin=1),
          "SHE": types.SimpleNamespace(mask="WHT", spin=2), "FLX": types.SimpleNamespace(mask="WHT", spin=3)}
SPINS = {("POS", "DEF", 0, 0): (0, 1), ("DEF", "DEF", 0, 0): (1, 1), ("DEF", "SHE", 0, 0): (1, 2), ("FLX", "POS", 0, 0): (3, 0),
         ("POS", "POS", 0, 0): (0, 0), ("SHE", "SHE", 0, 0): (2, 2)}
MKEYS = (("VIS", "VIS", 0, 0), ("VIS", "WHT", 0, 0), ("WHT", "WHT", 0, 0))
MSPINS = {k: (0, 0) for k in MKEYS}


def test_plan_of_other_spin_weights():
    plan = um.spice_plan(SPINS, MSPINS, FIELDS, exact_spin=True)
    assert plan.columns == dict(zip(SPINS, [(0, 2), (2, 4), (6, 4), (10, 2), (12, 1), (13, 4)]))
    assert plan.families.dtype == np.int32 and plan.families.shape == (17, 2) and plan.ncol == 17
    assert plan.families.tolist() == [[1, 0]] * 2 + [[1, 1]] * 2 + [[1, -1]] * 2 + [[1, 2]] * 2 + [[1, -2]] * 2 + [[3, 0]] * 2 + [[0, 0]] \
        + [[2, 2]] * 2 + [[2, -2]] * 2
    # the keys of spins {0, 2} keep their family beside their pair and stay on the family path
    assert plan.codes.tolist() == [-1] * 12 + [0, 1, 1, 2, 2] and plan.codes.dtype == np.int32
    # scalar masks: integer families as without exact_spin
    assert plan.mask_families.tolist() == [0, 0, 0] and plan.mask_codes is None and plan.ncol_mask == 3
    # (FLX, POS) asks for (WHT, VIS), found as (VIS, WHT): the second look-up of that mask; (VIS, VIS) is looked up three times
    assert plan.mask_col.tolist() == [0] * 2 + [0] * 4 + [1] * 4 + [1] * 2 + [0] + [2] * 4
    assert plan.ndamp.tolist() == [1] * 2 + [2] * 4 + [1] * 4 + [2] * 2 + [3] + [1] * 4
    assert plan.mask_key[("FLX", "POS", 0, 0)] == ("VIS", "WHT", 0, 0)
    # without the keyword: the "like spin 2" plan, unchanged
    old = um.spice_plan(SPINS, MSPINS, FIELDS)
    assert old.families.tolist() == [3, 3, 1, 1, 2, 2, 1, 1, 2, 2, 3, 3, 0, 1, 1, 2, 2] and old.codes is None and old.mask_codes is None
    for f in ("columns", "mask_key", "mask_columns"):
        assert getattr(old, f) == getattr(plan, f)
    np.testing.assert_array_equal(old.mask_col, plan.mask_col)
    np.testing.assert_array_equal(old.ndamp, plan.ndamp)


def test_plan_of_spins_0_and_2_does_not_change():
    spins = {k: s for k, s in SPINS.items() if set(s) <= {0, 2}}
    a, b = um.spice_plan(spins, MSPINS, FIELDS), um.spice_plan(spins, MSPINS, FIELDS, exact_spin=True)
    assert b.families.tolist() == [0, 1, 1, 2, 2] and b.codes is None and b.mask_codes is None
    for f in ("families", "mask_families", "mask_col", "ndamp"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
        assert getattr(a, f).dtype == getattr(b, f).dtype


def test_plan_with_masks_of_other_spin_weights():
    """A mask key with a spin outside {0, 2} gets pairs too; (s, 0) and (0, s) both run on T_{s,0}; a swapped four-column mask is read
    transposed as before."""
    fields = {"D": types.SimpleNamespace(mask="D", spin=1), "P": types.SimpleNamespace(mask="P", spin=0)}
    plan = um.spice_plan({("D", "D", 1, 0): (1, 1), ("D", "P", 1, 0): (1, 0)}, {("D", "D", 0, 1): (1, 1), ("P", "D", 0, 1): (0, 1)}, fields, exact_spin=True)
    assert plan.mask_families.tolist() == [[1, 1]] * 2 + [[1, -1]] * 2 + [[1, 0]] * 2 and plan.mask_codes.tolist() == [-1] * 6
    assert plan.families.tolist() == [[1, 1]] * 2 + [[1, -1]] * 2 + [[1, 0]] * 2 and plan.codes.tolist() == [-1] * 6
    assert plan.mask_col.tolist() == [0, 2, 1, 3, 4, 5]


def test_spin_pairs_and_column_transform_arguments():
    assert tr.spin_pairs((0, 0)) == [(0, 0)] and tr.spin_pairs((0, 3)) == [(3, 0)] * 2 == tr.spin_pairs((3, 0))
    assert tr.spin_pairs((1, 2)) == [(1, 2), (1, 2), (1, -2), (1, -2)]
    with pytest.raises(ValueError, match="pairs"):
        tr.cl2corr_columns(np.zeros((3, 4)), np.zeros((2, 2), dtype=np.int32), 3)
    with pytest.raises(ValueError, match="pairs"):
        tr.corr2cl_columns(np.zeros((3, 4)), np.zeros((3, 3), dtype=np.int32), 3)


# ---- the executor and the dict route on the reference tables ------------------------------------------------------------------------
N_DATA, N_MASK = 16, 24


def _ratio(xi_d, xi_num, num_col, ndamp, xi_den, den_col, x0):
    out = np.empty_like(xi_d)
    for c in range(xi_d.shape[0]):
        alpha = np.array(xi_num[num_col[c]])
        if xi_den is not None and den_col[c] >= 0:
            alpha = alpha / xi_den[den_col[c]]
        for _ in range(ndamp[c]):
            alpha = alpha * um.logistic(np.log10(abs(alpha)), x0=x0)
        out[c] = xi_d[c] / alpha
    return out


def _table_ops(tabs, calls):
    """forward / ratio / back of run_spice_plan in numpy on the reference tables; family codes are the pairs of corr_reference.FAMILIES."""
    def pairs_of(families):
        families = np.asarray(families)
        calls.append(families.shape)
        return [tuple(int(v) for v in p) for p in families] if families.ndim == 2 else [cr.FAMILIES[int(f)] for f in families]

    def forward(a, families, lmax):
        assert lmax == tabs.lmax
        return tabs.forward(a, pairs_of(families)).astype(np.float64)

    def back(xi, families, lmax, nl):
        assert lmax == tabs.lmax
        return tabs.back(xi, pairs_of(families), nl).astype(np.float64)

    return forward, _ratio, back


@pytest.fixture
def on_tables(monkeypatch):
    """The dict drivers on the same tables: the family kernels by corr_reference's sums, the column transforms by Tables."""
    x, w = np.polynomial.legendre.leggauss(N_MASK)
    tabs = xr.Tables(N_MASK - 1, x, w)

    def batch(fn, specs, lmax):
        assert lmax == tabs.lmax
        s = np.stack(specs)
        return (cr.cl2corr_truth(s, x) if fn.__name__ == "hx_cl2corr" else cr.corr2cl_truth(s, x, w)).astype(np.float64)

    monkeypatch.setattr(tr, "_batch", batch)
    monkeypatch.setattr(tr, "gauss_legendre", lambda n: np.polynomial.legendre.leggauss(n))
    monkeypatch.setattr(tr._lib, "load", lambda: types.SimpleNamespace(hx_cl2corr=types.SimpleNamespace(__name__="hx_cl2corr"),
                                                                        hx_corr2cl=types.SimpleNamespace(__name__="hx_corr2cl")))
    monkeypatch.setattr(tr, "cl2corr_columns", lambda a, families, lmax: tabs.forward(a, [tuple(p) for p in np.asarray(families).tolist()]).astype(np.float64))
    monkeypatch.setattr(tr, "corr2cl_columns", lambda xi, families, lmax: tabs.back(xi, [tuple(p) for p in np.asarray(families).tolist()], lmax + 1).astype(np.float64))
    return tabs


def _spectra(rng, scale=1.0):
    red = 1.0 / (1.0 + np.arange(N_DATA)) ** 2
    return {k: hx.Result(scale * rng.standard_normal(um._shape_of(s) + (N_DATA,)) * red, spin=s, axis=-1, ell=np.arange(N_DATA)) for k, s in SPINS.items()}


def _masks(tabs, rng):
    """Mask spectra whose correlation functions stay above 0.5: the damping factor is 1 in double, whatever the count."""
    out = {}
    for i, k in enumerate(MKEYS):
        xi = 0.6 + 0.1 * i + 0.3 * ((1 + tabs.x) / 2) ** (3 + i)
        out[k] = hx.Result(tabs.back(xi[None], [(0, 0)], N_MASK).astype(np.float64)[0], spin=(0, 0), axis=-1, ell=np.arange(N_MASK))
    return out


def _agree(got, want, what):
    """4 eps n_mask^2 max |C|: both routes run on the same long-double tables and round to double between the stages; a relative eps on
    xi comes back as 2 pi eps sum_k w_k |xi_k| <= eps n^2 max |C| (xi <= sum (2l + 1) / 4 pi |C_l| <= n^2 / 4 pi max |C|), once for each
    of the three roundings and once for the combinations either side."""
    for k in want:
        g, w = np.asarray(got[k].array), np.asarray(want[k].array)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        assert np.abs(g - w).max() <= 4 * np.finfo(np.float64).eps * N_MASK ** 2 * np.abs(w).max(), (what, k)
        np.testing.assert_array_equal(got[k].ell, want[k].ell)
        assert got[k].spin == want[k].spin


def test_batch_on_the_tables_is_the_dict_route(on_tables):
    tabs, rng = on_tables, np.random.default_rng(4)
    samples = {"a": _spectra(rng), "b": _spectra(rng, 3.0), "c": _spectra(rng)}
    masks = lambda: _masks(tabs, rng)  # noqa: E731  (naturalspice damps its masks in place: fresh ones per call)
    want = {i: um.naturalspice(s, masks(), FIELDS, exact_spin=True) for i, s in samples.items()}
    calls = []
    got = um.naturalspice_batch(samples, masks(), FIELDS, ops=_table_ops(tabs, calls), exact_spin=True)
    # masks: one call with families; data, each way: the columns that keep their family and the columns on their pair
    assert calls == [(3,), (15,), (36, 2), (15,), (36, 2)]
    chunked = um.naturalspice_batch(samples, masks(), FIELDS, ops=_table_ops(tabs, []), exact_spin=True, max_columns=17)
    for i in samples:
        _agree(got[i], want[i], i)
        for k in SPINS:
            np.testing.assert_array_equal(chunked[i][k].array, got[i][k].array)
    # what the keyword is for: "like spin 2" is another answer for the (1,1) key, the same for the keys of spins {0, 2}
    old = um.naturalspice_batch(samples, masks(), FIELDS, ops=_table_ops(tabs, []))
    k11, k22 = ("DEF", "DEF", 0, 0), ("SHE", "SHE", 0, 0)
    assert np.abs(old["a"][k11].array - got["a"][k11].array).max() > 1e-3 * np.abs(got["a"][k11].array).max()
    np.testing.assert_array_equal(old["a"][k22].array, got["a"][k22].array)
    np.testing.assert_array_equal(old["a"][("POS", "POS", 0, 0)].array, got["a"][("POS", "POS", 0, 0)].array)


def test_run_spice_plan_with_pairs_recovers_what_went_in(on_tables):
    """Mask correlation 1 (spectrum 4 pi at l = 0): the ratio is the identity, and every column comes back from l0 on; run_spice_plan
    alone, pairs through the ops hook."""
    tabs, rng = on_tables, np.random.default_rng(5)
    plan = um.spice_plan(SPINS, MSPINS, FIELDS, exact_spin=True)
    data = rng.standard_normal((2, plan.ncol, N_DATA))
    num = np.zeros((plan.ncol_mask, N_MASK))
    num[:, 0] = 4 * np.pi
    out = um.run_spice_plan(plan, data, num, N_MASK - 1, ops=_table_ops(tabs, []))
    for c, (a, b) in enumerate(plan.families.tolist()):
        l0 = max(abs(a), abs(b))
        assert (out[:, c, :l0] == 0).all()
        assert np.abs(out[:, c, l0:] - data[:, c, l0:]).max() < 1e-12, (c, a, b)


def test_footprint_correction_batch_passes_exact_spin(on_tables):
    tabs, rng = on_tables, np.random.default_rng(6)
    cls, mm = _spectra(rng), _masks(tabs, rng)
    calls = []
    got = jk.correct_footprint_naturalspice_batch({(1,): cls}, {(1,): mm}, _masks(tabs, rng), FIELDS, unmixed=True, ops=_table_ops(tabs, calls),
                                                  exact_spin=True)
    assert (12, 2) in calls and (5,) in calls
    want = um.naturalspice(cls, _masks(tabs, rng), FIELDS, exact_spin=True)
    _agree(got[(1,)], want, "footprint")
