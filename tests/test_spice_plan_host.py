"""The column plan of the batched NaturalSpice path (heracles_amd.unmixing.spice_plan, run_spice_plan, naturalspice_batch and
jackknife.correct_footprint_naturalspice_batch) WITHOUT a GPU: the plan is pure host logic, and the executor takes its three operations
as callables, here a numpy backend on the CPU oracle -- forward and back are oracle.cl2corr / oracle.corr2cl through the embedding of a
column in the four-column layout (family 0: TT; 1: EE = BB = a / 2; 2: EE = -BB = a / 2; 3: TE), the ratio is unmixing.logistic.  What is
tested is everything around the kernels: columns per spin case, their tables, which mask column divides which data column, the running
damping count of the reference's in-place quirk, the combinations either side, the cut at the data's band limit, the result dicts.
The same functions run on the kernels in tests/test_gpu_spice_batch.py."""

import os
import types

import numpy as np
import pytest

import heracles_amd as hx
from heracles_amd import jackknife as jk, unmixing as um
from corr_reference import dev_rel
from helpers import key_str

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"POS": types.SimpleNamespace(mask="VIS", spin=0), "SHE": types.SimpleNamespace(mask="WHT", spin=2)}
SPINS = {("POS", "POS", 0, 0): (0, 0), ("POS", "SHE", 0, 0): (0, 2), ("SHE", "SHE", 0, 0): (2, 2)}
MKEYS = (("VIS", "VIS", 0, 0), ("VIS", "WHT", 0, 0), ("WHT", "WHT", 0, 0))


# ---- plan contents ------------------------------------------------------------------------------------------------------------------
def test_columns_and_families_per_spin_case():
    plan = um.spice_plan(SPINS, {k: (0, 0) for k in MKEYS}, FIELDS)
    assert plan.columns == {("POS", "POS", 0, 0): (0, 1), ("POS", "SHE", 0, 0): (1, 2), ("SHE", "SHE", 0, 0): (3, 4)}
    assert plan.families.tolist() == [0, 3, 3, 1, 1, 2, 2] and plan.families.dtype == np.int32
    assert plan.mask_columns == {MKEYS[0]: (0, 1), MKEYS[1]: (1, 1), MKEYS[2]: (2, 1)}
    assert plan.mask_families.tolist() == [0, 0, 0]
    # a scalar mask divides every column of its data key
    assert plan.mask_col.tolist() == [0, 1, 1, 2, 2, 2, 2]
    assert plan.ndamp.tolist() == [1] * 7
    assert plan.ncol == 7 and plan.ncol_mask == 3
    assert plan.mask_key == dict(zip(SPINS, MKEYS))


def test_mask_sharing_and_running_damping_count():
    """Three bins of one field share one mask pair per bin pair; the fields' masks carry the bin indices of the data key.  Keys that
    look the same underlying mask key up count 1, 2, 3 in dict order -- the swapped look-up included."""
    fields = {"A": types.SimpleNamespace(mask="M", spin=0), "B": types.SimpleNamespace(mask="M", spin=0)}
    d = {("A", "A", 0, 1): (0, 0), ("A", "B", 0, 1): (0, 0), ("B", "A", 1, 0): (0, 0), ("B", "B", 1, 1): (0, 0)}
    m = {("M", "M", 0, 1): (0, 0), ("M", "M", 1, 1): (0, 0)}
    plan = um.spice_plan(d, m, fields)
    # (B, A, 1, 0) asks for (M, M, 1, 0), which is there only as (M, M, 0, 1): the same array, damped a third time
    assert plan.mask_col.tolist() == [0, 0, 0, 1]
    assert plan.ndamp.tolist() == [1, 2, 3, 1]
    assert plan.mask_key[("B", "A", 1, 0)] == ("M", "M", 0, 1)


def test_swapped_spin2_mask_is_read_transposed():
    """A 2 x 2 mask found only as (b, a, j, i) is looked up with its two spin axes swapped (_get_cl): data column (p, q) divides by mask
    column (q, p); an element-wise mask of a 0 x 2 key keeps its order."""
    fields = {"S": types.SimpleNamespace(mask="S", spin=2), "P": types.SimpleNamespace(mask="P", spin=0)}
    plan = um.spice_plan({("S", "S", 1, 0): (2, 2), ("S", "P", 1, 0): (2, 0)}, {("S", "S", 0, 1): (2, 2), ("P", "S", 0, 1): (0, 2)}, fields)
    assert plan.mask_col.tolist() == [0, 2, 1, 3, 4, 5]
    assert plan.mask_families.tolist() == [1, 1, 2, 2, 3, 3]
    direct = um.spice_plan({("S", "S", 0, 1): (2, 2)}, {("S", "S", 0, 1): (2, 2)}, fields)
    assert direct.mask_col.tolist() == [0, 1, 2, 3]


def test_missing_mask_raises_the_lookups_keyerror():
    with pytest.raises(KeyError, match="not found in Cls"):
        um.spice_plan(SPINS, {k: (0, 0) for k in MKEYS[:2]}, FIELDS)
    cls = {k: hx.Result(np.zeros(3), spin=(0, 0), axis=-1) for k in MKEYS[:2]}
    with pytest.raises(KeyError) as ours:
        um.spice_plan({("SHE", "SHE", 0, 0): (2, 2)}, {k: (0, 0) for k in MKEYS[:2]}, FIELDS)
    with pytest.raises(KeyError) as theirs:
        um._get_cl(("WHT", "WHT", 0, 0), cls)
    assert str(ours.value) == str(theirs.value)


def test_pack_and_unpack_are_the_dict_drivers_combinations():
    rng = np.random.default_rng(3)
    for spin in SPINS.values():
        a = rng.standard_normal(um._shape_of(spin) + (9,))
        cols = um._pack(a, spin)
        assert cols.shape == (um._ncols(spin), 9)
    a = rng.standard_normal((2, 2, 5))
    c = um._pack(a, (2, 2))
    np.testing.assert_array_equal(c, [a[0, 0] + a[1, 1], a[1, 0] - a[0, 1], -a[0, 1] - a[1, 0], a[0, 0] - a[1, 1]])
    b = rng.standard_normal((4, 5))
    u = um._unpack(b, (2, 2))
    # transforms.corr2cl: cl[0, 0], cl[1, 1] = EE, BB of (xi+, xi-) = (b0 + b3) / 2, (b0 - b3) / 2; cl[0, 1] = -EE, cl[1, 0] = BB of the second pair
    np.testing.assert_array_equal(u, [[(b[0] + b[3]) / 2, -(b[1] + b[2]) / 2], [(b[1] - b[2]) / 2, (b[0] - b[3]) / 2]])
    np.testing.assert_array_equal(um._unpack(b[:2], (0, 2)), [(b[0] + b[1]) / 2, (b[0] - b[1]) / 2])
    np.testing.assert_array_equal(um._pack(a[0], (0, 2)), [a[0, 0] + a[0, 1], a[0, 0] - a[0, 1]])


# ---- the executor on a numpy backend ------------------------------------------------------------------------------------------------
def _embed(col, family, n):
    """One column in the four-column layout of oracle.cl2corr / corr2cl, zero-padded to n."""
    out = np.zeros((n, 4))
    m = len(col)
    if family == 0:
        out[:m, 0] = col
    elif family == 1:
        out[:m, 1] = out[:m, 2] = col / 2
    elif family == 2:
        out[:m, 1] = col / 2
        out[:m, 2] = -col / 2
    else:
        out[:m, 3] = col
    return out


def _numpy_ops(oracle, calls):
    def forward(a, families, lmax):
        calls.append(("forward", a.shape[0]))
        return np.stack([oracle.cl2corr(_embed(c, f, lmax + 1), lmax)[:, f] for c, f in zip(a, families)])

    def ratio(xi_d, xi_num, num_col, ndamp, xi_den, den_col, x0):
        calls.append(("ratio", xi_d.shape[0]))
        out = np.empty_like(xi_d)
        with np.errstate(all="ignore"):
            for c in range(xi_d.shape[0]):
                alpha = np.array(xi_num[num_col[c]])
                if xi_den is not None and den_col[c] >= 0:
                    alpha = alpha / xi_den[den_col[c]]
                for _ in range(ndamp[c]):
                    alpha = alpha * um.logistic(np.log10(abs(alpha)), x0=x0)
                out[c] = xi_d[c] / alpha
        return out

    def back(xi, families, lmax, nl):
        calls.append(("back", xi.shape[0]))
        out = np.empty((xi.shape[0], nl))
        for c, f in enumerate(families):
            pol = np.zeros((lmax + 1, 4))
            pol[:, f] = xi[c]
            r = oracle.corr2cl(pol, lmax)
            # (xi in the Q+U or the Q-U column alone comes back as EE = +-BB = b / 2)
            out[c] = (r[:, 1] + r[:, 2] if f == 1 else r[:, 1] - r[:, 2] if f == 2 else r[:, f])[:nl]
        return out

    return forward, ratio, back


@pytest.fixture
def host_nodes(monkeypatch, oracle):
    monkeypatch.setattr(um, "gauss_legendre", oracle.gauss_legendre)
    return oracle


def test_naturalspice_batch_reference_vectors(host_nodes):
    """ns/default and ns/theta30 of reference_transforms.npz (data at lmax 256, masks at 512) within 8x the deviation of the dict drivers
    on the oracle, the bound of test_gpu_corr_stage.py::test_dict_drivers_and_naturalspice_reference_vectors; three samples (d, d, 2 d)
    through one batch and through chunks: equal samples agree to the bit, slots are not crossed, the masks are left alone."""
    oracle = host_nodes
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_transforms.npz"))
    Ld, Lm = 256, 512
    ell, ellm = np.arange(Ld + 1), np.arange(Lm + 1)
    d = {k: hx.Result(np.array(g[f"dict/d/{key_str(k)}"]), spin=s, axis=-1, ell=ell) for k, s in SPINS.items()}
    d2 = {k: hx.Result(2 * np.array(g[f"dict/d/{key_str(k)}"]), spin=s, axis=-1, ell=ell) for k, s in SPINS.items()}
    failures = []
    for tag, tm in (("default", None), ("theta30", 30.0)):
        m = {k: hx.Result(np.array(g[f"ns/m/{key_str(k)}"]), spin=(0, 0), axis=-1, ell=ellm) for k in MKEYS}
        calls = []
        res = um.naturalspice_batch({"a": d, "b": d, "c": d2}, m, FIELDS, theta_max=tm, ops=_numpy_ops(oracle, calls))
        # one forward over the mask columns, one over the data columns of all samples, one ratio, one way back
        assert calls == [("forward", 3), ("forward", 21), ("ratio", 21), ("back", 21)]
        assert list(res) == ["a", "b", "c"]
        for k in MKEYS:
            np.testing.assert_array_equal(m[k].array, g[f"ns/m/{key_str(k)}"])
        chunked = um.naturalspice_batch({"a": d, "b": d, "c": d2}, m, FIELDS, theta_max=tm, max_columns=7, ops=_numpy_ops(oracle, []))
        for k in d:
            ks = key_str(k)
            assert list(res["a"]) == list(d) and type(res["a"][k]) is hx.Result and res["a"][k].spin == SPINS[k]
            np.testing.assert_array_equal(res["a"][k].ell, ell)
            np.testing.assert_array_equal(res["a"][k].array, res["b"][k].array)
            np.testing.assert_array_equal(res["c"][k].array, 2 * res["a"][k].array)
            for i in res:
                np.testing.assert_array_equal(chunked[i][k].array, res[i][k].array)
            dev = dev_rel(res["a"][k].array, g[f"ns/{tag}/{ks}"])
            print(f"naturalspice_batch {tag} {ks}: max |d| / max |ref| {dev:.2e} (dict drivers on the oracle {g[f'ns/dev_{tag}/{ks}']:.2e})")
            if not dev <= 8 * g[f"ns/dev_{tag}/{ks}"]:
                failures.append(f"{tag} {ks}: {dev:.3e} > 8 * {g[f'ns/dev_{tag}/{ks}']:.3e}")
    assert not failures, "\n".join(failures)


def _jackknife_golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_jackknife.npz"))
    ks = lambda key: "|".join(str(k) for k in key)  # noqa: E731

    def spectra(group, keys_spins):
        return {k: hx.Result(np.array(g[f"{group}/{ks(k)}"]), spin=s, axis=-1, ell=np.arange(g[f"{group}/{ks(k)}"].shape[-1]))
                for k, s in keys_spins.items()}

    return g, ks, spectra


def test_footprint_correction_batch_reference_vectors(host_nodes):
    """mixed/out and unmixed/out of reference_jackknife.npz at that file's tolerance (test_gpu_jackknife.py), for two equal samples."""
    g, ks, spectra = _jackknife_golden()
    mspins = {k: (0, 0) for k in MKEYS}
    for tag, unmixed in (("mixed", False), ("unmixed", True)):
        cls, mls0, mljk = spectra("cls", SPINS), spectra("mls0", mspins), spectra("mljk", mspins)
        calls = []
        got = jk.correct_footprint_naturalspice_batch({(1,): cls, (2,): cls}, {(1,): mljk, (2,): mljk}, mls0, FIELDS, unmixed=unmixed,
                                                      ops=_numpy_ops(host_nodes, calls))
        assert list(got) == [(1,), (2,)]
        assert [c[0] for c in calls] == (["forward"] * 3 if not unmixed else ["forward"] * 2) + ["ratio", "back"]
        for k in SPINS:
            ref = g[f"{tag}/out/{ks(k)}"]
            assert list(got[(1,)]) == list(SPINS)
            np.testing.assert_allclose(np.asarray(got[(1,)][k].array), ref, rtol=1e-7, atol=1e-10 * np.abs(ref).max())
            np.testing.assert_array_equal(got[(2,)][k].array, got[(1,)][k].array)
            np.testing.assert_array_equal(got[(1,)][k].ell, np.arange(ref.shape[-1]))


@pytest.mark.parametrize("same_limit", [False, True])
def test_batch_results_carry_the_dtype_the_dict_drivers_leave(host_nodes, monkeypatch, same_limit):
    """The arrays come back with the dtype (metadata included) that the per-sample functions end with, whatever numpy decides about
    metadata in a division: compared against the dict drivers on the same stubs."""
    from heracles_amd import transforms as tr

    oracle = host_nodes

    def batch(fn, specs, lmax):
        f = oracle.cl2corr if fn.__name__ == "hx_cl2corr" else oracle.corr2cl
        return np.stack([f(s, lmax) for s in specs])

    monkeypatch.setattr(tr, "_batch", batch)
    monkeypatch.setattr(tr, "gauss_legendre", oracle.gauss_legendre)
    monkeypatch.setattr(tr._lib, "load", lambda: types.SimpleNamespace(hx_cl2corr=types.SimpleNamespace(__name__="hx_cl2corr"),
                                                                        hx_corr2cl=types.SimpleNamespace(__name__="hx_corr2cl")))
    g, ks, spectra = _jackknife_golden()
    mspins = {k: (0, 0) for k in MKEYS}
    cls, mls0, mljk = spectra("cls", SPINS), spectra("mls0", mspins), spectra("mljk", mspins)
    if same_limit:  # masks at the data's band limit and with metadata of their own, as the jackknife loop has them
        n = next(iter(cls.values())).array.shape[-1]
        mls0, mljk = ({k: hx.Result(np.array(r.array[:n]), spin=r.spin, axis=-1, ell=np.arange(n)) for k, r in mm.items()} for mm in (mls0, mljk))
        for r in list(mls0.values()) + list(mljk.values()):
            hx.update_metadata(r.array, nside=16)
    for r in cls.values():
        hx.update_metadata(r.array, bias=1.5)
    one = jk.correct_footprint_naturalspice(cls, {k: hx.Result(np.array(r.array), spin=r.spin, axis=-1, ell=r.ell) for k, r in mljk.items()}, mls0, FIELDS)
    got = jk.correct_footprint_naturalspice_batch({0: cls}, {0: mljk}, mls0, FIELDS, ops=_numpy_ops(oracle, []))[0]
    for k in SPINS:
        assert got[k].array.dtype == one[k].array.dtype and got[k].array.dtype.metadata == one[k].array.dtype.metadata, k
        np.testing.assert_allclose(got[k].array, one[k].array, rtol=1e-7, atol=1e-10 * np.abs(one[k].array).max())
        for f in ("spin", "axis"):
            assert getattr(got[k], f) == getattr(one[k], f)
        for f in ("ell", "lower", "upper", "weight"):
            np.testing.assert_array_equal(getattr(got[k], f), getattr(one[k], f))
