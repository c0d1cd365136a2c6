"""hx_gauss_cov_accumulate and heracles_amd.gausscov on the GPU against the numpy restatement (tests/gauss_cov_reference.py, pinned
on its own in tests/test_gauss_cov_host.py).

Kernel tests: a random symmetric Xi, mixed-sign spectra, lmax = 70 (71 multipoles: one more than a tile of 64 and a second chunk of
members).  Bound per element: |gpu - ref| <= 4 (n_b n_b' + 16) 2^-53 A, with A the absolute sum of the restatement and n_b the members
of bin b (1 unbinned).  The two-stage form adds the same terms as the direct sum, each rounded a few times, in n_b + n_b' + O(1)
additions: the bound is not tight.
Driver tests add the error of the table build: the (0,0) matrix is pinned to 1e-13 max |M| per element against the 3j oracle
(tests/test_gpu_mixmat.py::test_mixmat_vs_3j), which the restatement propagates through the same sums (``table_error``)."""

import itertools

import numpy as np
import pytest

import gauss_cov_reference as gr

pytestmark = pytest.mark.gpu

LMAX = 70
N = LMAX + 1
TABLE_TOL = 1e-13  # tests/test_gpu_mixmat.py::test_mixmat_vs_3j


@pytest.fixture(scope="module")
def hx():
    import heracles_amd

    heracles_amd.init(0)
    return heracles_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def case(hx, torch):
    """Table, spectra and their device copies; Xi as the kernel sees it (g00 / (2l' + 1))."""
    rng = np.random.default_rng(71)
    x = rng.standard_normal((N, N))
    g00 = 0.5 * (x + x.T) * (2 * np.arange(N) + 1)[None, :]
    xi = g00 / (2 * np.arange(N) + 1)[None, :]
    spec = rng.standard_normal((6, N)) * (1 + np.arange(N))[None, :] ** -0.5
    return dict(g00=g00, xi=xi, spec=spec, d_g00=torch.from_numpy(g00).cuda(), d_spec=torch.from_numpy(spec).cuda())


def plans(hx):
    ell = np.arange(N)
    return {
        "issue": hx.BinPlan(ell, np.array([2, 3, 4, 6, 10, 40, 71]), "2l+1"),  # l = 0, 1 in no bin, width-1 bins
        "short": hx.BinPlan(ell, np.array([1, 2, 9, 33, 60]), "2l+1"),          # the last edge lies below lmax
        "wide": hx.BinPlan(ell, np.array([0, 5, 70]), "l(l+1)"),                # a bin of 65 members: wider than a wave and a chunk
    }


#: one-term and two-term items, s0 == s1, row != col, a column that is no multiple of the block edge
def items_for(nbe):
    return [(0, 0, (0, 1, -1, -1)), (0, nbe, (2, 2, 3, 4)), (nbe, 3, (5, 0, 1, 1)), (nbe, nbe + 5, (4, 4, -1, -1))]


def reference(case, items, plan, rows, ldc):
    nbe = N if plan is None else plan.nbins
    ref, bound = np.zeros((rows, ldc)), np.zeros((rows, ldc))
    for row, col, s in items:
        terms = [(case["spec"][s[0]], case["spec"][s[1]])] + ([(case["spec"][s[2]], case["spec"][s[3]])] if s[2] >= 0 else [])
        c, A = gr.block(case["xi"], terms, plan)
        ref[row:row + nbe, col:col + nbe] += c
        bound[row:row + nbe, col:col + nbe] += gr.rounding_bound(A, N, plan)
    return ref, bound


def run(hx, torch, case, items, plan, cov):
    from heracles_amd.gausscov import _accumulate

    _accumulate(case["d_g00"], case["d_spec"], items, cov, plan)
    return cov.cpu().numpy()


def check(got, ref, bound, what):
    err = np.abs(got - ref)
    inside = bound > 0
    worst = (err[inside] / bound[inside]).max() if inside.any() else 0.0
    print(f"{what}: max |gpu - ref| = {err.max():.3e}, max |ref| = {np.abs(ref).max():.3e}, worst error / bound = {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


def test_unbinned(hx, torch, case):
    items = items_for(N)
    rows, ldc = 2 * N, 2 * N + 7  # ldc > N
    ref, bound = reference(case, items, None, rows, ldc)
    got = run(hx, torch, case, items, None, torch.zeros((rows, ldc), dtype=torch.float64, device="cuda"))
    check(got, ref, bound, "unbinned")
    assert np.all(got[bound == 0] == 0)


@pytest.mark.parametrize("name", ["issue", "short", "wide"])
def test_binned(hx, torch, case, name):
    plan = plans(hx)[name]
    nb = plan.nbins
    sizes = gr.bin_sizes(N, plan)
    if name == "issue":
        assert plan.which[0] == plan.which[1] == -1 and sizes.min() == 1
    if name == "short":
        assert plan.which[-1] == -1
    if name == "wide":
        assert sizes.max() > 64
    items = items_for(nb)
    rows, ldc = 2 * nb, 2 * nb + 7
    ref, bound = reference(case, items, plan, rows, ldc)
    got = run(hx, torch, case, items, plan, torch.zeros((rows, ldc), dtype=torch.float64, device="cuda"))
    check(got, ref, bound, f"binned ({name})")
    assert np.all(got[bound == 0] == 0)


@pytest.mark.parametrize("binned", [False, True])
def test_adds_into_cov_and_touches_nothing_else(hx, torch, case, binned):
    plan = plans(hx)["issue"] if binned else None
    nbe = plan.nbins if binned else N
    items = items_for(nbe)
    rows, ldc = 2 * nbe + 1, 2 * nbe + 7
    ref, bound = reference(case, items, plan, rows, ldc)
    rng = np.random.default_rng(5)
    pre = np.where(bound > 0, rng.standard_normal((rows, ldc)), np.nan)
    got = run(hx, torch, case, items, plan, torch.from_numpy(pre).cuda())
    inside = bound > 0
    want = pre[inside] + ref[inside]
    # one more addition: half an ulp of the sum
    assert np.all(np.abs(got[inside] - want) <= bound[inside] + 2.0**-52 * np.abs(want))
    assert np.array_equal(got[~inside].view(np.uint64), pre[~inside].view(np.uint64))


@pytest.mark.parametrize("binned", [False, True])
def test_bitwise_repeatable_and_independent_of_the_call(hx, torch, case, binned):
    plan = plans(hx)["wide"] if binned else None
    nbe = plan.nbins if binned else N
    items = items_for(nbe)
    shape = (2 * nbe, 2 * nbe + 7)

    def fresh():
        return torch.zeros(shape, dtype=torch.float64, device="cuda")

    one = run(hx, torch, case, items, plan, fresh())
    two = run(hx, torch, case, items, plan, fresh())
    assert np.array_equal(one.view(np.uint64), two.view(np.uint64))
    # the same items over two calls, in another order: other slots of the folded table, the same bits
    cov = fresh()
    run(hx, torch, case, items[2:][::-1], plan, cov)
    split = run(hx, torch, case, items[:2][::-1], plan, cov)
    assert np.array_equal(one.view(np.uint64), split.view(np.uint64))


def test_errors_leave_cov_untouched(hx, torch, case):
    lib = hx._lib.load()
    ptr = hx._lib.ptr
    plan = plans(hx)["issue"]
    nb = plan.nbins
    which = np.ascontiguousarray(plan.which, dtype=np.int32)
    w, norm = np.ascontiguousarray(plan.w, dtype=float), np.ascontiguousarray(plan.norm, dtype=float)
    rows, ldc = 2 * N, 2 * N
    pre = np.random.default_rng(6).standard_normal((rows, ldc))
    cov = torch.from_numpy(pre).cuda()
    nspec = case["spec"].shape[0]

    def items(*blocks):
        arr = (hx._lib.CovItem * len(blocks))()
        for n, (row, col, s) in enumerate(blocks):
            arr[n].row, arr[n].col = row, col
            arr[n].s[:] = s
        return arr

    good = items((0, 0, (0, 1, 2, 3)))
    g, s, c = ptr(case["d_g00"]), ptr(case["d_spec"]), ptr(cov)

    def call(g00=g, spec=s, nbins=0, bins=(None, None, None), it=good, nitem=1, out=c, ld=ldc, nsp=nspec):
        return lib.hx_gauss_cov_accumulate(LMAX, g00, nsp, spec, nbins, *[None if b is None else ptr(b) for b in bins], nitem, it, out, ld)

    binned = dict(nbins=nb, bins=(which, w, norm))
    bad_which = which.copy()
    bad_which[7] = nb
    bad_norm = norm.copy()
    bad_norm[2] = 0.0
    cases = {
        "null table": call(g00=None), "null spectra": call(spec=None), "null cov": call(out=None), "null items": call(it=None),
        "null bins": call(nbins=nb, bins=(which, None, norm)),
        "spectrum == nspec": call(it=items((0, 0, (nspec, 1, -1, -1)))),
        "negative spectrum": call(it=items((0, 0, (-1, 1, -1, -1)))),
        "second term out of range": call(it=items((0, 0, (0, 1, 2, nspec)))),
        "second item bad": call(it=items((0, 0, (0, 1, -1, -1)), (N, 0, (0, nspec + 3, -1, -1))), nitem=2),
        "block leaves ldc": call(it=items((0, N + 1, (0, 1, -1, -1)))),
        "binned block leaves ldc": call(it=items((0, ldc - nb + 1, (0, 1, -1, -1))), **binned),
        "negative row": call(it=items((-1, 0, (0, 1, -1, -1)))),
        "overlapping blocks": call(it=items((0, 0, (0, 1, -1, -1)), (N - 1, N - 1, (0, 1, -1, -1))), nitem=2),
        "which out of range": call(nbins=nb, bins=(bad_which, w, norm)),
        "zero norm": call(nbins=nb, bins=(which, w, bad_norm)),
        "negative lmax": lib.hx_gauss_cov_accumulate(-1, g, nspec, s, 0, None, None, None, 1, good, c, ldc),
    }
    for what, rc in cases.items():
        assert rc < 0, what
        assert lib.hx_last_error(), what
    assert np.array_equal(cov.cpu().numpy().view(np.uint64), pre.view(np.uint64))
    # and the same objects are fine in a good call
    assert call() == 0 and call(**binned) == 0


def test_flops_are_counted_and_scratch_is_released(hx, torch, case):
    plan = plans(hx)["issue"]
    hx._lib.executed_flops(reset=True)
    run(hx, torch, case, items_for(plan.nbins), plan, torch.zeros((2 * plan.nbins, 2 * plan.nbins + 7), dtype=torch.float64, device="cuda"))
    _, valu = hx._lib.executed_flops(reset=True)
    members = int((plan.which >= 0).sum())
    assert valu >= 2 * 7 * members * N  # the fold alone: six named spectra and the ones row
    hx.release_caches()
    got = run(hx, torch, case, items_for(N), None, torch.zeros((2 * N, 2 * N + 7), dtype=torch.float64, device="cuda"))
    assert np.isfinite(got).all()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
NSIDE, L = 16, 24


def make_cls(hx, rng, units, L, positive=False):
    """Spectra of mixed sign; ``positive``: small cross-spectra and positive auto-spectra (a covariance with a positive diagonal)."""
    cls = {}
    for (a, i), (b, j) in itertools.combinations_with_replacement(units, 2):
        da, db = (1 if a == "P" else 2), (1 if b == "P" else 2)
        arr = (0.1 if positive else 1.0) * rng.standard_normal((da, db, L + 1)) / (1 + np.arange(L + 1))
        if (a, i) == (b, j):
            arr = arr + arr.transpose(1, 0, 2)
            if positive:
                arr = arr + np.eye(da)[:, :, None] * (2.0 / (1 + np.arange(L + 1)))
        shape = tuple(d for d, n in ((da, a), (db, b)) if n != "P") + (L + 1,)
        cls[a, b, i, j] = hx.Result(np.ascontiguousarray(arr.reshape(shape)), spin=(0 if a == "P" else 2, 0 if b == "P" else 2))
    return cls


@pytest.fixture(scope="module")
def survey(hx, oracle):
    """Two bins of (Positions, Shears), four different smooth masks, their product spectra from the GPU."""
    fields = {"P": hx.Positions(None, mask="V"), "G": hx.Shears(None, mask="W")}
    masks = gr.smooth_masks(oracle, NSIDE, 4, 3, 11)
    mask_maps = {("V", 1): masks[0], ("V", 2): masks[1], ("W", 1): masks[2], ("W", 2): masks[3]}
    cls = make_cls(hx, np.random.default_rng(12), [("P", 1), ("P", 2), ("G", 1), ("G", 2)], L)
    hx.update_metadata(cls["P", "P", 1, 1].array, bias=0.125)
    mask_cls = hx.mask_product_cls(mask_maps, fields, list(cls), lmax=12)
    return dict(fields=fields, mask_maps=mask_maps, cls=cls, mask_cls=mask_cls, tables={})


def test_mask_product_cls_matches_the_oracle(hx, oracle, survey):
    maps, mask_cls = survey["mask_maps"], survey["mask_cls"]
    assert all(k == hx.table_key(k) for k in mask_cls)
    # every table the data vector needs: all pairs of pairs of the four masks that occur as (m_a m_c, m_b m_d)
    for key in list(mask_cls)[::7]:
        (k1, k2), (k3, k4) = key
        alm = oracle.map2alm(np.stack([maps[k1] * maps[k2], maps[k3] * maps[k4]]), NSIDE, 12)
        ref = oracle.alm2cl(alm[0], alm[1])
        assert np.abs(mask_cls[key] - ref).max() <= 1e-10 * np.abs(ref).max(), key
    # keys bound to one map object share their products: the spectra are equal bit for bit
    same = {("V", 1): maps["V", 1], ("W", 1): maps["V", 1]}
    fields = {"P": hx.Positions(None, mask="V"), "G": hx.Positions(None, mask="W")}
    got = hx.mask_product_cls(same, fields, lmax=12)
    first = next(iter(got.values()))
    assert len(got) > 1 and all(np.array_equal(v, first) for v in got.values())


@pytest.mark.parametrize("binned", [False, True])
def test_driver_against_the_reference(hx, oracle, survey, binned):
    plan = hx.BinPlan(np.arange(L + 1), np.array([2, 3, 5, 9, 17, L + 1]), "2l+1") if binned else None
    kw = dict(bins=np.array([2, 3, 5, 9, 17, L + 1]), weights="2l+1") if binned else {}
    got = hx.gaussian_covariance_coupled(survey["cls"], survey["mask_cls"], survey["fields"], **kw)
    assert got.is_cuda and got.dtype.is_floating_point and got.element_size() == 8
    got = got.cpu().numpy()

    def lookup(k1, k2, k3, k4):
        return hx.table_key(((k1, k2), (k3, k4)), survey["mask_cls"])

    ref, A, E = gr.covariance(oracle, survey["cls"], lookup, survey["fields"], plan, tables=survey["tables"], table_error=True)
    assert got.shape == ref.shape
    sizes = gr.bin_sizes(L + 1, plan).astype(float)
    members = np.tile(sizes, ref.shape[0] // len(sizes))
    bound = 4 * (np.outer(members, members) + 16) * 2.0**-53 * A
    bound = bound + 2 * TABLE_TOL * E  # twice: the folds read Xi_{l'l} for Xi_{ll'}
    check(got, ref, bound, f"driver ({'binned' if binned else 'unbinned'})")
    assert np.array_equal(got, got.T)


def test_driver_full_sky_is_gaussian_covariance_over_2l_plus_1(hx, survey):
    cls, fields = survey["cls"], survey["fields"]
    full = np.zeros(2 * L + 1)
    full[0] = 4 * np.pi
    tables = hx.covariance_requests(cls, fields).tables
    got = hx.gaussian_covariance_coupled(cls, {t: full for t in tables}, fields).cpu().numpy()
    want = hx.flatten(hx.gaussian_covariance(cls), order=list(cls))
    want = want / np.tile(2 * np.arange(L + 1) + 1, want.shape[0] // (L + 1))[None, :]
    # the table is the identity to 1e-13 per element (tests/test_gpu_mixmat.py::test_mixmat_shapes_and_identities); an unbinned element
    # is one table entry times two products of spectra, each at most smax^2, formed with a handful of roundings
    bs = hx.bias(cls)
    smax = max(np.abs(np.asarray(res.array) + bs[key]).max() for key, res in cls.items())
    err = np.abs(got - want).max()
    print(f"full sky: max |gpu - gaussian_covariance / (2l + 1)| = {err:.3e}, smax^2 = {smax**2:.3e}")
    assert err <= (1e-13 + 16 * 2.0**-53) * 2 * smax**2


def test_as_dict_blocks_are_slices_of_the_dense_matrix(hx, survey):
    cls, fields = survey["cls"], survey["fields"]
    edges = np.array([2, 3, 5, 9, 17, L + 1])
    plan = hx.BinPlan(np.arange(L + 1), edges, "2l+1")
    for kw, nbe in ((dict(), L + 1), (dict(bins=edges, weights="2l+1"), plan.nbins)):
        dense = hx.gaussian_covariance_coupled(cls, survey["mask_cls"], fields, **kw).cpu().numpy()
        blocks = hx.gaussian_covariance_coupled(cls, survey["mask_cls"], fields, as_dict=True, **kw)
        keys = list(cls)
        assert list(blocks) == [(a1, b1, a2, b2, i1, j1, i2, j2) for (a1, b1, i1, j1), (a2, b2, i2, j2) in itertools.combinations_with_replacement(keys, 2)]
        start, n = {}, 0
        for key in keys:
            start[key] = n
            n += np.asarray(cls[key].array).size // (L + 1) * nbe
        for (k1, k2), res in zip(itertools.combinations_with_replacement(keys, 2), blocks.values()):
            d1, d2 = np.asarray(cls[k1].array).shape[:-1], np.asarray(cls[k2].array).shape[:-1]
            arr = np.asarray(res.array)
            assert arr.shape == d1 + d2 + (nbe, nbe) and res.axis == (arr.ndim - 2, arr.ndim - 1)
            assert res.spin == tuple(cls[k1].spin) + tuple(cls[k2].spin)
            n1, n2 = int(np.prod(d1, dtype=int)), int(np.prod(d2, dtype=int))
            sl = dense[start[k1]:start[k1] + n1 * nbe, start[k2]:start[k2] + n2 * nbe].reshape(n1, nbe, n2, nbe).transpose(0, 2, 1, 3)
            assert np.array_equal(arr.reshape(n1, n2, nbe, nbe), sl)
            if kw:
                assert all(np.array_equal(e, plan.ell) for e in res.ell)
                assert all(np.array_equal(e, plan.lower) for e in res.lower) and all(np.array_equal(e, plan.upper) for e in res.upper)
        assert hx.flatten(blocks, order=keys).shape == dense.shape
        assert np.array_equal(hx.flatten(blocks, order=keys), dense)


def test_dense_result_is_a_shrinkage_target(hx, survey):
    fields = survey["fields"]
    rng = np.random.default_rng(13)
    cls = make_cls(hx, rng, [("P", 1), ("P", 2), ("G", 1), ("G", 2)], L, positive=True)
    dense = hx.gaussian_covariance_coupled(cls, survey["mask_cls"], fields)
    blocks = hx.gaussian_covariance_coupled(cls, survey["mask_cls"], fields, as_dict=True)
    assert float(dense.diagonal().min()) > 0
    cls1 = {}
    for k in range(6):
        cls1[(k,)] = {key: hx.Result(np.asarray(res.array) * (1 + 0.1 * rng.standard_normal(np.shape(res.array))), spin=res.spin) for key, res in cls.items()}
    lam_dense = hx.shrinkage_factor(cls1, dense)
    lam_dict = hx.shrinkage_factor(cls1, blocks)
    assert np.isfinite(lam_dense) and abs(lam_dense - lam_dict) <= 1e-12 * abs(lam_dict)
    jk = hx.jackknife_covariance(cls1)
    shrunk = hx.shrink(jk, blocks, lam_dense)
    assert set(shrunk) == set(jk)


def test_driver_errors_name_the_key(hx, survey):
    cls, fields, mask_cls = survey["cls"], survey["fields"], survey["mask_cls"]
    with pytest.raises(ValueError, match="no mask"):
        hx.gaussian_covariance_coupled(cls, mask_cls, {"P": fields["P"], "G": hx.Shears(None)})
    short = dict(cls)
    short["P", "P", 1, 1] = hx.Result(np.zeros(L), spin=(0, 0))
    with pytest.raises(ValueError, match="multipoles"):
        hx.gaussian_covariance_coupled(short, mask_cls, fields)
    missing = dict(mask_cls)
    gone = sorted(missing)[3]
    del missing[gone]
    with pytest.raises(KeyError) as info:
        hx.gaussian_covariance_coupled(cls, missing, fields)
    assert str(gone[0][0]) in str(info.value)


def test_monte_carlo_on_the_gpu(hx, torch, oracle):
    """synalm_components -> Plan.alm2map -> mask -> map2alm(niter=3) -> alm2cl against the driver: the conditions of the host check."""
    c = gr.MC
    nside, lf, Lm, n = c["nside"], c["lmax_field"], c["L"], c["nreal"]
    ma, mb = gr.smooth_masks(oracle, nside, 2, c["mask_lmax"], c["seed"])
    (caa, cab), (_, cbb) = c["spectra"]
    packed = torch.from_numpy(np.array([caa, cab, cbb])[:, None] * np.ones(lf + 1)).cuda()
    synth, analyse = hx.Plan(nside, lf), hx.Plan(nside, Lm)
    per = 4  # realisations per batch: eight components
    masks = torch.from_numpy(np.stack([ma, mb] * per)).cuda()
    alms = torch.empty((2 * per, synth.nlm), dtype=torch.complex128, device="cuda")
    pairs = [p for k in range(per) for p in ((2 * k, 2 * k), (2 * k, 2 * k + 1), (2 * k + 1, 2 * k + 1))]
    samples = np.empty((n, 3 * (Lm + 1)))
    for r0 in range(0, n, per):
        for k in range(per):
            hx.synalm_components(packed, 2, seed=c["seed"], realisation=r0 + k, out=alms[2 * k:2 * k + 2])
        maps = synth.alm2map(alms, 0) * masks
        pseudo = analyse.map2alm(maps, 0, niter=c["niter"])
        cl = hx.alm2cl_pairs([pseudo[k] for k in range(2 * per)], pairs, Lm)
        samples[r0:r0 + per] = cl.reshape(per, 3 * (Lm + 1))
    synth.close()
    analyse.close()
    fields = {"A": hx.Positions(None, mask="VA"), "B": hx.Positions(None, mask="VB")}
    one = np.ones(Lm + 1)
    cls = {("A", "A", 1, 1): hx.Result(caa * one, spin=(0, 0)), ("A", "B", 1, 1): hx.Result(cab * one, spin=(0, 0)),
           ("B", "B", 1, 1): hx.Result(cbb * one, spin=(0, 0))}
    mask_cls = hx.mask_product_cls({("VA", 1): ma, ("VB", 1): mb}, fields, list(cls), lmax=12, niter=c["niter"])
    cov = hx.gaussian_covariance_coupled(cls, mask_cls, fields).cpu().numpy()
    keep = np.flatnonzero(np.tile(np.arange(Lm + 1), 3) >= c["lmin"])
    zmax, zrms, diag = gr.z_statistic(samples, cov, keep)
    print(f"Monte Carlo, GPU, n = {n}: max |z| = {zmax:.2f}, rms z = {zrms:.3f}, mean diagonal ratio {diag:.4f}")
    assert zmax <= 6, zmax
    assert 0.8 <= zrms <= 1.2, zrms
