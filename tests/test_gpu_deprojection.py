"""Template deprojection on the device against the numpy restatement of the rule (tests/deprojection_reference.py).
u = 2^-53 throughout.

Gram.  Every element obeys |G - G_ref| <= K u A_ij, A_ij = sum |x_i x_j|, with K derived from the kernel's summation: a product
x_i(p) x_j(p) enters the accumulator of its slab in one step of the matrix instruction and then passes through at most one rounding
per later product of the slab -- a slab of S inner elements is a chain of at most S additions, however the instruction orders its
four products --, one more for the product itself (counted although the instruction fuses it), then the nslab - 1 additions of the
slab reduction (the first slab is added to 0.0 exactly), and the two mask products (1 + d)^2 of its operands:
    K = min(S, ncomp npix) + 1 + (nslab - 1) + 2,   S = max(8192, ceil(ncomp npix / ceil(2048 / tiles))) rounded up to 32, or HX_DEPROJ_SLAB
(first order in u; K u < 2e-12 here, the second-order terms are below 1e-8 of the bound).  Measured worst error / bound: 0.058 (npix 12, K = 27); 0.0067 at npix 12288.

Apply.  |out - ref| <= (ntemp + 3) u (|d| + |v| sum |alpha_i t_i|) per pixel: one rounding per product, ntemp additions, the mask
product, the subtraction.  The reference runs the same operations in the same order, so the measured error is 0.

deproject_templates.  With kappa = cond of the unit-diagonal matrix (asserted <= 100 by the reference before any comparison),
k templates, scaled amplitudes a~ = D^(1/2) alpha, |dG~_ij| <= K u (A_ij <= sqrt(G_ii G_jj)), |dr~_i| <= K u |d|,
|G~^+| <= kappa, |a~| <= sqrt(kappa) |d|, and c = 64 k u kappa for eigh and the host products (tests/test_deprojection_host.py):
    |da~| <= kappa (sqrt(k) + k sqrt(kappa)) K u |d| + c sqrt(kappa) |d|
    |cleaned - ref|(p) <= |da~| |f~(p)|_2 + (k + 3) u B(p),   f~_i = f_i / sqrt(G_ii),  B as in the apply bound,
and F^T d_c, evaluated by the Gram kernel on the cleaned map, is within K u A_i + sqrt(G_ii) (|E|_2 + c |d|) of zero, E the
per-pixel bound above.  Measured worst ratios: cleaned 6.2e-05, F^T d_c 5.7e-06.

hx_alm_apply_cl: within 3 u sum |cl alm| per coefficient and part (two products, one sum, or their fused form).

deprojection_bias against the reference formula with the oracle's transforms at nside 16, lmax 24: the transform parity pinned by
tests/test_gpu_sht.py is max |delta| <= 1e-11 max |alm| for the plain transforms and 1e-10 for the iterated analysis.  The alms of
f carry e_f = 1e-10; those of g pass a plain analysis, a synthesis (each 1e-11, carried on through the following transforms with
at most sqrt(npix) from the change of norm) and the iterated analysis: e_g = 1e-10 + 2 sqrt(npix) 1e-11.  A term w PCL_l(x, y) has
|PCL_l| <= max |x| max |y|, so the first two sums move by at most (e_f + e_g) T2 and the third by (2 e_f + e_g) T4, T2 and T4 the
sums of |w| max |x| max |y| the reference returns.  Measured worst error / bound: 2.7e-08.
The Monte Carlo run is the host test's setup through the device pipeline, 600 realisations batched as one stack per field:
max |z| <= 6 and 0.8 <= rms z <= 1.2 over l >= 2.  Measured: max |z| = 2.41, rms z = 0.983 (bias set to zero: max |z| = 22.2)."""

import ctypes

import numpy as np
import pytest

import deprojection_reference as dr

pytestmark = pytest.mark.gpu

U = 2.0**-53
HX_ERR_ARG = -1

# (npix, ncomp, ntemp, nmap, mask, where, slab hook of the second run)
GRAM_CASES = [
    (12, 1, 1, 1, False, "host", 32),
    (12, 2, 3, 2, True, "device", 32),
    (108, 1, 15, 1, True, "host", 64),
    (108, 2, 16, 1, False, "device", 96),
    (768, 1, 63, 1, True, "device", 160),
    (768, 2, 64, 1, True, "host", 500),
    (3072, 1, 70, 3, True, "device", 1000),
    (3072, 2, 0, 2, False, "device", 2500),
    (3072, 2, 3, 2, True, "host", 2500),
    (12288, 1, 70, 3, True, "device", 5000),
    (12288, 2, 15, 1, False, "device", 10000),
    (12288, 1, 0, 1, True, "host", 5000),
]


def slab_of(Q, n, hook=None):
    """The slab length and count of hx_deproject_gram (include/hxsht.h)."""
    nt = -(-n // 64)
    tiles = nt * (nt + 1) // 2
    target = -(-2048 // tiles)
    S = max(8192, -(-Q // target)) if hook is None else hook
    S = -(-S // 32) * 32
    return S, -(-Q // S)


def gram_K(Q, n, hook=None):
    S, nslab = slab_of(Q, n, hook)
    return min(S, Q) + 1 + (nslab - 1) + 2


def _data(npix, ncomp, ntemp, nmap, mask, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((ntemp, ncomp, npix)) * rng.uniform(0.5, 20.0, (ntemp, 1, 1)) + rng.uniform(-1, 1, (ntemp, 1, 1))
    d = rng.standard_normal((nmap, ncomp, npix))
    v = rng.uniform(0.0, 1.0, npix) if mask else None
    return t, d, v


def _place(arrays, where):
    import torch

    if where == "host":
        return [np.ascontiguousarray(a) for a in arrays]
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _guarded(n, where):
    """(buffer of NaN, the view of n doubles inside it, the buffer's bits)."""
    import torch

    if where == "host":
        buf = np.full(n + 64, np.nan)
        return buf, buf[32 : 32 + n], buf.view(np.int64).copy()
    buf = torch.full((n + 64,), float("nan"), dtype=torch.float64, device="cuda")
    return buf, buf[32 : 32 + n], buf.view(torch.int64).clone()


def _guards_intact(buf, n, bits):
    import torch

    if isinstance(buf, np.ndarray):
        now = buf.view(np.int64)
        return np.array_equal(now[:32], bits[:32]) and np.array_equal(now[32 + n :], bits[32 + n :])
    now = buf.view(torch.int64)
    return bool(torch.equal(now[:32], bits[:32]) and torch.equal(now[32 + n :], bits[32 + n :]))


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _ptrs(cols):
    """A host array of the addresses of the columns; None gives a null pointer."""
    import heracles_amd as hx

    arr = (ctypes.c_void_p * max(len(cols), 1))()
    for i, c in enumerate(cols):
        arr[i] = None if c is None else hx._lib.ptr(c).value
    return arr


def _gram_rc(tcols, mcols, mask, out, npix=None, ncomp=None, ntemp=None, nmap=None):
    """hx_deproject_gram called directly: its return code."""
    import heracles_amd as hx

    hx._lib.ensure_init()
    first = (list(mcols) + list(tcols))[0]
    return hx._lib.load().hx_deproject_gram(first.shape[1] if npix is None else npix, first.shape[0] if ncomp is None else ncomp,
                                            len(tcols) if ntemp is None else ntemp, _ptrs(tcols), len(mcols) if nmap is None else nmap,
                                            _ptrs(mcols), hx._lib.ptr(mask), hx._lib.ptr(out))


def _apply_rc(tcols, mask, mcols, alpha, ocols, ncomp=None):
    import heracles_amd as hx

    hx._lib.ensure_init()
    first = mcols[0]
    return hx._lib.load().hx_deproject_apply(first.shape[1], first.shape[0] if ncomp is None else ncomp, len(tcols), _ptrs(tcols),
                                             hx._lib.ptr(mask), len(mcols), _ptrs(mcols), hx._lib.ptr(alpha), _ptrs(ocols))


def _last_error():
    import heracles_amd as hx

    return hx._lib.load().hx_last_error().decode()


_gram_refs = {}


def _gram_ref(case):
    """(t, d, v, G_ref, A) of a case, computed once."""
    if case not in _gram_refs:
        npix, ncomp, ntemp, nmap, mask = case[:5]
        t, d, v = _data(npix, ncomp, ntemp, nmap, mask, 1000 + npix + 7 * ntemp + ncomp)
        _gram_refs[case] = (t, d, v) + dr.gram(t, d, v)
    return _gram_refs[case]


@pytest.mark.parametrize("case", GRAM_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_gram(case, monkeypatch):
    npix, ncomp, ntemp, nmap, mask, where, hook = case
    t, d, v, want, A = _gram_ref(case)
    n, Q = ntemp + nmap, ncomp * npix
    tc, mc = _place(list(t), where), _place(list(d), where)
    vm = None if v is None else _place([v], where)[0]
    monkeypatch.delenv("HX_DEPROJ_SLAB", raising=False)
    buf, view, bits = _guarded(n * n, where)
    assert _gram_rc(tc, mc, vm, view) == 0, _last_error()
    assert _guards_intact(buf, n * n, bits)
    got = _host(view).reshape(n, n).copy()
    K = gram_K(Q, n)
    ratio = float((np.abs(got - want) / (K * U * A)).max())
    assert np.array_equal(got, got.T)
    buf2, view2, _ = _guarded(n * n, where)
    assert _gram_rc(tc, mc, vm, view2) == 0
    assert _host(view2).tobytes() == _host(view).tobytes()  # two runs: the same bits
    # another slab length: at least three slabs at the largest size, the last one ragged
    S, nslab = slab_of(Q, n, hook)
    if npix == 12288:
        assert nslab >= 3 and Q % S != 0
    monkeypatch.setenv("HX_DEPROJ_SLAB", str(hook))
    assert _gram_rc(tc, mc, vm, view2) == 0
    other = _host(view2).reshape(n, n).copy()
    K2 = gram_K(Q, n, hook)
    ratio2 = float((np.abs(other - want) / (K2 * U * A)).max())
    print(f"gram {case}: K = {K}, worst error / bound {ratio:.3g}; slab {S} x {nslab}: K = {K2}, {ratio2:.3g}")
    assert ratio <= 1 and ratio2 <= 1
    assert np.array_equal(other, other.T)
    assert np.all(np.abs(other - got) <= (K + K2) * U * A)


APPLY_CASES = [
    (12, 1, 1, 1, False, "host"),
    (108, 2, 3, 2, True, "device"),
    (768, 1, 16, 1, True, "host"),
    (3072, 2, 64, 1, True, "device"),
    (3072, 1, 5, 9, True, "device"),  # more maps than one pass takes
    (12288, 1, 70, 3, False, "device"),
    (12288, 2, 0, 2, True, "device"),
]


@pytest.mark.parametrize("case", APPLY_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_apply(case):
    npix, ncomp, ntemp, nmap, mask, where = case
    t, d, v = _data(npix, ncomp, ntemp, nmap, mask, 2000 + npix + ntemp)
    alpha = np.random.default_rng(npix + ntemp).standard_normal((nmap, ntemp))
    want, B = dr.apply(d, t, v, alpha)
    tc, mc = _place(list(t), where), _place(list(d), where)
    vm = None if v is None else _place([v], where)[0]
    Q = ncomp * npix
    outs, views, guards = [], [], []
    for m in range(nmap):
        buf, view, bits = _guarded(Q, where)
        outs.append((buf, bits))
        views.append(view.reshape(ncomp, npix))
    al = alpha if ntemp else None
    assert _apply_rc(tc, vm, mc, al, views) == 0, _last_error()
    got = np.stack([_host(x) for x in views])
    assert all(_guards_intact(buf, Q, bits) for buf, bits in outs)
    ratio = float((np.abs(got - want) / np.maximum((ntemp + 3) * U * B, 1e-300)).max())
    print(f"apply {case}: worst error / bound {ratio:.3g}")
    assert ratio <= 1
    # in place: the same bits
    assert _apply_rc(tc, vm, mc, al, mc) == 0, _last_error()
    assert np.stack([_host(x) for x in mc]).tobytes() == got.tobytes()


# ---- deproject_templates end to end ----------------------------------------------------------------------------------------------------
def _smooth_case(oracle, nside, ncomp, k, nmap, seed):
    rng = np.random.default_rng(seed)
    npix = 12 * nside**2
    t = dr._band_limited(oracle, rng, nside, 4, k, 0 if ncomp == 1 else 2) + 0.3 * rng.standard_normal((k, ncomp, npix))
    v = 0.5 + 0.5 * rng.random(npix)
    d = v * rng.standard_normal((nmap, ncomp, npix))
    return d, t, v


def _cleaned_bound(ref, d, t, v, K):
    """(per-pixel bound E (nmap, ncomp, npix), the bound of |da~| per map) from the docstring."""
    k, kappa = len(t), ref["cond"]
    dn = np.sqrt((d.reshape(len(d), -1) ** 2).sum(axis=1))
    c = 64 * k * U * kappa
    da = kappa * (np.sqrt(k) + k * np.sqrt(kappa)) * K * U * dn + c * np.sqrt(kappa) * dn
    f = v * t
    fn = np.sqrt(((f / np.sqrt(np.diag(ref["gram"]))[:, None, None]) ** 2).sum(axis=0))
    _, B = dr.apply(d, t, v, ref["alpha"])
    return da[:, None, None] * fn[None] + (k + 3) * U * B, c


@pytest.mark.parametrize("nside,ncomp,k,nmap", [(8, 1, 5, 1), (16, 2, 9, 2)])
def test_deproject_templates_end_to_end(oracle, nside, ncomp, k, nmap):
    import torch

    import heracles_amd as hx
    from heracles_amd import deprojection as dp

    d, t, v = _smooth_case(oracle, nside, ncomp, k, nmap, 300 + nside)
    ref = dr.deproject(d, t, v)
    assert ref["cond"] <= 100 and ref["rank"] == k, ref["cond"]  # a condition on the inputs
    K = gram_K(d[0].size, k + nmap)
    E, c = _cleaned_bound(ref, d, t, v, K)
    cleaned, info = hx.deproject_templates(d, t, v)
    assert isinstance(cleaned, np.ndarray) and cleaned.shape == d.shape
    r1 = float((np.abs(cleaned - ref["cleaned"]) / E).max())
    assert r1 <= 1, r1
    assert info.rank == k and info.dropped == () and info.alpha.shape == (nmap, k) and info.removed.shape == (nmap,)
    assert np.all(np.abs(info.gram - ref["gram"]) <= K * U * ref["A"][:k, :k])
    assert np.allclose(info.removed, np.einsum("mi,im->m", ref["alpha"], ref["r"]), rtol=1e-9)
    # F^T d_c by the Gram kernel
    g = dp.deproject_gram(list(np.ascontiguousarray(t)), list(np.ascontiguousarray(cleaned)), v)
    _, Ac = dr.gram(t, cleaned, v)
    dn = np.sqrt((d.reshape(nmap, -1) ** 2).sum(axis=1))
    En = np.sqrt((E.reshape(nmap, -1) ** 2).sum(axis=1))
    zb = K * U * Ac[:k, k:] + np.sqrt(np.diag(ref["gram"]))[:, None] * (En + c * dn)[None, :]
    r2 = float((np.abs(g[:k, k:]) / zb).max())
    assert r2 <= 1, r2
    # an injected contaminant goes
    beta = np.linspace(-3.0, 5.0, k)
    dirty = d + v * np.einsum("i,icp->cp", beta, t)[None]
    refd = dr.deproject(dirty, t, v)
    Ed, cd = _cleaned_bound(refd, dirty, t, v, K)
    got = hx.deproject_templates(dirty, t, v)[0]
    dirty_n = np.sqrt((dirty.reshape(nmap, -1) ** 2).sum(axis=1))
    assert np.all(np.abs(got - ref["cleaned"]) <= Ed + (cd * dirty_n)[:, None, None])
    # CUDA in, CUDA out; a DeviceArray keeps its metadata; out = the input works in place; a list of templates
    dt, tt, vt = torch.from_numpy(d).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(v).cuda()
    ct, _ = hx.deproject_templates(dt, tt, vt)
    assert ct.is_cuda and tuple(ct.shape) == d.shape and ct.cpu().numpy().tobytes() == cleaned.tobytes()
    da, _ = hx.deproject_templates(hx.DeviceArray(dt[0], {"spin": 0 if ncomp == 1 else 2, "nside": nside}), [x for x in tt], vt)
    assert isinstance(da, hx.DeviceArray) and da.dtype.metadata["nside"] == nside and da.shape == d[0].shape
    work = dt.clone()
    same, _ = hx.deproject_templates(work, tt, vt, out=work)
    assert same is work and work.cpu().numpy().tobytes() == cleaned.tobytes()
    one, _ = hx.deproject_templates(d[0, 0] if ncomp == 1 else d[0], t, v)
    assert one.shape == (d[0, 0] if ncomp == 1 else d[0]).shape
    print(f"deproject_templates nside {nside}, ncomp {ncomp}: cond {ref['cond']:.2f}, cleaned error / bound {r1:.3g}, F^T d_c / bound {r2:.3g}")


def test_duplicate_and_zero_templates_on_the_device(oracle):
    import heracles_amd as hx

    d, t, v = _smooth_case(oracle, 8, 1, 4, 1, 91)
    more = np.concatenate([t, t[2:3], np.zeros_like(t[:1])])
    a, ia = hx.deproject_templates(d, t, v)
    b, ib = hx.deproject_templates(d, more, v)
    assert (ia.rank, ia.dropped) == (4, ()) and (ib.rank, ib.dropped) == (4, (5,))
    assert np.abs(a - b).max() <= 1e-12 * np.abs(d).max()


# ---- hx_alm_apply_cl ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax", [0, 1, 33])
@pytest.mark.parametrize("nin,nout", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_alm_apply_cl(lmax, nin, nout):
    import torch

    from heracles_amd import deprojection as dp

    rng = np.random.default_rng(100 * lmax + 10 * nin + nout)
    nlm = (lmax + 1) * (lmax + 2) // 2
    cl = rng.standard_normal((nout, nin, lmax + 1))
    alm = rng.standard_normal((nin, nlm)) + 1j * rng.standard_normal((nin, nlm))
    want, A = dr.apply_cl(cl, alm)
    got = dp.alm_apply_cl(cl, alm)
    assert got.shape == (nout, nlm)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    assert np.all(err <= 3 * U * A)
    dev = dp.alm_apply_cl(torch.from_numpy(cl).cuda(), torch.from_numpy(alm).cuda())
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == got.tobytes()


# ---- the bias ----------------------------------------------------------------------------------------------------------------------------
class _Field:
    def __init__(self, spin, mask, mapper):
        self.spin, self.mask, self.mapper = spin, mask, mapper


@pytest.fixture(scope="module")
def mc(oracle):
    import heracles_amd as hx

    c = dr.MC
    s = dr.mc_setup(oracle)
    mapper = hx.HipHealpixMapper(c["nside"], c["lmax"], deconvolve=False, niter=c["niter"])
    fields = {"P": _Field(0, "VP", mapper), "G": _Field(2, "VG", mapper)}
    mask_maps = {("VP", 1): s["masks"][0], ("VG", 1): s["masks"][1]}
    cls = {key: hx.Result(arr, spin=(0 if key[0] == "P" else 2, 0 if key[1] == "P" else 2), axis=-1) for key, arr in s["blocks"].items()}
    return dict(s=s, fields=fields, mask_maps=mask_maps, cls=cls, mapper=mapper)


def _units(s):
    units = {}
    for name, spin, v in (("P", 0, s["masks"][0]), ("G", 2, s["masks"][1])):
        G, _ = dr.gram(s["templates"][name], np.zeros((0,) + s["templates"][name].shape[1:]), v)
        M, rank, _, cond = dr.pinv(G)
        assert rank == dr.MC["ntemp"] and cond <= 100
        units[name] = dict(spin=spin, v=v, f=s["templates"][name] * v, M=M)
    return units


def test_bias_matches_the_reference_formula(oracle, mc):
    import heracles_amd as hx

    c, s = dr.MC, mc["s"]
    npix = 12 * c["nside"] ** 2
    units = _units(s)
    # the infos as deproject_maps returns them (the maps do not matter for G^+)
    maps = {("P", 1): np.zeros(npix), ("G", 1): np.zeros((2, npix))}
    _, infos = hx.deproject_maps(mc["fields"], maps, s["templates"], mc["mask_maps"])
    got = hx.deprojection_bias(mc["cls"], mc["fields"], s["templates"], mc["mask_maps"], infos)
    e_f, e_g = 1e-10, 1e-10 + 2 * np.sqrt(npix) * 1e-11
    worst = 0.0
    for key in mc["cls"]:
        a, b = key[:2]
        da, db = (1 if a == "P" else 2), (1 if b == "P" else 2)
        want, T2, T4 = dr.bias(oracle, c["nside"], c["lmax"], c["niter"], units[a], units[b], s["blocks"][key].reshape(da, db, -1), with_scale=True)
        tol = (e_f + e_g) * T2 + (2 * e_f + e_g) * T4
        arr = np.asarray(got[key].array)
        assert arr.shape == s["blocks"][key].shape and got[key].spin == mc["cls"][key].spin
        worst = max(worst, float(np.abs(arr.reshape(want.shape) - want).max() / tol))
        assert np.abs(want).max() > 1e3 * tol  # the bound resolves the bias
    print(f"deprojection_bias: worst error / bound {worst:.3g}")
    assert worst <= 1
    # a field without templates drops its terms
    only_p = hx.deprojection_bias(mc["cls"], mc["fields"], {"P": s["templates"]["P"]}, mc["mask_maps"], infos, keys=[("P", "G", 1, 1)])
    want = dr.bias(oracle, c["nside"], c["lmax"], c["niter"], units["P"], dict(units["G"], f=None), s["blocks"]["P", "G", 1, 1].reshape(1, 2, -1))
    assert np.abs(np.asarray(only_p["P", "G", 1, 1].array) - want[0]).max() <= 1e-8 * np.abs(want).max()


def test_bias_passes_the_monte_carlo_check_on_the_device(mc):
    import torch

    import heracles_amd as hx

    c, s = dr.MC, mc["s"]
    nside, L, n = c["nside"], c["lmax"], c["nreal"]
    npix = 12 * nside**2
    plan = hx.get_plan(nside, L)
    packed = torch.from_numpy(s["cl"]).cuda()
    dpm = torch.empty((n, 1, npix), dtype=torch.float64, device="cuda")
    dgm = torch.empty((n, 2, npix), dtype=torch.float64, device="cuda")
    for r in range(n):
        alm = hx.synalm_components(packed, 3, seed=c["seed"], realisation=r)
        plan.alm2map(alm[:1], 0, out=dpm[r])
        plan.alm2map(alm[1:], 2, out=dgm[r])
    vp, vg = (torch.from_numpy(m).cuda() for m in s["masks"])
    dpm *= vp
    dgm *= vg
    tp, tg = torch.from_numpy(s["templates"]["P"]).cuda(), torch.from_numpy(s["templates"]["G"]).cuda()
    cp, ip = hx.deproject_templates(dpm, tp, vp)
    cg, ig = hx.deproject_templates(dgm, tg, vg)
    mapper = mc["mapper"]

    def vectors(pm, gm):
        out = np.empty((n, 7 * (L + 1)))
        for r0 in range(0, n, 12):
            m = min(12, n - r0)
            ap = mapper.transform(pm[r0 : r0 + m, 0].contiguous(), 0)
            ag = mapper.transform(gm[r0 : r0 + m].contiguous(), 2)
            comps, pairs = [], []
            for q in range(m):
                base = len(comps)
                comps += [ap[q], ag[q, 0], ag[q, 1]]
                pairs += [(base + x, base + y) for x, y in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2))]
            out[r0 : r0 + m] = np.asarray(hx.alm2cl_pairs(comps, pairs, L)).reshape(m, -1)
        return out

    delta = vectors(cp, cg) - vectors(dpm, dgm)
    infos = {("P", 1): ip, ("G", 1): ig}
    bias = hx.deprojection_bias(mc["cls"], mc["fields"], s["templates"], mc["mask_maps"], infos)
    vec = dr.mc_vector(bias["P", "P", 1, 1].array, bias["P", "G", 1, 1].array, bias["G", "G", 1, 1].array)
    zmax, zrms = dr.mc_statistic(delta, vec, L + 1, c["lmin"])
    zmax0, _ = dr.mc_statistic(delta, np.zeros_like(vec), L + 1, c["lmin"])
    print(f"Monte Carlo, device, n = {n}: max |z| = {zmax:.2f}, rms z = {zrms:.3f}; with the bias set to zero max |z| = {zmax0:.1f}")
    assert zmax0 > 6
    assert zmax <= 6, zmax
    assert 0.8 <= zrms <= 1.2, zrms


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_outputs_untouched():
    import heracles_amd as hx

    npix = 108
    rng = np.random.default_rng(8)
    t = [rng.standard_normal((1, npix)) for _ in range(4)]
    d = [rng.standard_normal((1, npix)) for _ in range(2)]
    v = rng.uniform(0, 1, npix)
    gram = np.full((6, 6), 7.0)

    def refused(rc, *words):
        assert rc == HX_ERR_ARG, (rc, _last_error())
        assert all(w in _last_error() for w in words), _last_error()
        assert np.all(gram == 7.0)

    refused(_gram_rc(t, d, v, gram, ncomp=3), "ncomp = 3")
    refused(_gram_rc(t, d, v, gram, npix=0), "npix")
    refused(_gram_rc(t, d, v, gram, ntemp=0, nmap=0), "0 columns")
    many = t * 256 + d[:1]
    refused(_gram_rc(many, [], v, np.full(4, 7.0)), "1025 columns")
    refused(_gram_rc(t, d, v, None), "null")
    refused(_gram_rc(t[:2] + [None] + t[3:], d, v, gram), "template 2")
    refused(_gram_rc(t, [d[0], None], v, gram), "map 1")
    bad = [x.copy() for x in t]
    bad[2][0, 17] = np.nan
    refused(_gram_rc(bad, d, v, gram), "template 2")
    inf = [x.copy() for x in d]
    inf[1][0, 5] = np.inf
    refused(_gram_rc(t, inf, v, gram), "map 1")
    refused(_gram_rc(t, inf, None, gram), "map 1")
    with pytest.raises(hx.HxError, match="template 2"):
        hx.deproject_templates(np.stack(d), np.stack(bad), v)
    # apply: overlapping outputs, wrong component count, null pointers
    alpha = rng.standard_normal((2, 4))
    store = np.full((3, 1, npix), 7.0)

    def refused_apply(rc, *words):
        assert rc == HX_ERR_ARG, (rc, _last_error())
        assert all(w in _last_error() for w in words), _last_error()
        assert np.all(store == 7.0)

    flat = store.reshape(-1)
    shifted = flat[npix // 2 : npix // 2 + npix].reshape(1, npix)
    refused_apply(_apply_rc(t, v, d, alpha, [store[0], shifted]), "overlap")
    refused_apply(_apply_rc(t, v, d, alpha, [store[0], store[0]]), "overlap")
    refused_apply(_apply_rc(t, v, [store[0], store[1]], alpha, [store[1], store[2]]), "overlap")  # out[0] is maps[1]
    refused_apply(_apply_rc(t, v, d, alpha, [store[0], t[1]]), "template 1")
    refused_apply(_apply_rc(t, v, d, alpha, [store[0], store[1]], ncomp=3), "ncomp = 3")
    refused_apply(_apply_rc(t, v, d, None, [store[0], store[1]]), "null")
    refused_apply(_apply_rc(t, v, d, alpha, [store[0], None]), "null")
    # alm_apply_cl
    L = hx._lib.load()
    alm = np.full(6, 7.0 + 0j)
    cl = np.ones((1, 1, 3))
    assert L.hx_alm_apply_cl(2, 1, 1, hx._lib.ptr(cl), hx._lib.ptr(alm), hx._lib.ptr(alm)) == HX_ERR_ARG and "overlap" in _last_error()
    assert L.hx_alm_apply_cl(2, 3, 1, hx._lib.ptr(cl), hx._lib.ptr(alm), hx._lib.ptr(np.empty(6, complex))) == HX_ERR_ARG
    assert L.hx_alm_apply_cl(2, 1, 1, None, hx._lib.ptr(alm), hx._lib.ptr(np.empty(6, complex))) == HX_ERR_ARG
    assert np.all(alm == 7.0)
    # wrong lengths and missing keys, before anything runs
    with pytest.raises(ValueError, match="template 1"):
        hx.deproject_templates(d[0], [t[0], np.ones((1, npix + 1))], v)
    with pytest.raises(ValueError, match="mask"):
        hx.deproject_templates(d[0], np.stack(t), v[:-1])
    with pytest.raises(ValueError, match="3 components"):
        hx.deproject_templates(np.ones((3, npix)), np.ones((1, 3, npix)))
    fields = {"P": _Field(0, "V", None)}
    with pytest.raises(KeyError, match=r"\('V', 1\)"):
        hx.deproject_maps(fields, {("P", 1): d[0][0]}, {"P": np.stack(t)[:, 0]}, {})
    with pytest.raises(KeyError, match="Q"):
        hx.deproject_maps(fields, {("P", 1): d[0][0]}, {"Q": np.stack(t)[:, 0]}, {("V", 1): v})


def test_flops_and_profile_names():
    import heracles_amd as hx
    from heracles_amd import deprojection as dp

    npix = 3072
    rng = np.random.default_rng(1)
    t, d = [rng.standard_normal((1, npix)) for _ in range(3)], [rng.standard_normal((1, npix))]
    hx._lib.executed_flops(reset=True)
    hx._lib.profile_enable(True)
    hx._lib.profile_reset()
    dp.deproject_gram(t, d, None)
    dp.deproject_apply(t, None, d, np.ones((1, 3)), [np.empty((1, npix))])
    mfma, _ = hx._lib.executed_flops(reset=True)
    hx._lib.profile_enable(False)
    assert mfma == (npix // 32) * 8 * 1 * 2048  # one tile, one slab, n = 4: stages x steps x (one live 16 x 16 block) x 2 * 16 * 16 * 4
    assert hx._lib.profile_get("deproject_gram")[0] >= 1 and hx._lib.profile_get("deproject_apply")[0] >= 1
