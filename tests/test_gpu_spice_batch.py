"""The batched NaturalSpice path on the kernels: naturalspice_batch, correct_footprint_naturalspice_batch and
jackknife_cls(..., mask_correction="Full", batched=True) -- columns of all samples through hx_cl2corr_cols, hx_xi_ratio and
hx_corr2cl_cols -- against the reference's own vectors and against the per-sample functions.  The plan and the executor run on a
numpy backend in tests/test_spice_plan_host.py."""

import os
import types

import numpy as np
import pytest

import corr_reference as cr
from helpers import key_str

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = {"POS": types.SimpleNamespace(mask="VIS", spin=0), "SHE": types.SimpleNamespace(mask="WHT", spin=2)}
SPINS = {("POS", "POS", 0, 0): (0, 0), ("POS", "SHE", 0, 0): (0, 2), ("SHE", "SHE", 0, 0): (2, 2)}
MKEYS = (("VIS", "VIS", 0, 0), ("VIS", "WHT", 0, 0), ("WHT", "WHT", 0, 0))


def test_naturalspice_batch_reference_vectors():
    """Three samples (the fixture's d, the same again, 2 d) with masks at twice the data's band limit: equal samples agree to the bit,
    the doubled sample is exactly twice the first (a power of two scales every product and sum exactly: crossed batch slots would
    show), and every sample is within 8x the oracle path's deviation from the reference's ns/default and ns/theta30."""
    import heracles_amd as hx

    g = np.load(os.path.join(HERE, "golden", "reference_transforms.npz"))
    Ld, Lm = 256, 512
    ell, ellm = np.arange(Ld + 1), np.arange(Lm + 1)
    d = {k: hx.Result(np.array(g[f"dict/d/{key_str(k)}"]), spin=s, axis=-1, ell=ell) for k, s in SPINS.items()}
    d2 = {k: hx.Result(2 * np.array(g[f"dict/d/{key_str(k)}"]), spin=s, axis=-1, ell=ell) for k, s in SPINS.items()}
    failures = []
    for tag, tm in (("default", None), ("theta30", 30.0)):
        m = {k: hx.Result(np.array(g[f"ns/m/{key_str(k)}"]), spin=(0, 0), axis=-1, ell=ellm) for k in MKEYS}
        res = hx.naturalspice_batch({1: d, 2: d, 3: d2}, m, FIELDS, theta_max=tm)
        assert list(res) == [1, 2, 3]
        for k in MKEYS:
            np.testing.assert_array_equal(m[k].array, g[f"ns/m/{key_str(k)}"])  # the masks are not damped in place
        chunked = hx.naturalspice_batch({1: d, 2: d, 3: d2}, m, FIELDS, theta_max=tm, max_columns=7)
        for k in d:
            ks = key_str(k)
            assert list(res[1]) == list(d) and type(res[1][k]) is hx.Result and res[1][k].spin == SPINS[k]
            np.testing.assert_array_equal(res[1][k].ell, ell)
            np.testing.assert_array_equal(res[2][k].array, res[1][k].array)
            np.testing.assert_array_equal(res[3][k].array, 2 * res[1][k].array)
            for i in res:
                np.testing.assert_array_equal(chunked[i][k].array, res[i][k].array)
                ref = g[f"ns/{tag}/{ks}"] * (2 if i == 3 else 1)
                a = cr.dev_rel(res[i][k].array, ref)
                print(f"naturalspice_batch {tag} sample {i} {ks}: max |d| / max |ref| {a:.2e} (oracle {g[f'ns/dev_{tag}/{ks}']:.2e})")
                if not a <= 8 * g[f"ns/dev_{tag}/{ks}"]:
                    failures.append(f"naturalspice_batch {tag} sample {i} {ks}: {a:.3e} > 8 * {g[f'ns/dev_{tag}/{ks}']:.3e}")
    hx.release_caches()
    assert not failures, "\n".join(failures)


def test_footprint_correction_batch_reference_golden():
    """correct_footprint_naturalspice_batch against reference_jackknife.npz, mixed and unmixed, at the tolerance recorded for this
    composition (tests/test_gpu_jackknife.py::test_full_footprint_correction_against_reference_golden); two samples, the second with
    doubled data: exactly twice the first."""
    import heracles_amd as hx

    g = np.load(os.path.join(HERE, "golden", "reference_jackknife.npz"))
    ks = lambda key: "|".join(str(k) for k in key)  # noqa: E731

    def spectra(group, spins, scale=1):
        return {k: hx.Result(scale * np.array(g[f"{group}/{ks(k)}"]), spin=s, axis=-1, ell=np.arange(g[f"{group}/{ks(k)}"].shape[-1]))
                for k, s in spins.items()}

    mspins = {k: (0, 0) for k in MKEYS}
    for tag, unmixed in (("mixed", False), ("unmixed", True)):
        cls, cls2 = spectra("cls", SPINS), spectra("cls", SPINS, 2)
        got = hx.correct_footprint_naturalspice_batch({"a": cls, "b": cls2}, {"a": spectra("mljk", mspins), "b": spectra("mljk", mspins)},
                                                      spectra("mls0", mspins), FIELDS, unmixed=unmixed)
        assert list(got) == ["a", "b"] and list(got["a"]) == list(SPINS)
        for k in SPINS:
            ref = g[f"{tag}/out/{ks(k)}"]
            np.testing.assert_allclose(np.asarray(got["a"][k].array), ref, rtol=1e-7, atol=1e-10 * np.abs(ref).max())
            np.testing.assert_array_equal(got["b"][k].array, 2 * got["a"][k].array)


# ---- the jackknife loop: a small set-up like tests/test_gpu_jackknife.py::_setup ---------------------------------------------------
NSIDE, LMAX, NJK = 16, 24, 4


def _setup(rng):
    import heracles_amd as hx

    npix = 12 * NSIDE**2
    mapper = hx.HipHealpixMapper(NSIDE, LMAX, deconvolve=False, niter=0)
    # mask keys follow the field's mask name in the reference; here data and visibility maps share their keys
    fields = {"POS": types.SimpleNamespace(spin=0, mapper_or_error=mapper, mask="POS"),
              "SHE": types.SimpleNamespace(spin=2, mapper_or_error=mapper, mask="SHE")}
    jk = np.zeros(npix)
    theta = np.arccos(1 - 2 * (np.arange(npix) + 0.5) / npix)
    footprint = theta < 2.0
    jk[footprint] = 1 + (np.arange(npix)[footprint] % NJK)
    maps, vis = {}, {}
    for name, bins in (("POS", (1, 2)), ("SHE", (1,))):
        for b in bins:
            m = rng.standard_normal(((2,) if name == "SHE" else ()) + (npix,)) * footprint
            md = {"spin": fields[name].spin, "nside": NSIDE, "kernel": "healpix", "fsky": 0.4, "musq": 1.3 + b, "dens": 2.5}
            m = np.ascontiguousarray(m)
            m.dtype = np.dtype(m.dtype, metadata=md)
            maps[name, b] = m
            v = (jk > 0).astype(float) * (1.0 + 0.1 * b)
            v = np.ascontiguousarray(np.stack([v, 0 * v]) if name == "SHE" else v)
            v.dtype = np.dtype(v.dtype, metadata={"spin": fields[name].spin, "nside": NSIDE})
            vis[name, b] = v
    return fields, maps, vis, jk


@pytest.fixture(scope="module")
def jackknife_runs():
    """Per nd: the per-sample loop, the batch in one chunk, and the batch cut into at least three chunks; computed once."""
    import heracles_amd as hx

    fields, maps, vis, jk = _setup(np.random.default_rng(79))
    runs = {}
    for nd in (1, 2):
        loop = hx.jackknife_cls(maps, vis, jk, fields, mask_correction="Full", nd=nd)
        one = hx.jackknife_cls(maps, vis, jk, fields, mask_correction="Full", nd=nd, batched=True)
        # 11 data columns per sample (3 POS x POS keys, 2 POS x SHE keys, 1 SHE x SHE key): 4 samples one by one, 6 samples in pairs
        chunks = hx.jackknife_cls(maps, vis, jk, fields, mask_correction="Full", nd=nd, batched=True, max_columns=11 * nd)
        runs[nd] = (loop, one, chunks)
    return runs


@pytest.mark.parametrize("nd", [1, 2])
def test_jackknife_cls_batched_full_correction(jackknife_runs, nd):
    """batched=True against the per-sample loop at the tolerance of the composition (rtol 1e-7, atol 1e-10 max |ref|): same regions, keys,
    key order, Result fields and metadata (the `bias` of correct_bias among it); the chunked run is the one-chunk run to the bit."""
    from dataclasses import fields as dc_fields
    from itertools import combinations

    loop, one, chunks = jackknife_runs[nd]
    combos = list(combinations(range(1, NJK + 1), nd))
    assert list(loop) == combos and list(one) == combos and list(chunks) == combos
    nsamp = len(combos)
    assert -(-nsamp // nd) >= 3, "the chunked run must take at least three chunks"
    for regions in combos:
        assert list(one[regions]) == list(loop[regions])
        for key, ref in loop[regions].items():
            got = one[regions][key]
            a, r = np.asarray(got.array), np.asarray(ref.array)
            assert a.shape == r.shape and a.dtype == r.dtype and a.dtype.metadata == r.dtype.metadata, (regions, key)
            np.testing.assert_allclose(a, r, rtol=1e-7, atol=1e-10 * np.nanmax(np.abs(r)))
            np.testing.assert_array_equal(np.asarray(chunks[regions][key].array), a)
            assert np.asarray(chunks[regions][key].array).dtype.metadata == a.dtype.metadata
            for f in dc_fields(ref):
                if f.name == "array":
                    continue
                x, y = getattr(got, f.name), getattr(ref, f.name)
                if isinstance(y, np.ndarray) or isinstance(x, np.ndarray):
                    np.testing.assert_array_equal(x, y, err_msg=f.name)
                else:
                    assert x == y, f.name
    md = loop[combos[0]]["POS", "POS", 1, 1].array.dtype.metadata
    print(f"nd {nd}: {nsamp} samples, metadata of POS x POS (1, 1) after the Full correction: {md}")
