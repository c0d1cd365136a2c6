"""Golden vectors for the covariance estimators of DICES (heracles/dices/jackknife.py:449-593, heracles/dices/shrinkage.py:46-181).

Run ONCE in the build container (needs /root/reference; never on the GPU box):

    python tests/golden/make_golden_covariance.py

`heracles.dices.jackknife` / `heracles.dices.shrinkage` are imported through the bare-package shim of make_golden.py after
`coroutines`, `fitsio` and `healpy` are registered as empty modules (only the module headers of `..mapping` / `..io` import them;
the covariance functions never call them).  Only inputs and outputs are stored.

The reference's shrinkage_factor flattens the target in `list(set(keys))` order (heracles/utils.py:188-190) and the samples in
dict order.  The script runs itself under PYTHONHASHSEED=0 (so the file is reproducible bit for bit) and orders the spectra keys so
that the set order equals the dict order, and asserts it, before it stores lambda*: the file pins the reference's intended arithmetic,
not one hash seed's pairing.
"""

import importlib
import itertools
import os
import subprocess
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import key_str, ref_modules  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
NJK = 10
NELL = 5


def dices_modules():
    for name in ("coroutines", "fitsio", "healpy"):
        sys.modules.setdefault(name, types.ModuleType(name))
    h = ref_modules()
    h.jackknife = importlib.import_module("heracles.dices.jackknife")
    h.shrinkage = importlib.import_module("heracles.dices.shrinkage")
    return h


def spectra_keys(maps):
    return [(f1, f2, i1, i2) for (f1, i1), (f2, i2) in itertools.combinations_with_replacement(maps, 2)]


SPIN = {"POS": 0, "SHE": 2}


def shape_of(key, L):
    return tuple(2 for f in key[:2] if SPIN[f] == 2) + (L,)


def make_cls(h, rng, keys, L, ell_kw, base, scale, with_bias):
    """one spectra dict: base spectra times (1 + scale noise), bias metadata on the auto spectra"""
    out = {}
    for key in keys:
        arr = base[key] * (1.0 + scale * rng.standard_normal(base[key].shape))
        meta = {"nside": 8}
        if with_bias and key[0] == key[1] and key[2] == key[3]:
            meta["bias"] = float(base[key].reshape(-1)[0] * 0.1)
        h.core.update_metadata(arr, **meta)
        f1, f2 = key[:2]
        out[key] = h.result.Result(arr, spin=(SPIN[f1], SPIN[f2]), axis=-1, **ell_kw)
    return out


def base_spectra(rng, keys, L):
    ell = np.arange(L)
    base = {}
    for key in keys:
        shp = shape_of(key, L)
        auto = key[0] == key[1] and key[2] == key[3]
        amp = 1.0 if auto else 0.3
        arr = amp * (1.0 + 0.2 * rng.standard_normal(shp)) / (1.0 + ell) + (2.0 if auto else 0.0)
        if len(shp) == 3:  # spin-2 x spin-2: small off-diagonal (EB / BE) spectra
            arr[0, 1] *= 0.1
            arr[1, 0] *= 0.1
        base[key] = arr
    return base


def set_order(target):
    ks = [(k[0], k[1], k[4], k[5]) for k in target]
    return list(set(ks))


def plain(a):
    """the array without dtype metadata (which npz does not keep)"""
    return np.ascontiguousarray(a).view(np.float64) if np.asarray(a).dtype == np.float64 else np.asarray(a)


def store_dict(out, tag, d, with_ell=False):
    for key, res in d.items():
        out[f"{tag}/{key_str(key)}"] = plain(res.array)
        out[f"{tag}/spin/{key_str(key)}"] = np.asarray(res.spin)
        out[f"{tag}/axis/{key_str(key)}"] = np.asarray(res.axis)
        if with_ell:
            for n, e in enumerate(res.ell):
                out[f"{tag}/ell{n}/{key_str(key)}"] = np.asarray(e)


def main():
    h = dices_modules()
    jk, sh = h.jackknife, h.shrinkage
    rng = np.random.default_rng(53)
    out = {}

    # ---- case "a": POS x 2 bins, SHE x 2 bins, 5 unbinned l; 10 delete-1 and 45 delete-2 samples -----------------------------------
    # order the keys so that the reference's set order of the target's row keys is the dict order (see the module docstring):
    # start from the natural order and re-order by the set order until it is a fixed point; the tomographic bin labels are the
    # first pair (in a fixed scan) for which that iteration converges
    for b0, b1 in itertools.permutations(range(8), 2):
        maps = [("POS", b0), ("POS", b1), ("SHE", b0), ("SHE", b1)]
        keys = spectra_keys(maps)
        base = base_spectra(np.random.default_rng(53), keys, NELL)
        for _ in range(8):
            order = set_order(sh.gaussian_covariance(make_cls(h, rng, keys, NELL, {}, base, 0.0, True)))
            if order == keys:
                break
            keys = order
        else:
            continue
        break
    else:
        raise AssertionError("no key order found whose set order is the dict order")
    rng = np.random.default_rng(54)
    cls0 = make_cls(h, rng, keys, NELL, {}, base, 0.0, True)
    cls1 = {(k,): make_cls(h, rng, keys, NELL, {}, base, 0.05, True) for k in range(1, NJK + 1)}
    cls2 = {kk: make_cls(h, rng, keys, NELL, {}, base, 0.07, True) for kk in itertools.combinations(range(1, NJK + 1), 2)}
    out["a/keys"] = np.array([key_str(k) for k in keys])
    for k in keys:
        out[f"a/cls0/{key_str(k)}"] = plain(cls0[k].array)
        out[f"a/bias/{key_str(k)}"] = np.asarray((cls0[k].array.dtype.metadata or {}).get("bias", 0.0))
        out[f"a/cls1/{key_str(k)}"] = np.stack([plain(s[k].array) for s in cls1.values()])
        out[f"a/cls2/{key_str(k)}"] = np.stack([plain(s[k].array) for s in cls2.values()])
    out["a/regions1"] = np.array([kk[0] for kk in cls1])
    out["a/regions2"] = np.array(list(cls2))

    cov1 = jk.jackknife_covariance(cls1, nd=1)
    cov2 = jk.jackknife_covariance(cls2, nd=2)
    Q = jk.delete2_correction(cls0, cls1, cls2)
    deb = jk.debias_covariance(cov1, cls0, cls1, cls2)
    gauss = sh.gaussian_covariance(cls0)
    store_dict(out, "a/jk1", cov1, with_ell=True)
    store_dict(out, "a/jk2", cov2)
    store_dict(out, "a/q", Q)
    store_dict(out, "a/debias", deb)
    store_dict(out, "a/gauss", gauss, with_ell=True)

    # shrinkage factor: the target's set order must be the data order for the reference's pairing to be the intended one
    data_keys = list(next(iter(cls1.values())))
    fa, fb = h.utils.flatten(gauss), h.utils.flatten(gauss, order=data_keys)
    assert np.array_equal(fa, fb)
    lam = sh.shrinkage_factor(cls1, gauss)
    out["a/lambda"] = np.asarray(lam)
    store_dict(out, "a/shrink", sh.shrink(deb, gauss, lam))

    # ---- case "b": binned results (explicit ell / lower / upper / weight) pin the ell tuples of the outputs ---------------------------
    rng = np.random.default_rng(55)
    maps_b = [("POS", 0), ("SHE", 0)]
    keys_b = spectra_keys(maps_b)
    Lb = 4
    edges = np.array([2.0, 5.0, 9.0, 14.0, 20.0])
    ell_kw = {"ell": 0.5 * (edges[:-1] + edges[1:]), "lower": edges[:-1], "upper": edges[1:], "weight": np.ones(Lb)}
    base_b = base_spectra(rng, keys_b, Lb)
    cls1b = {(k,): make_cls(h, rng, keys_b, Lb, ell_kw, base_b, 0.05, True) for k in range(1, 6)}
    cls0b = make_cls(h, rng, keys_b, Lb, ell_kw, base_b, 0.0, True)
    out["b/keys"] = np.array([key_str(k) for k in keys_b])
    for k in ("ell", "lower", "upper", "weight"):
        out[f"b/{k}"] = ell_kw[k]
    for k in keys_b:
        out[f"b/cls0/{key_str(k)}"] = plain(cls0b[k].array)
        out[f"b/bias/{key_str(k)}"] = np.asarray((cls0b[k].array.dtype.metadata or {}).get("bias", 0.0))
        out[f"b/cls1/{key_str(k)}"] = np.stack([plain(s[k].array) for s in cls1b.values()])
    store_dict(out, "b/jk1", jk.jackknife_covariance(cls1b, nd=1), with_ell=True)
    store_dict(out, "b/gauss", sh.gaussian_covariance(cls0b), with_ell=True)

    path = os.path.join(OUT, "reference_covariance.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if os.environ.get("PYTHONHASHSEED") != "0":
        # a fresh child with a fixed string hash: the key order found above (and so the file) is reproducible
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)], env={**os.environ, "PYTHONHASHSEED": "0"}))
    main()
