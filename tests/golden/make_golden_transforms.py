"""Golden vectors of the Cl <-> xi transforms past one thread block, from the reference's own functions.

Run ONCE in the build container (needs /root/reference; never on the GPU box):

    python tests/golden/make_golden_transforms.py

``heracles.transforms._cl2corr`` / ``_corr2cl`` at lmax 300, 1024, 2048 (make_golden.py stops at 97), the dict-level ``cl2corr`` /
``corr2cl`` at lmax 256 and ``heracles.unmixing.naturalspice`` with data at lmax 256 and masks at lmax 512, through the bare-package
shim of make_golden.py.  Only inputs and outputs are stored -- no reference source text.

At these sizes element-wise parity with the reference cannot hold: its Gauss-Legendre weights (numpy ``leggauss``) are off by 9e-9
(n = 1025) to 7e-8 (n = 2049) relative at the end nodes, and xi has zero crossings.  So the fixture also stores, per array and column,
how far the CPU ORACLE (oracle/hx_oracle.c: the same formulas, long-double Newton nodes and weights) is from the reference, in the
norm that makes sense at size: ``max |d| / max |ref|`` for correlation functions, ``max |d| (1 + l)^2`` for the red spectra coming
back, and for naturalspice ``max |d| / max |ref|``.  The tests ask the oracle to stay within 1.5x of these (a stale oracle) and the GPU
within 8x.
"""

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from corr_reference import dev_back, dev_cl, dev_rel, dev_xi  # noqa: E402
from make_golden import key_str, ref_modules  # noqa: E402

KEYS = {("POS", "POS", 0, 0): (0, 0), ("POS", "SHE", 0, 0): (0, 2), ("SHE", "SHE", 0, 0): (2, 2)}
MASK_KEYS = (("VIS", "VIS", 0, 0), ("VIS", "WHT", 0, 0), ("WHT", "WHT", 0, 0))
L_DATA, L_MASK = 256, 512


def cap_legendre(theta_flat, theta_zero, lmax):
    """I_l = int m(x) P_l(x) dx of a polar cap that is 1 up to theta_flat degrees and falls to 0 at theta_zero with a cos^2 taper."""
    x, w = np.polynomial.legendre.leggauss(8192)
    th = np.degrees(np.arccos(x))
    t = np.clip((th - theta_flat) / (theta_zero - theta_flat), 0.0, 1.0)
    m = np.cos(0.5 * np.pi * t) ** 2
    return np.polynomial.legendre.legvander(x, lmax).T @ (w * m)


def stub_kernels(tr, um, ho):
    """heracles_amd's Python layer on the oracle (the stubs of tests/test_host_drivers.py::host_kernels)."""
    def batch(fn, specs, lmax):
        f = ho.cl2corr if fn.__name__ == "hx_cl2corr" else ho.corr2cl
        return np.stack([f(s, lmax) for s in specs])

    tr._batch = batch
    tr.gauss_legendre = ho.gauss_legendre
    um.gauss_legendre = ho.gauss_legendre


def main():
    from oracle import hxoracle as ho

    h = ref_modules()
    out = {}

    # ---- _cl2corr / _corr2cl (transforms.py:115-204) past one block ------------------------------------------------
    for lm in (300, 1024, 2048):
        rng = np.random.default_rng(lm)
        cls4 = rng.standard_normal((lm + 1, 4)) / (1 + np.arange(lm + 1))[:, None] ** 2
        corr = h.transforms._cl2corr(cls4)
        back = h.transforms._corr2cl(corr)
        xv, wv = h.transforms._cached_gauss_legendre(lm + 1)
        out[f"c2c/{lm}/cls"], out[f"c2c/{lm}/corr"], out[f"c2c/{lm}/cls_back"] = cls4, corr, back
        out[f"c2c/{lm}/x"], out[f"c2c/{lm}/w"] = xv, wv
        out[f"c2c/{lm}/dev_corr"] = dev_xi(ho.cl2corr(cls4), corr)
        out[f"c2c/{lm}/dev_back"] = dev_cl(ho.corr2cl(corr), back)
        ox, ow = ho.gauss_legendre(lm + 1)
        print(f"lmax {lm}: oracle vs reference: xi {out[f'c2c/{lm}/dev_corr']}, cl back {out[f'c2c/{lm}/dev_back']}, "
              f"nodes {np.abs(ox - xv).max():.1e}, weights {np.abs(ow / wv - 1).max():.1e}")

    # ---- dict-level cl2corr / corr2cl / naturalspice (transforms.py:207-363, unmixing.py:36-102) --------------------
    Result = h.result.Result
    rng = np.random.default_rng(256)
    ell, ellm = np.arange(L_DATA + 1), np.arange(L_MASK + 1)
    shapes = {k: (2,) * sum(1 for s in spin if s) for k, spin in KEYS.items()}
    d = {}
    for k, shp in shapes.items():
        arr = rng.standard_normal(shp + (L_DATA + 1,)) / (1 + ell) ** 2
        if shp:
            arr[..., :2] = 0.0
        d[k] = Result(arr, spin=KEYS[k], axis=-1, ell=ell)
        out[f"dict/d/{key_str(k)}"] = arr
    wd = h.transforms.cl2corr(d)
    back = h.transforms.corr2cl(wd)
    iv, iw = cap_legendre(30.0, 40.0, L_MASK), cap_legendre(38.0, 50.0, L_MASK)
    mcl = {MASK_KEYS[0]: np.pi * iv * iv, MASK_KEYS[1]: np.pi * iv * iw, MASK_KEYS[2]: np.pi * iw * iw}
    for k, arr in mcl.items():
        out[f"ns/m/{key_str(k)}"] = arr
    fields = {"POS": types.SimpleNamespace(mask="VIS", spin=0), "SHE": types.SimpleNamespace(mask="WHT", spin=2)}
    ns = {}
    for tag, tm in (("default", None), ("theta30", 30.0)):
        # naturalspice mutates the mask correlation functions in place -> fresh copies
        m = {k: Result(np.array(v), spin=(0, 0), axis=-1, ell=ellm) for k, v in mcl.items()}
        ns[tag] = h.unmixing.naturalspice(d, m, fields, theta_max=tm)

    # the same through heracles_amd's Python layer on the oracle: the deviations the tests scale
    import heracles_amd as hx
    from heracles_amd import transforms as tr, unmixing as um

    stub_kernels(tr, um, ho)
    d2 = {k: hx.Result(np.array(v.array), spin=KEYS[k], axis=-1, ell=ell) for k, v in d.items()}
    wd2 = hx.cl2corr(d2)
    back2 = hx.corr2cl({k: hx.Result(np.array(wd[k].array), spin=KEYS[k], axis=-1, ell=wd2[k].ell) for k in d})
    for k in d:
        ks = key_str(k)
        out[f"dict/wd/{ks}"], out[f"dict/back/{ks}"] = np.asarray(wd[k].array), np.asarray(back[k].array)
        out[f"dict/dev_wd/{ks}"] = np.array(dev_rel(wd2[k].array, out[f"dict/wd/{ks}"]))
        out[f"dict/dev_back/{ks}"] = np.array(dev_back(back2[k].array, out[f"dict/back/{ks}"]))
        print(f"dict {ks}: oracle vs reference: xi {out[f'dict/dev_wd/{ks}']:.2e}, cl back (1+l)^2 {out[f'dict/dev_back/{ks}']:.2e}")
    for tag, tm in (("default", None), ("theta30", 30.0)):
        m = {k: hx.Result(np.array(v), spin=(0, 0), axis=-1, ell=ellm) for k, v in mcl.items()}
        res = hx.naturalspice(d2, m, fields, theta_max=tm)
        for k in d:
            ks = key_str(k)
            ref = np.asarray(ns[tag][k].array)
            out[f"ns/{tag}/{ks}"] = ref
            out[f"ns/dev_{tag}/{ks}"] = np.array(dev_rel(res[k].array, ref))
            ok = np.allclose(res[k].array, ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max())
            print(f"naturalspice {tag} {ks}: oracle path vs reference max |d| / max |ref| = {out[f'ns/dev_{tag}/{ks}']:.2e}; "
                  f"rtol 1e-6, atol 1e-9 max|ref| {'holds' if ok else 'DOES NOT HOLD'}")

    path = os.path.join(HERE, "reference_transforms.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {len(out)} arrays to reference_transforms.npz ({os.path.getsize(path) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
